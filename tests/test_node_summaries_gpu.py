"""swz_node_summaries_device against tests/summary_ref.py, compared exactly.  One table holds every edge the kernel has, placed
by T = node_summaries_tile(): nodes of one row, T one-row nodes filling one tile (a full window), a run across lanes 63 / 64, a
node that starts on the last row of a tile and runs over more than two tiles, empty nodes in between, rows that belong to no
node.  The rows of no node hold the extremes (0, 65535, 255, NaN) that no neighbouring node may show.  uint16 values reach 0 and
65535; GPS times hold NaN, +-inf and +-0.0, and one node's times are all NaN; scan angles hold -128, -1 and 127."""
import numpy as np
import pytest

import filter_ref as F
import summary_ref as S
import schwarzwald_amd as swz

pytestmark = pytest.mark.gpu
ERR_BAD_ARG = 2


def _table(T):
    nodes = []  # (offset, count, why)
    at = 0

    def add(count, why, gap=0):
        nonlocal at
        at += gap
        nodes.append((at, count, why))
        at += count

    add(0, "empty at the front")
    add(1, "one row", gap=3)
    add(58, "all NaN, ends in front of lane 63")
    add(5, "crosses lanes 63 / 64")
    add(T - 67 - 1, "ends one row in front of the tile's last")
    add(1, "the last row of tile 0")
    assert at == T
    add(0, "empty in the middle")
    for _ in range(T):
        add(1, "one of T one-row nodes filling tile 1")
    assert at == 2 * T
    add(T - 1 - 7, "behind a gap", gap=7)
    assert at == 3 * T - 1
    add(2 * T + 5, "starts on the last row of tile 2, runs over tiles 3 and 4 into 5")
    add(0, "empty behind the long node")
    add(2, "two rows", gap=1)
    add(0, "empty at the end")
    n = at + 6
    return (np.array([o for o, _, _ in nodes], dtype=np.uint64), np.array([c for _, c, _ in nodes], dtype=np.uint64), [w for _, _, w in nodes], n)


def _columns(n, off, cnt, why, rng):
    in_node = np.zeros(n, bool)
    for o, c in zip(off, cnt):
        in_node[int(o):int(o + c)] = True
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, -1e300, 5e-324, -5e-324, 1.0, -1.0])
    gps = np.where(rng.random(n) < 0.3, rng.choice(special, n), rng.standard_normal(n) * 1e5)
    cols = {"intensity": rng.integers(1, 65534, n, endpoint=True).astype(np.uint16), "classification": rng.choice([2, 3, 5, 6, 9, 64, 65, 200], n).astype(np.uint8),
            "edge_of_flight_line": rng.integers(0, 1, n, endpoint=True).astype(np.uint8), "gps_time": gps,
            "number_of_returns": rng.integers(1, 7, n, endpoint=True).astype(np.uint8), "return_number": rng.integers(1, 7, n, endpoint=True).astype(np.uint8),
            "point_source_id": rng.integers(1, 300, n, endpoint=True).astype(np.uint16), "scan_direction_flag": np.ones(n, np.uint8),
            "scan_angle_rank": rng.integers(-90, 90, n, endpoint=True).astype(np.int8), "user_data": rng.integers(0, 254, n, endpoint=True).astype(np.uint8)}
    node = {w: k for k, w in enumerate(why)}
    rows = lambda w: slice(int(off[node[w]]), int(off[node[w]] + cnt[node[w]]))  # noqa: E731
    cols["gps_time"][rows("all NaN, ends in front of lane 63")] = np.nan
    long_rows = rows("starts on the last row of tile 2, runs over tiles 3 and 4 into 5")
    first, last = long_rows.start, long_rows.stop - 1
    cols["gps_time"][first], cols["gps_time"][last] = -np.inf, np.inf          # the extremes sit in tile 2 and in tile 5
    cols["gps_time"][first + 1] = np.nan
    cols["intensity"][first], cols["intensity"][last] = 0, 65535
    cols["point_source_id"][last - 1], cols["point_source_id"][first + 2] = 0, 65535
    cols["scan_angle_rank"][first], cols["scan_angle_rank"][last], cols["scan_angle_rank"][first + 300] = -128, 127, -1
    cross = rows("crosses lanes 63 / 64")
    cols["scan_angle_rank"][cross] = [-1, -128, 127, -1, 0]
    cols["gps_time"][cross] = [0.0, -0.0, 0.0, -0.0, -0.0]
    cols["intensity"][cross] = [65535, 7, 7, 7, 0]
    two = rows("two rows")
    cols["gps_time"][two] = [np.inf, np.inf]
    # the rows of no node hold what no node may show
    out = ~in_node
    cols["intensity"][out] = np.where(np.arange(out.sum()) % 2 == 0, 0, 65535)
    cols["point_source_id"][out] = 65535
    cols["user_data"][out] = 255
    cols["scan_direction_flag"][out] = 0
    cols["classification"][out] = 255
    return cols


@pytest.fixture(scope="module")
def case():
    import torch
    T = swz.node_summaries_tile()
    off, cnt, why, n = _table(T)
    rng = np.random.default_rng(6021)
    cols = _columns(n, off, cnt, why, rng)
    want = S.summaries(cols, F.SCALARS, off, cnt)                # computed once, shared, never changed
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(v.view(np.uint8) if v.dtype == np.int8 else v.view(np.int16) if v.dtype == np.uint16 else v).to(dev) for k, v in cols.items()}
    torch.cuda.synchronize()
    return dict(T=T, off=off, cnt=cnt, why=why, n=n, cols=cols, want=want, d=d, ptrs={k: v.data_ptr() for k, v in d.items()})


def test_the_case_is_what_it_is_meant_to_be(case):
    T, cnt, want = case["T"], case["cnt"], case["want"]
    names = S.ordered(F.SCALARS)
    assert (cnt == 1).sum() >= T + 2 and (cnt > 2 * T).any() and (cnt == 0).sum() >= 4 and case["n"] > 5 * T
    gps, inten, angle = want[:, names.index("gps_time")], want[:, names.index("intensity")], want[:, names.index("scan_angle_rank")]
    assert ((gps["flags"] == 1) & np.isposinf(gps["lo"]) & np.isneginf(gps["hi"]) & (cnt > 1)).any(), "no node whose times are all NaN"
    assert (np.isneginf(gps["lo"]) & np.isposinf(gps["hi"]) & (gps["flags"] == 1)).any()
    assert (np.isposinf(gps["lo"]) & np.isposinf(gps["hi"])).any(), "no node whose only time is +inf"
    assert ((gps["lo"] == 0) & (gps["hi"] == 0)).any()
    assert ((inten["lo"] == 0) & (inten["hi"] == 65535)).sum() == 2
    assert ((angle["lo"] == -128) & (angle["hi"] == 127)).sum() >= 2
    user = want[:, names.index("user_data")]
    assert not ((user["set"][:, 3] >> np.uint64(63)) & np.uint64(1)).any(), "a node shows the byte of the rows of no node"


MASKS = [F.SCALARS] + [(name,) for name in F.SCALARS]


@pytest.mark.parametrize("names", MASKS, ids=lambda m: "all" if len(m) > 1 else m[0])
def test_summaries_are_the_reference_exactly(case, names):
    pick = [S.ordered(F.SCALARS).index(k) for k in S.ordered(names)]
    want = case["want"][:, pick]
    nodes = dict(offset=case["off"], count=case["cnt"])
    with swz.Context(0) as ctx:
        images = []
        for poison in ("1", "255"):  # the result does not depend on what the workspace held
            ctx.release_workspace()
            ctx.set_option("SWZ_POISON", poison)
            # every column is handed over, the mask chooses
            got = ctx.node_summaries_device(case["n"], case["ptrs"], nodes, attrs=names)
            assert got.shape == want.shape and got.dtype == S.DTYPE
            for k, why in enumerate(case["why"]):
                assert S.same(got[k], want[k]), (why, poison, got[k], want[k])
            assert (got["reserved"] == 0).all()
            images.append(got.tobytes())
        assert images[0] == images[1]
        empty = case["cnt"] == 0
        assert np.isposinf(got[empty]["lo"]).all() and np.isneginf(got[empty]["hi"]).all() and not got[empty]["set"].any()


def test_nothing_to_reduce_launches_nothing(case):
    u = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    ptrs, n = case["ptrs"], case["n"]

    def preset(got, shape):
        return got.shape == shape and np.isposinf(got["lo"]).all() and np.isneginf(got["hi"]).all() and not got["set"].any() and not got["flags"].any()

    with swz.Context(0) as ctx:
        ctx.profile_enable(True)
        assert preset(ctx.node_summaries_device(0, {}, dict(offset=u(), count=u()), attrs=F.SCALARS), (0, 10))
        assert preset(ctx.node_summaries_device(0, {}, dict(offset=u(0, 0), count=u(0, 0)), attrs=F.SCALARS), (2, 10))     # n == 0: no columns needed
        assert preset(ctx.node_summaries_device(n, ptrs, dict(offset=u(), count=u())), (0, 10))
        assert preset(ctx.node_summaries_device(n, ptrs, dict(offset=u(5, 9), count=u(0, 0))), (2, 10))
        assert preset(ctx.node_summaries_device(n, ptrs, dict(offset=u(0, 10), count=u(10, 5)), attrs=()), (2, 0))          # an empty mask
        assert "node_summaries" not in ctx.profile_get()


def test_refusals_come_before_anything_is_launched(case):
    u = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    ptrs, n = case["ptrs"], case["n"]
    good = dict(offset=u(0, 10), count=u(10, 5))
    without = {k: v for k, v in ptrs.items() if k != "gps_time"}
    cases = [("node offsets are not ascending", n, ptrs, dict(offset=u(10, 0), count=u(5, 10)), None),
             ("node ranges overlap", n, ptrs, dict(offset=u(0, 9), count=u(10, 5)), None),
             ("a node range passes the last row", n, ptrs, dict(offset=u(0, n - 2), count=u(10, 3)), None),
             ("a node range passes the last row", n, ptrs, dict(offset=u(0, 16), count=u(10, 2 ** 64 - 8)), None),
             ("more than 2^32-65536 rows", 2 ** 32 - 65535, ptrs, good, None),
             ("the mask names SWZ_ATTR_GPS_TIME, which has no input column", n, without, good, F.SCALARS),
             ("SWZ_ATTR_RGB is not a scalar column", n, ptrs, good, 1 | swz.SUMMARY_SCALARS),
             ("SWZ_ATTR_NORMAL is not a scalar column", n, ptrs, good, 2),
             ("a bit of the mask that names no attribute", n, ptrs, good, 1 << 12),
             ("the column of SWZ_ATTR_INTENSITY is not aligned to its element", n, dict(ptrs, intensity=ptrs["intensity"] + 1), good, None),
             ("the column of SWZ_ATTR_GPS_TIME is not aligned to its element", n, dict(ptrs, gps_time=ptrs["gps_time"] + 4), good, None)]
    with swz.Context(0) as ctx:
        ctx.profile_enable(True)
        for words, rows, columns, nodes, attrs in cases:
            with pytest.raises(swz.SwzError) as e:
                ctx.node_summaries_device(rows, columns, nodes, attrs=attrs)
            assert e.value.code == ERR_BAD_ARG and "swz_node_summaries_device" in str(e.value) and words in str(e.value), (words, str(e.value))
        assert "node_summaries" not in ctx.profile_get()
        # the context takes a valid call afterwards
        got = ctx.node_summaries_device(n, ptrs, good)
        assert S.same(got, S.summaries(case["cols"], F.SCALARS, good["offset"], good["count"]))
        assert ctx.profile_get()["node_summaries"]["launches"] == 2
