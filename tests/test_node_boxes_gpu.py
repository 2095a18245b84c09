"""swz_node_boxes_device against numpy min / max with exact ==.  One table holds every edge the kernel has, placed by
T = node_boxes_tile(): nodes of one row, nodes that end and start on the last row of a tile, a node over more than three
tiles, T one-row nodes filling one tile, a run across lanes 63 / 64 of a wave, empty nodes at the front, in the middle and at
the end, rows that belong to no node.  The values mix signs, +-1e300, denormals, repeated values and a constant axis; one
node is all-negative, others straddle zero: the negative half of the double ordering is where an integer code of a double
goes wrong."""
import numpy as np
import pytest

import schwarzwald_amd as swz

ERR_BAD_ARG = 2


def _table(T):
    """(offset, count) per node and what each node is there for; rows in gaps belong to no node"""
    nodes = []  # (offset, count, why)
    at = 0

    def add(count, why, gap=0):
        nonlocal at
        at += gap
        nodes.append((at, count, why))
        at += count

    add(0, "empty at the front")
    add(0, "empty at the front, twice")
    add(1, "one row", gap=3)                       # rows 0..2 belong to no node
    add(58, "ends in front of lane 63")            # rows 4..61
    add(5, "crosses lanes 63 / 64")                # rows 62..66
    add(T - 67 - 1, "ends one row in front of the tile's last")
    add(1, "the last row of tile 0: starts and ends on it")
    assert at == T
    add(0, "empty in the middle")
    for i in range(T):
        add(1, "one of T one-row nodes filling tile 1")
    assert at == 2 * T
    add(T - 1 - 7, "ends in front of a gap", gap=7)  # tile 2 begins with rows of no node
    assert at == 3 * T - 1
    add(3 * T + 5, "starts on the last row of tile 2, runs over tiles 3, 4, 5 into 6")
    add(0, "empty behind the long node")
    add(2, "two rows", gap=1)
    add(0, "empty at the end")
    add(0, "empty at the end, twice")
    n = at + 6                                     # rows behind the last node belong to no node either
    off = np.array([o for o, _, _ in nodes], dtype=np.uint64)
    cnt = np.array([c for _, c, _ in nodes], dtype=np.uint64)
    return off, cnt, [w for _, _, w in nodes], n


def _values(rows, rng):
    special = np.array([0.0, -0.0, 1e300, -1e300, 5e-324, -5e-324, 2.5e-310, -2.5e-310, 1.0, -1.0, 3.5, -3.5, 1e-300, -1e-300,
                        np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)])
    xyz = np.where(rng.random((rows, 3)) < 0.4, rng.choice(special, size=(rows, 3)), rng.standard_normal((rows, 3)) * 10.0 ** rng.integers(-5, 6, (rows, 3)))
    xyz[:, 1] = -7.25  # a constant axis
    return np.ascontiguousarray(xyz, dtype=np.float64)


def _host_case():
    T = swz.node_boxes_tile()
    off, cnt, why, n = _table(T)
    assert n >= 4 * T + 7
    rng = np.random.default_rng(20240607)
    pool = n + 100                                  # the pool is larger than what the table reaches
    xyz = _values(pool, rng)
    perm = rng.permutation(pool).astype(np.uint32)[:n + 50]
    order = rng.permutation(n + 50).astype(np.uint32)[:n]
    # the nodes named for it: all-negative, and straddling zero, whatever the draw
    src_plain, src_order = perm[:n], perm[order]
    neg = next(k for k, w in enumerate(why) if w == "ends in front of lane 63")
    for src in (src_plain, src_order):
        rows = src[int(off[neg]):int(off[neg] + cnt[neg])]
        xyz[rows, 0] = -np.abs(xyz[rows, 0]) - 1e-320
        xyz[rows, 2] = -np.abs(xyz[rows, 2]) - 5e-324
    long_node = next(k for k, w in enumerate(why) if w.startswith("starts on the last row"))
    rows = src_plain[int(off[long_node]):int(off[long_node] + cnt[long_node])]
    xyz[rows[0], 0], xyz[rows[-1], 0] = -1e300, 1e300  # the extremes sit on its first and last row: tile 2 and tile 6
    return dict(T=T, off=off, cnt=cnt, why=why, n=n, xyz=xyz, perm=perm, order=order)


@pytest.fixture(scope="module")
def case():
    import torch
    S = _host_case()
    xyz, perm, order = S["xyz"], S["perm"], S["order"]
    dev = torch.device("cuda:0")
    d = dict(xyz=torch.from_numpy(xyz).to(dev), perm=torch.from_numpy(perm.view(np.int32)).to(dev),
             order=torch.from_numpy(order.view(np.int32)).to(dev))
    torch.cuda.synchronize()
    return dict(S, d=d)


def _expected(xyz, src, off, cnt):
    lo = np.full((len(off), 3), np.inf)
    hi = np.full((len(off), 3), -np.inf)
    for k in range(len(off)):
        if cnt[k]:
            rows = xyz[src[int(off[k]):int(off[k] + cnt[k])]]
            lo[k], hi[k] = rows.min(axis=0), rows.max(axis=0)
    return lo, hi


@pytest.mark.gpu
@pytest.mark.parametrize("with_order", [False, True])
def test_boxes_are_numpy_min_max_exactly(case, with_order):
    S = case
    d = S["d"]
    src = S["perm"][S["order"]] if with_order else S["perm"][:S["n"]]
    want_lo, want_hi = _expected(S["xyz"], src, S["off"], S["cnt"])
    # the data is what the docstring says: an all-negative node, nodes that straddle zero, a long node over four tiles
    assert any((want_hi[k] < 0)[[0, 2]].all() for k in range(len(S["off"])) if S["cnt"][k] > 1)
    assert any(want_lo[k][0] < 0 < want_hi[k][0] for k in range(len(S["off"])))
    assert (S["cnt"] > 3 * S["T"]).any() and (S["cnt"] == 0).sum() >= 6 and (S["cnt"] == 1).sum() >= S["T"]
    with swz.Context(0) as ctx:
        for poison in (None, "1", "255"):  # the result does not depend on what the workspace held
            if poison is not None:
                ctx.release_workspace()
                ctx.set_option("SWZ_POISON", poison)
            lo, hi = ctx.node_boxes_device(d["perm"].data_ptr(), d["order"].data_ptr() if with_order else None, S["n"], d["xyz"].data_ptr(),
                                           dict(offset=S["off"], count=S["cnt"]))
            for k, why in enumerate(S["why"]):
                assert (lo[k] == want_lo[k]).all() and (hi[k] == want_hi[k]).all(), (why, poison, lo[k], want_lo[k], hi[k], want_hi[k])
            empty = S["cnt"] == 0
            assert np.isposinf(lo[empty]).all() and np.isneginf(hi[empty]).all()
            assert (lo[~empty][:, 1] == -7.25).all() and (hi[~empty][:, 1] == -7.25).all()


@pytest.mark.gpu
def test_nothing_to_reduce_launches_nothing(case):
    S = case
    d = S["d"]
    u = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    with swz.Context(0) as ctx:
        ctx.profile_enable(True)
        lo, hi = ctx.node_boxes_device(None, None, 0, None, dict(offset=u(), count=u()))
        assert lo.shape == (0, 3) and hi.shape == (0, 3)
        lo, hi = ctx.node_boxes_device(d["perm"].data_ptr(), None, S["n"], d["xyz"].data_ptr(), dict(offset=u(), count=u()))
        assert lo.shape == (0, 3)
        lo, hi = ctx.node_boxes_device(None, None, 0, None, dict(offset=u(0, 0), count=u(0, 0)))
        assert np.isposinf(lo).all() and np.isneginf(hi).all() and lo.shape == (2, 3)
        lo, hi = ctx.node_boxes_device(d["perm"].data_ptr(), None, S["n"], d["xyz"].data_ptr(), dict(offset=u(5, 9), count=u(0, 0)))
        assert np.isposinf(lo).all() and np.isneginf(hi).all()
        assert "node_boxes" not in ctx.profile_get()


@pytest.mark.gpu
def test_bad_tables_are_refused_before_anything_is_launched(case):
    S = case
    d = S["d"]
    n = S["n"]
    u = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    perm, xyz = d["perm"].data_ptr(), d["xyz"].data_ptr()
    good = dict(offset=u(0, 10), count=u(10, 5))
    cases = [
        ("offsets not ascending", perm, xyz, n, dict(offset=u(10, 0), count=u(5, 10))),
        ("offsets of empty nodes not ascending", perm, xyz, n, dict(offset=u(10, 0), count=u(0, 0))),
        ("ranges overlap", perm, xyz, n, dict(offset=u(0, 9), count=u(10, 5))),
        ("range passes n", perm, xyz, n, dict(offset=u(0, n - 2), count=u(10, 3))),
        ("offset passes n", perm, xyz, n, dict(offset=u(0, n + 1), count=u(10, 1))),
        ("count wraps around", perm, xyz, n, dict(offset=u(0, 16), count=u(10, 2 ** 64 - 8))),
        ("NULL perm", None, xyz, n, good),
        ("NULL positions", perm, None, n, good),
        ("n above the limit", perm, xyz, 2 ** 32 - 65535, good),
    ]
    with swz.Context(0) as ctx:
        ctx.profile_enable(True)
        for name, p, x, rows, nodes in cases:
            with pytest.raises(swz.SwzError) as e:
                ctx.node_boxes_device(p, None, rows, x, nodes)
            assert e.value.code == ERR_BAD_ARG and "swz_node_boxes_device" in str(e.value), name
        assert "node_boxes" not in ctx.profile_get()
        # the context takes a valid call afterwards
        lo, hi = ctx.node_boxes_device(perm, None, n, xyz, good)
        src = S["perm"]
        assert (lo[1] == S["xyz"][src[10:15]].min(axis=0)).all() and (hi[0] == S["xyz"][src[0:10]].max(axis=0)).all()
        assert ctx.profile_get()["node_boxes"]["launches"] == 2
