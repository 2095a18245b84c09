"""swz_filter_select_device alone: the stable compaction of the rows of a region that also pass a filter over the attribute
columns.

The reference is tests/filter_ref.py on top of tests/region_ref.py -- region_mask & filter_mask in numpy on the host copies --
and everything is compared for byte equality: xyz[mask], col[mask] and np.flatnonzero(mask).  Every output is pre-filled with
a poison byte and carries guard bands on both sides: nothing but the rows [0, count) may change."""
import numpy as np
import pytest

import filter_ref as F
import region_ref as R

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
POISON = 0xA5
GUARD = 64
INF = float("inf")
BOX = ([0.25, 0.25, 0.25], [0.75, 0.75, 0.75])
UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ALL = ("rgb", "normal") + F.SCALARS
# kind -> (region, where rows lie that the region accepts, where rows lie that are in BOX and that the kind's test refuses)
KINDS = {"box": (None, ([0.3, 0.3, 0.3], [0.7, 0.7, 0.7]), ([0.8, 0.3, 0.3], [0.9, 0.7, 0.7])),
         "planes": (("planes", [[1.0, 0.0, 0.0, -0.4]]), ([0.45, 0.3, 0.3], [0.7, 0.7, 0.7]), ([0.3, 0.3, 0.3], [0.35, 0.7, 0.7])),
         "polygon": (("polygon", R.L_SHAPE), ([0.3, 0.3, 0.3], [0.45, 0.45, 0.7]), ([0.55, 0.55, 0.3], [0.7, 0.7, 0.7]))}


@pytest.fixture(scope="module")
def G():
    import torch
    import schwarzwald_amd as swz
    with swz.Context(0) as ctx:
        yield dict(ctx=ctx, T=swz.box_select_tile(), dev=torch.device("cuda", 0))


def _columns(n, names, seed=5):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(seed)
    out = {}
    for name in names:
        _, dt, width = swz.ATTRIBUTES[name]
        raw = rng.integers(0, 256, n * width * np.dtype(dt).itemsize, dtype=np.uint8)
        out[name] = raw.view(dt).reshape((n, width) if width > 1 else (n,)).copy()
    if "gps_time" in out:                                    # random bytes hold NaN; the special values have a test of their own
        out["gps_time"] = rng.random(n) * 1e6
    return out


def _between(n, lo_hi, seed=7):
    lo, hi = np.asarray(lo_hi[0]), np.asarray(lo_hi[1])
    return lo + (hi - lo) * np.random.default_rng(seed).random((n, 3))


def _cloud(n, seed):
    return np.random.default_rng(seed).random((n, 3))


class Outputs:
    """poisoned device buffers with guard bands: positions, rows and the named columns"""

    def __init__(self, G, capacity, names):
        import torch
        import schwarzwald_amd as swz
        self.widths = {"xyz": 24, "row": 4}
        self.widths.update({k: swz.ATTRIBUTES[k][2] * np.dtype(swz.ATTRIBUTES[k][1]).itemsize for k in names})
        self.buf = {k: torch.full(((capacity + 2 * GUARD) * w,), POISON, dtype=torch.uint8, device=G["dev"]) for k, w in self.widths.items()}

    def ptr(self, k):
        return self.buf[k].data_ptr() + GUARD * self.widths[k]

    def host(self, k):
        return self.buf[k].cpu().numpy()

    def rows_of(self, k, count, dtype, width):
        w = self.widths[k]
        raw = self.host(k)[GUARD * w:(GUARD + count) * w].copy()
        return raw.view(dtype).reshape((count, width) if width > 1 else (count,))

    def assert_poison_beyond(self, count, only=None):
        for k, w in self.widths.items():
            if only is not None and k not in only:
                continue
            h = self.host(k)
            assert (h[:GUARD * w] == POISON).all(), k
            assert (h[(GUARD + count) * w:] == POISON).all(), k


def _upload(G, xyz, cols):
    import torch
    pad = np.zeros(8, np.uint8)  # (an empty tensor has no address)
    d_xyz = torch.from_numpy(np.concatenate([np.ascontiguousarray(xyz).view(np.uint8).reshape(-1), pad])).to(G["dev"])
    d_cols = {k: torch.from_numpy(np.concatenate([np.ascontiguousarray(v).view(np.uint8).reshape(-1), pad])).to(G["dev"]) for k, v in cols.items()}
    return d_xyz, d_cols


def _run(G, xyz, cols, box, region, filter, returned=None, capacity=None, call="filter"):
    """cols: every column on the device; returned: the columns asked back (default: all of cols)"""
    import torch
    import schwarzwald_amd as swz
    n = len(xyz)
    returned = tuple(cols) if returned is None else tuple(returned)
    d_xyz, d_cols = _upload(G, xyz, cols)
    cap = n if capacity is None else capacity
    out = Outputs(G, cap, returned)
    ins, outs = {k: v.data_ptr() for k, v in d_cols.items()}, {k: out.ptr(k) for k in returned}
    rg = region if isinstance(region, swz.Region) else R.as_region(swz, region)
    if call == "region":
        count = G["ctx"].region_select_device(d_xyz.data_ptr(), n, box[0], box[1], rg, cap, out.ptr("xyz"), {k: ins[k] for k in returned}, outs,
                                              d_row_out=out.ptr("row"))
    else:
        fl = filter if isinstance(filter, swz.Filter) else F.as_filter(swz, filter)
        count = G["ctx"].filter_select_device(d_xyz.data_ptr(), n, box[0], box[1], rg, fl, cap, out.ptr("xyz"), ins, outs, d_row_out=out.ptr("row"))
    torch.cuda.synchronize()
    return count, out


def _check(G, xyz, cols, box, region, filter, returned=None):
    import schwarzwald_amd as swz
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    mask = F.select_mask(xyz, cols, box, region, filter)
    count, out = _run(G, xyz, cols, box, region, filter, returned)
    assert count == int(mask.sum())
    assert out.rows_of("xyz", count, np.float64, 3).tobytes() == xyz[mask].tobytes()
    for k in (tuple(cols) if returned is None else returned):
        _, dt, width = swz.ATTRIBUTES[k]
        assert out.rows_of(k, count, dt, width).tobytes() == cols[k][mask].tobytes(), k
    assert np.array_equal(out.rows_of("row", count, np.uint32, 1), np.flatnonzero(mask).astype(np.uint32))
    out.assert_poison_beyond(count)
    return mask


def _sizes(T):
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


def _patterns(n, T):
    idx = np.arange(n)
    pats = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "wave_ends": (idx % 64 == 0) | (idx % 64 == 63),
            "tile_ends": (idx % T == 0) | (idx % T == T - 1), "every_other": idx % 2 == 0}
    if n:
        pats["one_in_the_last_tile"] = idx == n - 1
    return pats


@pytest.mark.parametrize("size", range(9))
@pytest.mark.parametrize("kind", list(KINDS))
def test_sizes_and_patterns(G, kind, size):
    """every row is in the region: it is the filter that draws the pattern"""
    n = _sizes(G["T"])[size]
    region, inside, _ = KINDS[kind]
    xyz = _between(n, inside)
    cols = _columns(n, ("rgb", "intensity", "classification"))
    for name, passing in _patterns(n, G["T"]).items():
        cols["classification"] = np.where(passing, 2, 3).astype(np.uint8)
        mask = _check(G, xyz, cols, BOX, region, [("any_of", "classification", [2])])
        assert np.array_equal(mask, passing), name


def _planted(name, n, values, seed):
    """a random column with `values` planted at its front and its end (the first and the last tile)"""
    col = _columns(n, (name,), seed)[name]
    v = np.asarray(values, dtype=col.dtype)
    col[:len(v)] = v
    col[n - len(v):] = v
    return col


def _attribute_cases():
    cases = []
    for name in ("intensity", "point_source_id"):
        edge = [0, 65535, 1, 65534, 300]
        for lo, hi in ((0, 0), (65535, 65535), (0.5, 65534.5), (-INF, 20000.25), (300, 300), (40000, INF), (-5.0, 70000.0)):
            cases.append((name, edge, ("range", name, lo, hi)))
    name = "scan_angle_rank"
    edge = [-128, -1, 0, 127, 5]
    for lo, hi in ((-128, -128), (-1, -1), (0, 0), (127, 127), (-0.5, 127), (-128, -0.5), (-1.5, 0.5), (-INF, INF)):
        cases.append((name, edge, ("range", name, lo, hi)))
    for values in ([-1], [0], [-128], [127, -128], list(range(256))):
        cases.append((name, edge, ("any_of", name, values)))
        cases.append((name, edge, ("none_of", name, values)))
    for name in F.ONE_BYTE:
        if name == "scan_angle_rank":
            continue
        edge = [0, 255, 1, 254, 128, 127, 64, 63]
        for lo, hi in ((0, 0), (255, 255), (1.5, 7.25), (128, 128), (127.5, INF)):
            cases.append((name, edge, ("range", name, lo, hi)))
        for values in ([0], [255], list(range(256)), [63, 64, 127, 128, 191, 192]):
            cases.append((name, edge, ("any_of", name, values)))
        cases.append((name, edge, ("none_of", name, [0, 255])))
    return cases


def test_every_attribute_as_range_and_as_set(G):
    n = G["T"] + 37
    xyz = _cloud(n, 11)
    seen = set()
    for i, (name, edge, clause) in enumerate(_attribute_cases()):
        cols = {name: _planted(name, n, edge, 100 + len(name))}
        mask = _check(G, xyz, cols, UNIT, None, [clause], returned=())
        # the planted values decide as the contract says, stated here without the reference
        v = cols[name][:len(edge)].astype(np.float64)
        if clause[0] == "range":
            assert mask[:len(edge)].tolist() == [bool(clause[2] <= x <= clause[3]) for x in v], clause
        else:
            has = [int(x) & 255 in {int(s) & 255 for s in clause[2]} for x in cols[name][:len(edge)]]
            assert mask[:len(edge)].tolist() == [h == (clause[0] == "any_of") for h in has], clause
        seen.add((name, clause[0] == "range"))
    assert {k for k, _ in seen} == set(F.SCALARS) - {"gps_time"}
    assert {k for k, r in seen if not r} == set(F.ONE_BYTE)


GPS_SPECIALS = [float("nan"), 0.0, -0.0, INF, -INF, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, -1.0, np.nextafter(1.0, 2.0)]


@pytest.mark.parametrize("kind", ["range", "not_range"])
def test_gps_time_specials(G, kind):
    n = G["T"] + 5
    xyz = _cloud(n, 13)
    gps = np.random.default_rng(3).normal(size=n)
    gps[:len(GPS_SPECIALS)] = GPS_SPECIALS
    gps[n - len(GPS_SPECIALS):] = GPS_SPECIALS
    cols = {"gps_time": gps, "classification": _columns(n, ("classification",))["classification"]}
    k = len(GPS_SPECIALS)
    for lo, hi in ((0.0, 0.0), (-0.0, 0.0), (-INF, INF), (5e-324, 1.0), (-5e-324, 5e-324), (INF, INF), (-INF, -INF), (-INF, -5e-324),
                   (1.0, 1.0), (np.nextafter(1.0, 2.0), 2.0), (-0.25, 0.75)):
        mask = _check(G, xyz, cols, UNIT, None, [(kind, "gps_time", lo, hi)], returned=("gps_time", "classification"))
        plain = [bool(lo <= x <= hi) for x in GPS_SPECIALS]            # (Python: a NaN fails both compares)
        assert mask[:k].tolist() == (plain if kind == "range" else [not p for p in plain]), (lo, hi)
        assert bool(mask[0]) == (kind == "not_range")                  # the NaN fails a RANGE and passes its inversion
    # +0.0 and -0.0 are one value to the compares
    assert F.clause_mask(np.array([0.0, -0.0]), ("range", "gps_time", 0.0, 0.0)).all()


def test_clause_counts(G):
    n = 2 * G["T"] + 9
    xyz = _cloud(n, 17)
    cols = _columns(n, ("rgb",) + F.SCALARS)
    one = [("range", "intensity", 1000, 60000.5)]
    two = one + [("none_of", "classification", list(range(0, 256, 3)))]
    eight = two + [("range", "gps_time", 1e5, INF), ("range", "scan_angle_rank", -100, 100), ("not_range", "point_source_id", 100, 4000),
                   ("any_of", "user_data", list(range(16, 250))), ("range", "number_of_returns", 3, 255), ("range", "intensity", 2000, 50000)]
    counts = []
    for filter in (one, two, eight):
        mask = _check(G, xyz, cols, UNIT, None, filter)
        counts.append(int(mask.sum()))
    assert n > counts[0] > counts[1] > counts[2] > 0
    # two clauses on one attribute whose intersection is empty
    for filter in ([("range", "classification", 2, 2), ("none_of", "classification", [2])],
                   [("range", "intensity", 0, 100), ("range", "intensity", 100.5, 65535)]):
        assert _check(G, xyz, cols, UNIT, None, filter).sum() == 0


@pytest.mark.parametrize("kind", list(KINDS))
def test_region_kinds_with_a_filter(G, kind):
    n = 2 * G["T"] + 3
    region, inside, outside = KINDS[kind]
    in_region = np.arange(n) % 3 != 0
    xyz = _between(n, outside, 19)
    xyz[in_region] = _between(int(in_region.sum()), inside, 23)
    cols = _columns(n, ("rgb", "return_number", "intensity"))
    cols["return_number"] = (np.arange(n) % 5).astype(np.uint8)
    filter = [("range", "return_number", 1, 1)]
    mask = _check(G, xyz, cols, BOX, region, filter)
    assert np.array_equal(mask, in_region & (cols["return_number"] == 1)) and 0 < mask.sum() < in_region.sum()
    # a region that rejects every row, with a filter that passes every row
    assert _check(G, _between(n, outside, 29), cols, BOX, region, [("range", "return_number", 0, 255)]).sum() == 0
    # a filter that rejects every row of a region that holds every row
    assert _check(G, _between(n, inside, 31), cols, BOX, region, [("any_of", "return_number", [77])]).sum() == 0
    # a row with a NaN position and a passing attribute is out
    few = _between(8, inside, 37)
    for a in range(3):
        few[1 + 2 * a, a] = np.nan
    mask = _check(G, few, {"return_number": np.ones(8, np.uint8)}, BOX, region, filter)
    assert mask.tolist() == [True, False, True, False, True, False, True, True]


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_filtered_column_outside_the_mask(G, kind):
    import torch
    n = G["T"] + 21
    region, inside, _ = KINDS[kind]
    xyz = _between(n, inside, 41)
    cols = _columns(n, ("classification", "intensity", "gps_time"))
    filter = [("range", "classification", 0, 99), ("range", "gps_time", 2e5, INF)]
    mask = _check(G, xyz, cols, BOX, region, filter, returned=("intensity",))
    assert 0 < mask.sum() < n
    # an output buffer passed for a filtered column that the mask does not name stays as it was
    d_xyz, d_cols = _upload(G, xyz, cols)
    out = Outputs(G, n, ("intensity", "classification", "gps_time"))
    count = G["ctx"].filter_select_device(d_xyz.data_ptr(), n, BOX[0], BOX[1], R.as_region(__import__("schwarzwald_amd"), region),
                                          F.as_filter(__import__("schwarzwald_amd"), filter), n, out.ptr("xyz"),
                                          {k: v.data_ptr() for k, v in d_cols.items()}, {k: out.ptr(k) for k in cols}, attrs=("intensity",),
                                          d_row_out=out.ptr("row"))
    torch.cuda.synchronize()
    assert count == int(mask.sum())
    assert out.rows_of("intensity", count, np.uint16, 1).tobytes() == cols["intensity"][mask].tobytes()
    out.assert_poison_beyond(0, only=("classification", "gps_time"))
    out.assert_poison_beyond(count)
    for k, v in cols.items():                                          # and the inputs are read, never written
        assert d_cols[k].cpu().numpy()[:v.nbytes].tobytes() == v.tobytes(), k


@pytest.mark.parametrize("kind", list(KINDS))
def test_no_filter_gives_the_bytes_of_the_region_call(G, kind):
    import schwarzwald_amd as swz
    xyz = _cloud(3 * G["T"] + 5, 43)
    cols = _columns(len(xyz), ALL)
    region = KINDS[kind][0]
    want_count, want = _run(G, xyz, cols, BOX, region, None, call="region")
    assert 0 < want_count < len(xyz)
    for filter in (None, swz.Filter()):
        count, got = _run(G, xyz, cols, BOX, region, filter)
        assert count == want_count
        for k in want.buf:
            assert got.host(k).tobytes() == want.host(k).tobytes(), k


@pytest.mark.parametrize("kind", list(KINDS))
def test_count_only_capacity_and_two_runs(G, kind):
    import torch
    import schwarzwald_amd as swz
    n = 2 * G["T"] + 9
    region = KINDS[kind][0]
    xyz, cols = _cloud(n, 47), _columns(n, ("classification", "intensity", "rgb", "gps_time", "normal"))
    filter = [("range", "intensity", 9000, INF), ("none_of", "classification", [7, 18])]
    want = int(F.select_mask(xyz, cols, BOX, region, filter).sum())
    assert 1 < want < n
    d_xyz, d_cols = _upload(G, xyz, cols)
    ins = {k: v.data_ptr() for k, v in d_cols.items()}
    rg, fl = R.as_region(swz, region), F.as_filter(swz, filter)
    assert G["ctx"].filter_select_device(d_xyz.data_ptr(), n, BOX[0], BOX[1], rg, fl, 0, None, ins) == want    # counts, writes nothing
    a, b = _run(G, xyz, cols, BOX, region, filter, capacity=want), _run(G, xyz, cols, BOX, region, filter, capacity=want)
    assert a[0] == b[0] == want
    a[1].assert_poison_beyond(want)
    for k in a[1].buf:
        assert a[1].host(k).tobytes() == b[1].host(k).tobytes(), k
    # one row short: refused with the needed count, every output still poison
    out = Outputs(G, want - 1, tuple(cols))
    with pytest.raises(swz.SwzError) as e:
        G["ctx"].filter_select_device(d_xyz.data_ptr(), n, BOX[0], BOX[1], rg, fl, want - 1, out.ptr("xyz"), ins, {k: out.ptr(k) for k in cols},
                                      d_row_out=out.ptr("row"))
    torch.cuda.synchronize()
    assert e.value.code == ERR_BAD_ARG and "capacity" in str(e.value) and e.value.needed == want
    out.assert_poison_beyond(0)


def test_refusals_launch_nothing(G):
    import torch
    import schwarzwald_amd as swz
    n = G["T"] + 1
    xyz = np.full((n, 3), 0.5)
    cols = {"classification": np.full(n, 2, np.uint8), "intensity": np.full(n, 9, np.uint16)}
    d_xyz, d_cols = _upload(G, xyz, cols)
    ins = {k: v.data_ptr() for k, v in d_cols.items()}
    out = Outputs(G, n, ("intensity",))
    ctx = G["ctx"]
    Fl = swz.Filter

    def refused(word, filter, d_in=ins, region=None, xyz_out=None):
        with pytest.raises(swz.SwzError) as e:
            ctx.filter_select_device(d_xyz.data_ptr(), n, UNIT[0], UNIT[1], region, filter, n, out.ptr("xyz") if xyz_out is None else xyz_out,
                                     d_in, {"intensity": out.ptr("intensity")}, d_row_out=out.ptr("row"))
        assert e.value.code == ERR_BAD_ARG and "swz_filter_select_device" in str(e.value) and word in str(e.value), str(e.value)

    ok = lambda: Fl().range("intensity", 0, 10)
    # a filtered column missing from d_in, named
    refused("the filter names SWZ_ATTR_CLASSIFICATION,", ok().any_of("classification", [2]), d_in={"intensity": ins["intensity"]})
    refused("the filter names SWZ_ATTR_GPS_TIME,", ok().range("gps_time", 0, 1))
    # everything swz_filter_check refuses, with the clause's number
    nine = Fl()
    nine.count = 9
    refused("8 clauses", nine)
    refused("reserved", Fl(reserved=1))
    refused("clause 1: an attribute outside the table", ok().clause(12, swz.FILTER_RANGE, 0, 1))
    refused("clause 1: SWZ_ATTR_RGB", ok().range("rgb", 0, 1))
    refused("clause 1: SWZ_ATTR_NORMAL", ok().range("normal", 0, 1))
    refused("clause 1: an unknown kind", ok().clause("intensity", 2, 0, 1))
    refused("clause 1: an unknown flag bit", ok().clause("intensity", 0x200, 0, 1))
    refused("clause 1: a SET on SWZ_ATTR_INTENSITY", ok().any_of("intensity", [1]))
    refused("clause 1: a RANGE with lo > hi", ok().range("intensity", 2, 1))
    refused("clause 1: a RANGE with a NaN bound", ok().range("intensity", float("nan"), 1))
    refused("clause 1: a SET with a lo or hi", ok().clause("classification", swz.FILTER_SET, lo=1.0))
    refused("clause 1: a RANGE with a set", ok().clause("classification", swz.FILTER_RANGE, 0, 1, bits=(1, 0, 0, 0)))
    # and what the region call refuses, with a filter that is in order
    refused("a = b = c = 0", ok(), region=swz.Region.planes([[0.0, 0.0, 0.0, 1.0]]))
    refused("aliases", ok(), xyz_out=d_xyz.data_ptr())
    refused("aliases", ok().any_of("classification", [2]), xyz_out=d_cols["classification"].data_ptr())   # a column only the filter reads
    torch.cuda.synchronize()
    out.assert_poison_beyond(0)
    assert np.array_equal(d_xyz.cpu().numpy()[:xyz.nbytes].view(np.float64).reshape(-1, 3), xyz)
    # n == 0: nothing is launched, the count is 0
    assert ctx.filter_select_device(0, 0, UNIT[0], UNIT[1], None, ok(), n, out.ptr("xyz"), ins, {"intensity": out.ptr("intensity")}) == 0
    out.assert_poison_beyond(0)
