"""swz_box_select_device alone: the stable compaction of the rows of a closed box.

The reference is numpy on the host copies: xyz[mask], col[mask] and np.flatnonzero(mask), compared exactly.  Every output is
pre-filled with a poison byte and carries guard bands on both sides: nothing but the rows [0, count) may change."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
POISON = 0xA5
GUARD = 64  # rows of guard band in front of and behind every output
BOX = ([0.25, 0.25, 0.25], [0.75, 0.75, 0.75])
INSIDE, OUTSIDE = (0.5, 0.5, 0.5), (0.9, 0.5, 0.5)
ALL = ("rgb", "normal", "intensity", "classification", "edge_of_flight_line", "gps_time", "number_of_returns", "return_number",
       "point_source_id", "scan_direction_flag", "scan_angle_rank", "user_data")
ONE_OF_EACH_WIDTH = ("classification", "intensity", "rgb", "gps_time", "normal")  # u8, u16, 3 x u8, f64, 3 x f32


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
        raw = rng.integers(0, 256, n * width * np.dtype(dt).itemsize, dtype=np.uint8)  # any bit pattern, NaN payloads included
        out[name] = raw.view(dt).reshape((n, width) if width > 1 else (n,))
    return out


def _positions(n, inside, seed=7):
    """rows of `inside` get points strictly inside BOX, the others strictly outside; all rows differ"""
    rng = np.random.default_rng(seed)
    xyz = np.empty((n, 3))
    xyz[:] = 0.8 + 0.15 * rng.random((n, 3))
    xyz[inside] = 0.3 + 0.4 * rng.random((int(np.count_nonzero(inside)), 3))
    return xyz


def _truth(xyz, box):
    lo, hi = np.asarray(box[0]), np.asarray(box[1])
    with np.errstate(invalid="ignore"):
        return ((xyz >= lo) & (xyz <= hi)).all(axis=1)


class Outputs:
    """poisoned device buffers with guard bands: positions, columns, rows"""

    def __init__(self, G, capacity, names, rows=True):
        import torch
        import schwarzwald_amd as swz
        self.cap, self.names = capacity, names
        self.widths = {"xyz": 24, "row": 4}
        self.widths.update({k: swz.ATTRIBUTES[k][2] * np.dtype(swz.ATTRIBUTES[k][1]).itemsize for k in names})
        self.buf = {k: torch.full(((capacity + 2 * GUARD) * w,), POISON, dtype=torch.uint8, device=G["dev"])
                    for k, w in self.widths.items() if rows or k != "row"}

    def ptr(self, k):
        return self.buf[k].data_ptr() + GUARD * self.widths[k]

    def host(self, k):
        return self.buf[k].cpu().numpy()

    def rows_of(self, k, count, dtype, width):
        w = self.widths[k]
        raw = self.host(k)[GUARD * w:(GUARD + count) * w].copy()
        return raw.view(dtype).reshape((count, width) if width > 1 else (count,))

    def assert_poison_beyond(self, count):
        for k, w in self.widths.items():
            if k not in self.buf:
                continue
            h = self.host(k)
            assert (h[:GUARD * w] == POISON).all(), k
            assert (h[(GUARD + count) * w:] == POISON).all(), k


def _run(G, xyz, cols, box=BOX, capacity=None, rows=True, attrs=None):
    import torch
    n = len(xyz)
    pad = np.zeros(8, np.uint8)  # (an empty tensor has no address)
    d_xyz = torch.from_numpy(np.concatenate([np.ascontiguousarray(xyz).view(np.uint8).reshape(-1), pad])).to(G["dev"])
    d_cols = {k: torch.from_numpy(np.concatenate([np.ascontiguousarray(v).view(np.uint8).reshape(-1), pad])).to(G["dev"])
              for k, v in cols.items()}
    cap = n if capacity is None else capacity
    out = Outputs(G, cap, tuple(cols), rows)
    count = G["ctx"].box_select_device(d_xyz.data_ptr(), n, box[0], box[1], cap, out.ptr("xyz"),
                                       {k: v.data_ptr() for k, v in d_cols.items()}, {k: out.ptr(k) for k in cols}, attrs=attrs,
                                       d_row_out=out.ptr("row") if rows else None)
    torch.cuda.synchronize()
    return count, out


def _check(G, xyz, cols, box=BOX, rows=True):
    import schwarzwald_amd as swz
    mask = _truth(xyz, box)
    count, out = _run(G, xyz, cols, box, rows=rows)
    assert count == int(mask.sum())
    assert out.rows_of("xyz", count, np.float64, 3).tobytes() == xyz[mask].tobytes()
    for k, v in cols.items():
        _, dt, width = swz.ATTRIBUTES[k]
        assert out.rows_of(k, count, dt, width).tobytes() == v[mask].tobytes(), k
    if rows:
        assert np.array_equal(out.rows_of("row", count, np.uint32, 1), np.flatnonzero(mask).astype(np.uint32))
    out.assert_poison_beyond(count)
    return count, out


def _sizes(T):
    return [0, 1, T - 1, T, T + 1, 3 * T + 5]


def _patterns(n, T):
    idx = np.arange(n)
    pats = {"all_in": np.ones(n, bool), "all_out": np.zeros(n, bool), "every_other": idx % 2 == 0, "every_64th": idx % 64 == 0}
    if n:
        pats["only_first"] = idx == 0
        pats["only_last"] = idx == n - 1
    if n > T:
        pats["tile_edge"] = (idx == T - 1) | (idx == T)
    if n >= 3 * T:
        pats["tile_out_between"] = (idx < T) | ((idx >= 2 * T) & (idx < 3 * T))
    return pats


@pytest.mark.parametrize("columns", [(), ONE_OF_EACH_WIDTH, ALL], ids=["none", "widths", "all"])
@pytest.mark.parametrize("size", range(6))
def test_patterns(G, size, columns):
    n = _sizes(G["T"])[size]
    cols = _columns(n, columns)
    for name, inside in _patterns(n, G["T"]).items():
        count, _ = _check(G, _positions(n, inside), cols)
        assert count == int(inside.sum()), name


def test_patterns_cover_the_tile_cases(G):
    T = G["T"]
    assert {"tile_edge", "tile_out_between", "only_last"} <= set(_patterns(3 * T + 5, T))


def test_without_row_output(G):
    n = 2 * G["T"] + 3
    _check(G, _positions(n, np.arange(n) % 3 == 0), _columns(n, ONE_OF_EACH_WIDTH), rows=False)


def test_faces_nan_and_degenerate_box(G):
    lo, hi = np.array([0.25, -3.0, 1e6]), np.array([0.75, -1.0, 1e6 + 1])
    mid = (lo + hi) / 2
    rows, want = [], []
    for a in range(3):
        for bound, away in ((lo, -np.inf), (hi, np.inf)):
            p = mid.copy()
            p[a] = bound[a]
            rows.append(p.copy())
            want.append(True)                          # on the face
            p[a] = np.nextafter(bound[a], away)
            rows.append(p.copy())
            want.append(False)                         # one ulp outside
        p = mid.copy()
        p[a] = np.nan
        rows.append(p)
        want.append(False)
    rows += [lo.copy(), hi.copy(), mid.copy()]
    want += [True, True, True]
    xyz = np.array(rows)
    assert _truth(xyz, (lo, hi)).tolist() == want
    count, _ = _check(G, xyz, _columns(len(xyz), ("classification",)), box=(lo.tolist(), hi.tolist()))
    assert count == sum(want)
    # min == max: the points equal to it, and -0.0 == 0.0
    pt = np.array([0.5, 0.0, -2.0])
    xyz = np.array([pt, [0.5, -0.0, -2.0], np.nextafter(pt, np.inf), np.nextafter(pt, -np.inf), [np.nan, 0.0, -2.0], pt])
    count, _ = _check(G, xyz, {}, box=(pt.tolist(), pt.tolist()))
    assert count == 3


def test_two_runs_give_the_same_bytes(G):
    n = 3 * G["T"] + 5
    rng = np.random.default_rng(11)
    xyz, cols = rng.random((n, 3)), _columns(n, ALL)
    a, b = _run(G, xyz, cols), _run(G, xyz, cols)
    assert a[0] == b[0] > 0
    for k in a[1].buf:
        assert a[1].host(k).tobytes() == b[1].host(k).tobytes(), k


def test_count_only_and_capacity(G):
    import torch
    import schwarzwald_amd as swz
    n = 2 * G["T"] + 9
    rng = np.random.default_rng(13)
    xyz, cols = rng.random((n, 3)), _columns(n, ONE_OF_EACH_WIDTH)
    want = int(_truth(xyz, BOX).sum())
    assert 1 < want < n
    d_xyz = torch.from_numpy(xyz).to(G["dev"])
    assert G["ctx"].box_select_device(d_xyz.data_ptr(), n, BOX[0], BOX[1], 0, None) == want   # counts, writes nothing
    count, out = _run(G, xyz, cols, capacity=want)                                              # exactly enough
    assert count == want
    out.assert_poison_beyond(want)
    with pytest.raises(swz.SwzError) as e:
        _run(G, xyz, cols, capacity=want - 1)
    assert e.value.code == ERR_BAD_ARG and "capacity" in str(e.value) and e.value.needed == want
    # the refused call's outputs: all poison
    out = Outputs(G, want - 1, tuple(cols))
    d_cols = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to(G["dev"]) for k, v in cols.items()}
    with pytest.raises(swz.SwzError):
        G["ctx"].box_select_device(d_xyz.data_ptr(), n, BOX[0], BOX[1], want - 1, out.ptr("xyz"), {k: v.data_ptr() for k, v in d_cols.items()},
                                   {k: out.ptr(k) for k in cols}, d_row_out=out.ptr("row"))
    torch.cuda.synchronize()
    out.assert_poison_beyond(0)


def test_refusals_launch_nothing(G):
    import torch
    import schwarzwald_amd as swz
    n = G["T"] + 1
    xyz = np.full((n, 3), 0.5)
    d_xyz = torch.from_numpy(xyz).to(G["dev"])
    d_cls = torch.zeros(n, dtype=torch.uint8, device=G["dev"])
    out = Outputs(G, n, ("classification",))
    ctx = G["ctx"]

    def refused(word, n=n, box=BOX, d_in=None, d_out=None, attrs=None, xyz_out=None, capacity=n):
        with pytest.raises(swz.SwzError) as e:
            ctx.box_select_device(d_xyz.data_ptr(), n, box[0], box[1], capacity, out.ptr("xyz") if xyz_out is None else xyz_out, d_in, d_out,
                                  attrs=attrs, d_row_out=out.ptr("row"))
        assert e.value.code == ERR_BAD_ARG and word in str(e.value), str(e.value)

    refused("2^32-65536", n=(1 << 32) - 65535)
    refused("input column", attrs=("classification",), d_out={"classification": out.ptr("classification")})
    refused("output column", attrs=("classification",), d_in={"classification": d_cls.data_ptr()})
    refused("does not exist", attrs=1 << 12)
    refused("box_min > box_max", box=([0.5, 0.5, 0.5], [0.5, 0.4, 0.5]))
    refused("not finite", box=([0.0, 0.0, 0.0], [1.0, float("inf"), 1.0]))
    refused("not finite", box=([float("nan"), 0.0, 0.0], [1.0, 1.0, 1.0]))
    refused("aliases", xyz_out=d_xyz.data_ptr())
    refused("aliases", xyz_out=d_xyz.data_ptr() + 24 * (n - 1))
    refused("aliases", attrs=("classification",), d_in={"classification": d_cls.data_ptr()}, d_out={"classification": d_cls.data_ptr()})
    torch.cuda.synchronize()
    out.assert_poison_beyond(0)
    assert np.array_equal(d_xyz.cpu().numpy(), xyz)
    # n == 0: nothing is launched, the count is 0
    assert ctx.box_select_device(0, 0, BOX[0], BOX[1], n, out.ptr("xyz")) == 0
    out.assert_poison_beyond(0)
