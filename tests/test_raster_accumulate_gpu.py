"""swz_raster_clear_device and swz_raster_accumulate_device against tests/raster_ref.py: the whole cell table, integer fields
exactly, min and max by value.  The shapes are placed by swz_raster_tile(): rows around the tile, runs of lanes of one cell
that cross the 64-lane and the tile boundary, cells that alternate lane by lane, rows on cell edges and on the faces of the box,
rows just outside it, and values whose floating-point sum would depend on the order."""
import numpy as np
import pytest

import raster_ref as RR

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
BOX = ([0.0, 0.0, 0.0], [1.0, 2.0, 3.0])


@pytest.fixture(scope="module")
def G():
    import schwarzwald_amd as swz
    with swz.Context(0) as ctx:
        yield dict(swz=swz, ctx=ctx, T=swz.raster_tile())


def _up(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))


def _table(G, frame, batches, box, clear=True):
    """the table after the batches (xyz, column or None), one accumulate call each"""
    import torch
    swz, ctx = G["swz"], G["ctx"]
    n = frame["nx"] * frame["ny"]
    d_cells = torch.full((n, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=torch.device("cuda", ctx.device))   # not what a clear leaves
    if clear:
        ctx.raster_clear_device(frame, d_cells.data_ptr())
    for xyz, column in batches:
        d_xyz = _up(ctx, np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
        d_col = None if column is None else _up(ctx, column)
        ctx.raster_accumulate_device(d_xyz.data_ptr() if len(xyz) else None, len(xyz), box[0], box[1], frame, d_cells.data_ptr(),
                                     None if d_col is None or not len(xyz) else d_col.data_ptr())
    cells = d_cells.cpu().numpy().view(swz.RASTER_CELL_DTYPE).reshape(-1)
    got = swz.raster_finish(frame, cells)
    got.update(sum=cells["sum"].reshape(got["count"].shape), cells=cells)
    return got


def _check(G, box, nx, ny, xyz, value="z", column=None):
    frame = G["swz"].raster_frame_of(box[0], box[1], nx, ny, value)
    got = _table(G, frame, [(xyz, column)], box)
    ref_frame, want = RR.raster(box, nx, ny, xyz, value, column)
    assert RR.same_table(got, ref_frame, want)
    fin = RR.finish(ref_frame, want)
    assert np.array_equal(got["mean"], fin["mean"], equal_nan=True)
    return got


def _cloud(n, seed, box=BOX):
    """rows in and a little around the box"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(box[0]), np.array(box[1])
    return lo + (rng.random((n, 3)) * 1.2 - 0.1) * (hi - lo)


def test_rows_around_the_tile(G):
    T = G["T"]
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 17):
        got = _check(G, BOX, 7, 3, _cloud(n, 100 + n))        # not square: a swap of ix and iy would show
        assert got["count"].shape == (3, 7) and got["count"].sum() <= n and (n < T - 1 or got["count"].sum() > n // 4)   # (some rows lie outside)
    assert _check(G, BOX, 7, 3, [[0.5, 1.0, 1.5]])["count"][1, 3] == 1
    assert _check(G, BOX, 7, 3, np.zeros((0, 3)))["count"].sum() == 0


def test_one_cell_takes_every_row_in_any_order(G):
    """z of magnitudes 1e-3 and 1e3: a floating sum would depend on the order of the atomics; the integer sum does not"""
    n = 4 * G["T"] + 5
    rng = np.random.default_rng(7)
    box = ([0.0, 0.0, -2000.0], [1.0, 2.0, 2000.0])
    xyz = np.empty((n, 3))
    xyz[:, 0] = 3.5 / 7 + rng.random(n) * 0.01          # cell (ix 3, iy 1) of 7 x 3
    xyz[:, 1] = 1.0 + rng.random(n) * 0.01
    xyz[:, 2] = np.where(rng.random(n) < 0.5, 1e-3, 1e3) * (rng.random(n) * 2 - 1)
    got = _check(G, box, 7, 3, xyz)
    assert got["count"][1, 3] == n and got["count"].sum() == n
    again = _check(G, box, 7, 3, xyz[rng.permutation(n)])
    assert again["cells"].tobytes() == got["cells"].tobytes()


def test_neighbouring_rows_never_share_a_cell(G):
    n = 2 * G["T"] + 9
    rng = np.random.default_rng(8)
    xyz = _cloud(n, 9)
    xyz[:, 0] = np.where(np.arange(n) % 2 == 0, 0.05, 0.95) + rng.random(n) * 0.01
    xyz[:, 1] = np.where(np.arange(n) % 2 == 0, 0.1, 1.9)
    got = _check(G, BOX, 7, 3, xyz)
    assert got["count"][0, 0] > 0 and got["count"][2, 6] > 0 and got["count"][0, 0] + got["count"][2, 6] == got["count"].sum()


def test_runs_of_every_length_laid_end_to_end(G):
    """runs of 1 .. 70 lanes of one cell: they start at every lane, cross the 64-lane boundary and the tile boundary"""
    rng = np.random.default_rng(10)
    cell = np.concatenate([np.full(k, k % 21) for k in range(1, 71)])
    assert len(cell) > 9 * G["T"]
    n = len(cell)
    xyz = np.empty((n, 3))
    xyz[:, 0] = ((cell % 7) + 0.25 + 0.5 * rng.random(n)) / 7
    xyz[:, 1] = ((cell // 7) + 0.25 + 0.5 * rng.random(n)) * 2 / 3
    xyz[:, 2] = rng.random(n) * 3
    got = _check(G, BOX, 7, 3, xyz)
    assert got["count"].reshape(-1).tolist() == np.bincount(cell, minlength=21).tolist()
    # ... and with rows outside the box inside the runs: an outside lane breaks a run
    xyz[rng.random(n) < 0.2, 2] = 3.5
    _check(G, BOX, 7, 3, xyz)


def test_rows_on_the_cell_edges(G):
    box = ([0.25, -1.0, 0.0], [0.95, 1.0, 1.0])
    nx = 7
    frame = G["swz"].raster_frame_of(box[0], box[1], nx, 2)
    x = np.minimum(box[0][0] + np.arange(nx + 1) * frame["cw"], box[1][0])
    x[nx] = box[1][0]                                      # on box_max: the closed box keeps it, the clamp puts it into the last cell
    xyz = np.stack([np.repeat(x, 2), np.tile([-1.0, 1.0], nx + 1), np.full(2 * (nx + 1), 0.5)], axis=1)
    got = _check(G, box, nx, 2, xyz)
    assert got["count"].sum() == 2 * (nx + 1) and got["count"][0, nx - 1] >= 1 and got["count"][1, nx - 1] >= 1


def test_rows_just_outside_the_box_are_skipped(G):
    lo, hi = np.array(BOX[0]), np.array(BOX[1])
    mid = (lo + hi) / 2
    out = []
    for a in range(3):
        for bound, away in ((lo[a], -np.inf), (hi[a], np.inf)):
            p = mid.copy()
            p[a] = np.nextafter(bound, away)
            out.append(p)
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            p = mid.copy()
            p[a] = bad
            out.append(p)
    out = np.array(out)
    got = _check(G, BOX, 7, 3, out)
    assert got["count"].sum() == 0 and np.all(got["min"] == np.inf) and np.all(got["max"] == -np.inf) and np.all(np.isnan(got["mean"]))
    on = np.array([[lo[0], mid[1], mid[2]], [hi[0], mid[1], mid[2]], [mid[0], lo[1], mid[2]], [mid[0], hi[1], mid[2]], [mid[0], mid[1], lo[2]],
                   [mid[0], mid[1], hi[2]], hi, lo])
    rows = np.concatenate([out, on, out[::-1]])
    got = _check(G, BOX, 7, 3, rows)
    assert got["count"].sum() == len(on)


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 4096), (4096, 1)])
def test_grid_shapes(G, nx, ny):
    got = _check(G, BOX, nx, ny, _cloud(2 * G["T"] + 3, 11))
    assert got["count"].shape == (ny, nx) and got["count"].sum() > G["T"]


def test_flat_boxes(G):
    xyz = _cloud(G["T"] + 7, 12)
    xyz[::2, 2] = 1.5
    box = ([0.0, 0.0, 1.5], [1.0, 2.0, 1.5])              # flat in z: scale 1, every q is 0
    got = _check(G, box, 7, 3, xyz)
    assert got["count"].sum() > 0 and not got["sum"].any() and set(got["mean"][got["count"] > 0].tolist()) == {1.5}
    xyz[::2, 0] = 0.5
    box = ([0.5, 0.0, 0.0], [0.5, 2.0, 3.0])              # flat in x: one cell along it, no division
    got = _check(G, box, 1, 3, xyz)
    assert got["count"].sum() > 0


def test_signed_zeros(G):
    box = ([0.0, 0.0, -1.0], [1.0, 2.0, 1.0])
    xyz = np.array([[0.5, 1.0, 0.0], [0.5, 1.0, -0.0], [0.1, 0.1, -0.0], [0.9, 1.9, 0.0]] * 70)
    got = _check(G, box, 7, 3, xyz)
    held = got["count"] > 0          # the range is 2: scale 2^29, and q = (0 - -1) * 2^29 for either zero
    assert got["count"].sum() == len(xyz) and np.all(got["sum"][held] == got["count"][held].astype(np.int64) << 29)
    assert np.all(got["mean"][got["count"] > 0] == 0.0)


def test_value_intensity(G):
    n = 2 * G["T"] + 31
    rng = np.random.default_rng(13)
    xyz = _cloud(n, 14)
    col = rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)
    col[:4] = [0, 65535, 65535, 0]
    xyz[:4] = [[0.5, 1.0, 1.0]] * 4
    got = _check(G, BOX, 7, 3, xyz, "intensity", col)
    assert got["min"][1, 3] == 0.0 and got["max"][1, 3] == 65535.0
    every = np.full(n, 65535, dtype=np.uint16)
    got = _check(G, BOX, 1, 1, xyz, "point_source_id", every)
    assert got["sum"][0, 0] == 65535 * int(got["count"][0, 0]) and got["mean"][0, 0] == 65535.0


def test_value_scan_angle_rank_is_signed(G):
    n = G["T"] + 5
    rng = np.random.default_rng(15)
    xyz = _cloud(n, 16)
    col = rng.integers(-128, 127, n, endpoint=True).astype(np.int8)
    col[:2] = [-128, -1]
    xyz[:2] = [[0.5, 1.0, 1.0]] * 2
    got = _check(G, BOX, 7, 3, xyz, "scan_angle_rank", col)
    assert got["min"][1, 3] == -128.0 and got["sum"].sum() == int(col[RR.R.box_mask(xyz, BOX)].astype(np.int64).sum())
    unsigned = rng.integers(0, 255, n, endpoint=True).astype(np.uint8)
    unsigned[:2] = [255, 128]
    got = _check(G, BOX, 7, 3, xyz, "classification", unsigned)
    assert got["max"][1, 3] == 255.0


def test_two_calls_are_one_call_on_the_concatenation(G):
    swz = G["swz"]
    a, b = _cloud(G["T"] + 3, 17), _cloud(2 * G["T"] - 1, 18)
    frame = swz.raster_frame_of(BOX[0], BOX[1], 7, 3)
    two = _table(G, frame, [(a, None), (b, None)], BOX)
    one = _table(G, frame, [(np.concatenate([a, b]), None)], BOX)
    assert two["cells"].tobytes() == one["cells"].tobytes()
    ref_frame, want = RR.raster(BOX, 7, 3, np.concatenate([a, b]))
    assert RR.same_table(two, ref_frame, want)


def test_what_accumulate_refuses(G):
    import torch
    swz, ctx = G["swz"], G["ctx"]
    frame = swz.raster_frame_of(BOX[0], BOX[1], 7, 3)
    by_value = swz.raster_frame_of(BOX[0], BOX[1], 7, 3, "intensity")
    d_xyz = _up(ctx, _cloud(8, 19))
    d_col = _up(ctx, np.zeros(16, dtype=np.uint16))
    d_cells = torch.zeros((21, 4), dtype=torch.int64, device=d_xyz.device)
    ctx.raster_clear_device(frame, d_cells.data_ptr())
    before = d_cells.cpu().numpy().tobytes()
    other_box = ([0.0, 0.0, 0.0], [1.5, 2.0, 3.0])         # another cell width
    cases = ((dict(n=(1 << 32) - 65535), "more than 2^32-65536 rows"),
             (dict(d_xyz=None), "NULL d_xyz"),
             (dict(frame=by_value), "the value is SWZ_ATTR_INTENSITY, which has no input column"),
             (dict(frame=by_value, d_value=d_col.data_ptr() + 1), "the column of SWZ_ATTR_INTENSITY is not aligned to its element"),
             (dict(box=other_box), "the frame is not the one swz_raster_frame_of derives from this box"),
             (dict(frame=dict(frame, scale=2.0)), "the frame is not the one swz_raster_frame_of derives from this box"),
             (dict(frame=dict(frame, nx=0)), "nx or ny is 0"),
             (dict(d_xyz=d_xyz.data_ptr() + 4), "positions or cells that are not aligned to their element"))
    for change, words in cases:
        args = dict(d_xyz=d_xyz.data_ptr(), n=8, box=BOX, frame=frame, d_value=None)
        args.update(change)
        with pytest.raises(swz.SwzError) as e:
            ctx.raster_accumulate_device(args["d_xyz"], args["n"], args["box"][0], args["box"][1], args["frame"], d_cells.data_ptr(), args["d_value"])
        assert e.value.code == ERR_BAD_ARG and "swz_raster_accumulate_device: " + words in str(e.value), str(e.value)
    assert d_cells.cpu().numpy().tobytes() == before        # nothing was launched
