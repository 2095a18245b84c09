"""The host side of the raster (include/swz_gpu.h), no GPU: tests/raster_ref.py against a plain Python loop, every refusal of
swz_raster_frame_of by its text, the frame's scale over twelve and more decades of z range, swz_raster_finish on a handmade
table, and the sizes of the structs as the bindings lay them out."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import raster_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = 2


@pytest.fixture(scope="module")
def swz():
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    import schwarzwald_amd
    schwarzwald_amd.load_library()
    return schwarzwald_amd


def test_reference_against_a_plain_loop():
    """300 random rows, some outside the box, some on its faces: the table of raster_ref is the one a double loop builds"""
    rng = np.random.default_rng(31)
    box = ([-1.0, 2.0, 10.0], [3.0, 5.0, 14.5])
    nx, ny = 5, 4
    xyz = rng.random((300, 3)) * [4.4, 3.4, 5.0] + [-1.2, 1.8, 9.8]
    xyz[:6] = [[3.0, 5.0, 14.5], [-1.0, 2.0, 10.0], [3.0, 2.0, 12.0], [1.0, 5.0, 12.0], [np.nan, 3.0, 12.0], [0.0, 3.0, np.inf]]
    frame, table = RR.raster(box, nx, ny, xyz)
    cw, ch = (3.0 - -1.0) / 5, (5.0 - 2.0) / 4
    assert frame["cw"] == cw and frame["ch"] == ch and frame["v0"] == 10.0 and frame["scale"] == 2.0 ** 28   # 4.5 = 1.125 x 2^2
    count, total = [0] * (nx * ny), [0] * (nx * ny)
    lo, hi = [math.inf] * (nx * ny), [-math.inf] * (nx * ny)
    inside = 0
    for x, y, z in xyz.tolist():
        if not (-1.0 <= x <= 3.0 and 2.0 <= y <= 5.0 and 10.0 <= z <= 14.5):
            continue
        inside += 1
        ix = min(int(math.floor((x - -1.0) / cw)), nx - 1)
        iy = min(int(math.floor((y - 2.0) / ch)), ny - 1)
        cell = iy * nx + ix
        count[cell] += 1
        total[cell] += round((z - 10.0) * 2.0 ** 28)        # Python's round: ties to even
        lo[cell], hi[cell] = min(lo[cell], z), max(hi[cell], z)
    assert 100 < inside < 300 and count[nx * ny - 1] >= 1 and count[0] >= 1
    assert table["count"].tolist() == count and table["sum"].tolist() == total
    assert table["min"].tolist() == lo and table["max"].tolist() == hi
    fin = RR.finish(frame, table)
    for cell in range(nx * ny):
        got = fin["mean"].reshape(-1)[cell]
        if count[cell] == 0:
            assert math.isnan(got)
        else:
            assert got == 10.0 + (float(total[cell]) / float(count[cell])) / 2.0 ** 28
            exact = math.fsum(z for x, y, z in xyz.tolist() if -1.0 <= x <= 3.0 and 2.0 <= y <= 5.0 and 10.0 <= z <= 14.5
                              and min(int(math.floor((y - 2.0) / ch)), ny - 1) * nx + min(int(math.floor((x + 1.0) / cw)), nx - 1) == cell) / count[cell]
            assert abs(got - exact) <= 4.5 * 2.0 ** -31 + 4 * np.finfo(np.float64).eps * 14.5   # half a step, and the roundings


def test_frame_is_the_references(swz):
    for box, nx, ny, value in ((([0.0, 0.0, 0.0], [1.0, 1.0, 1.0]), 7, 3, "z"), (([-3.5, 2.25, 100.0], [9.0, 2.25, 100.0]), 11, 1, "z"),
                               (([1e6, 5e6, -20.0], [1e6 + 333.3, 5e6 + 777.7, 3000.0]), 1000, 999, "z"),
                               (([0.0, 0.0, 0.0], [0.3, 0.7, 0.1]), 3, 7, "intensity")):
        got = swz.raster_frame_of(box[0], box[1], nx, ny, value)
        want = RR.frame_of(box[0], box[1], nx, ny, value)
        for k in ("x0", "y0", "cw", "ch", "v0", "scale"):
            assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])
        assert (got["nx"], got["ny"], got["reserved"]) == (nx, ny, 0)
        assert got["value"] == (swz.RASTER_VALUE_Z if value == "z" else swz.ATTRIBUTES[value][0])


@pytest.mark.parametrize("rng", [0.0, 1.0, 1000.0, 1e-12, 1e12])
def test_scale_keeps_the_range_below_2_31(swz, rng):
    f = swz.raster_frame_of([0.0, 0.0, 5.0], [1.0, 1.0, 5.0 + rng], 2, 2)
    real = (5.0 + rng) - 5.0     # the range the library sees
    assert f["v0"] == 5.0 and math.frexp(f["scale"])[0] == 0.5      # a power of two
    if rng == 0.0:
        assert f["scale"] == 1.0
    else:
        assert 2.0 ** 30 <= real * f["scale"] < 2.0 ** 31
        assert f["scale"] == 2.0 ** (30 - (math.frexp(real)[1] - 1))


REFUSALS = (
    (dict(nx=0), "nx or ny is 0"),
    (dict(ny=0), "nx or ny is 0"),
    (dict(nx=1 << 13, ny=(1 << 13) + 1), "nx * ny is more than SWZ_RASTER_MAX_CELLS (2^26): 8192 x 8193"),
    (dict(box_max=[1.0, math.inf, 1.0]), "a bound of the box is not finite"),
    (dict(box_min=[math.nan, 0.0, 0.0]), "a bound of the box is not finite"),
    (dict(box_min=[0.0, 0.0, 2.0]), "box_min > box_max"),
    (dict(box_min=[1.0, 0.0, 0.0], nx=2), "the box is flat along x (box_min == box_max) and nx is not 1"),
    (dict(box_min=[0.0, 1.0, 0.0], ny=3), "the box is flat along y (box_min == box_max) and ny is not 1"),
    (dict(value="gps_time"), "SWZ_ATTR_GPS_TIME is not a value the raster takes"),
    (dict(value="rgb"), "SWZ_ATTR_RGB is not a value the raster takes"),
    (dict(value="normal"), "SWZ_ATTR_NORMAL is not a value the raster takes"),
    (dict(value=12), "a value that is neither SWZ_RASTER_VALUE_Z nor an attribute of the table"),
    (dict(value=-2), "a value that is neither SWZ_RASTER_VALUE_Z nor an attribute of the table"),
    (dict(reserved=1), "the grid's reserved must be 0"),
    (dict(box_min=[-1e308, 0.0, 0.0], box_max=[1e308, 1.0, 1.0]), "the box is wider than a double holds"),
)


@pytest.mark.parametrize("change,words", REFUSALS, ids=[w[:40] + "/" + ",".join(c) for c, w in REFUSALS])
def test_frame_refusals(swz, change, words):
    args = dict(box_min=[0.0, 0.0, 0.0], box_max=[1.0, 1.0, 1.0], nx=4, ny=4, value="z", reserved=0)
    args.update(change)
    with pytest.raises(swz.SwzError) as e:
        swz.raster_frame_of(**args)
    assert e.value.code == ERR_BAD_ARG and "swz_raster_frame_of: " + words in str(e.value), str(e.value)


def test_what_is_accepted_at_the_edges(swz):
    assert swz.raster_frame_of([0, 0, 0], [1, 1, 1], 1 << 13, 1 << 13)["nx"] == 1 << 13          # exactly SWZ_RASTER_MAX_CELLS
    flat = swz.raster_frame_of([2.0, 3.0, 4.0], [2.0, 3.0, 4.0], 1, 1)                           # a point: one cell, no division
    assert (flat["cw"], flat["ch"], flat["scale"], flat["v0"]) == (0.0, 0.0, 1.0, 4.0)
    for name in RR.ONE_OR_TWO_BYTES:
        f = swz.raster_frame_of([0, 0, 0], [1, 1, 1], 2, 2, name)
        assert (f["v0"], f["scale"], f["value"]) == (0.0, 1.0, swz.ATTRIBUTES[name][0])


def _code(v):
    b = int(np.float64(v).view(np.uint64))
    return (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else b | (1 << 63)


def test_finish_on_a_handmade_table(swz):
    frame = swz.raster_frame_of([0.0, 0.0, -8.0], [5.0, 1.0, 8.0], 5, 1)       # range 16: scale 2^26
    assert frame["scale"] == 2.0 ** 26
    cells = np.zeros(5, dtype=swz.RASTER_CELL_DTYPE)
    cells[0] = (0, 0, 0xFFF0000000000000, 0x000FFFFFFFFFFFFF)                   # empty, as the clear kernel leaves it
    cells[1] = (1, round((1.75 - -8.0) * 2 ** 26), _code(1.75), _code(1.75))   # one row
    cells[2] = (1 << 32, 1 << 62, _code(-8.0), _code(8.0))
    cells[3] = (3, -(1 << 62), _code(-0.0), _code(0.0))
    cells[4] = (2, 3, _code(-7.5), _code(-1e-300))
    got = swz.raster_finish(frame, cells)
    assert got["count"].shape == (1, 5) and got["count"].tolist() == [[0, 1, 1 << 32, 3, 2]]
    assert got["min"][0, 0] == math.inf and got["max"][0, 0] == -math.inf and math.isnan(got["mean"][0, 0])
    assert (got["min"][0, 1], got["max"][0, 1], got["mean"][0, 1]) == (1.75, 1.75, 1.75)
    assert got["mean"][0, 2] == -8.0 + (float(1 << 62) / float(1 << 32)) / 2.0 ** 26 == 8.0
    assert got["mean"][0, 3] == -8.0 + (float(-(1 << 62)) / 3.0) / 2.0 ** 26
    assert math.copysign(1.0, got["min"][0, 3]) == -1.0 and math.copysign(1.0, got["max"][0, 3]) == 1.0
    assert (got["min"][0, 4], got["max"][0, 4]) == (-7.5, -1e-300) and got["mean"][0, 4] == -8.0 + (3.0 / 2.0) / 2.0 ** 26
    # ... and it is the reference's decode
    table = dict(count=cells["count"].copy(), sum=cells["sum"].copy(), min=got["min"].reshape(-1), max=got["max"].reshape(-1))
    want = RR.finish(RR.frame_of([0.0, 0.0, -8.0], [5.0, 1.0, 8.0], 5, 1), table)
    assert np.array_equal(got["mean"], want["mean"], equal_nan=True)
    with pytest.raises(ValueError):
        swz.raster_finish(frame, cells[:4])


def test_struct_sizes_are_the_headers(swz):
    from schwarzwald_amd import api
    header = open(os.path.join(ROOT, "include", "swz_gpu.h")).read()
    source = open(os.path.join(ROOT, "schwarzwald_amd", "csrc", "swz_raster.hip")).read()
    for struct, ctype, size in (("swz_raster_grid", api._RasterGrid, 16), ("swz_raster_frame", api._RasterFrame, 64),
                                ("swz_raster_cell", api._RasterCell, 32)):
        assert C.sizeof(ctype) == size
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (struct, size), header), struct
        assert re.search(r"sizeof\(%s\) == %d\b" % (struct, size), source), struct
    assert api.RASTER_CELL_DTYPE.itemsize == 32 and api.RASTER_CELL_DTYPE.fields["max_code"][1] == 24 == api._RasterCell.max_code.offset
    assert api._RasterFrame.v0.offset == 32 and api._RasterFrame.nx.offset == 48 and api._RasterFrame.value.offset == 56
    assert swz.raster_tile() % 64 == 0 and api.RASTER_MAX_CELLS == 1 << 26 and api.RASTER_VALUE_Z == -1
