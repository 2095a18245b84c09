"""swz_dataset_rasterize on small data sets in all five formats.  The oracle is code that has tests of its own: the raster of a
data set must be tests/raster_ref.py over the rows swz_dataset_query_filtered returns for the same box, region, filter and
depth -- every field of every cell exactly.  The box-alone path (one pass over the chunk-local rows) and the compacting path
(selection first) give the same bytes, as do small chunks and the default, and a query with and without node-summaries.swz."""
import os
import shutil

import numpy as np
import pytest

import filter_ref as F
import raster_ref as RR
import region_ref as R

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
SUB = ([0.2, 0.1, 0.3], [0.8, 0.9, 0.7])
ERR_BAD_ARG = 2
COLUMNS = ("rgb",) + F.SCALARS
FORMATS = ("BIN", "BINZ", "LAS", "ENTWINE_LAS", "3DTILES")
WRITTEN = {fmt: COLUMNS for fmt in FORMATS[:4]}
WRITTEN["3DTILES"] = ("rgb", "intensity")
CHUNK = 500
NX, NY = 16, 12
BIG_L = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.25], [0.25, 0.25], [0.25, 1.0], [0.0, 1.0]])
FILTER = [("any_of", "classification", [2]), ("range", "gps_time", 0, 6e4)]
FILTER_LOSSY = [("range", "intensity", 0, 20000)]           # all a .pnts file carries beside RGB
NARROW = [("range", "point_source_id", 1, 1)]               # one flight strip: a quarter of the nodes can hold it


def _cloud():
    """the cloud of tests/test_dataset_summarize_gpu.py: the columns follow the positions"""
    rng = np.random.default_rng(2718)
    n = 8000
    xyz = rng.random((n, 3))
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    cols = {"rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
            "intensity": np.floor(x * 50000).astype(np.uint16),
            "classification": np.where(z < 0.35, 2, rng.choice([3, 4, 5, 6, 9], n)).astype(np.uint8),
            "edge_of_flight_line": rng.integers(0, 1, n, endpoint=True).astype(np.uint8),
            "gps_time": 1e5 * y,
            "number_of_returns": rng.integers(3, 5, n, endpoint=True).astype(np.uint8),
            "return_number": rng.integers(1, 3, n, endpoint=True).astype(np.uint8),
            "point_source_id": (1 + np.floor(x * 4)).astype(np.uint16),
            "scan_direction_flag": rng.integers(0, 1, n, endpoint=True).astype(np.uint8),
            "scan_angle_rank": np.where(x < 0.5, -1 - np.floor(x * 250), np.floor(x * 127)).astype(np.int8),
            "user_data": rng.integers(0, 255, n, endpoint=True).astype(np.uint8)}
    return xyz, cols


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    import schwarzwald_amd as swz
    root = tmp_path_factory.mktemp("rasterize")
    with swz.Context(0) as ctx:
        spacing = swz.spacing_from_diagonal(*UNIT, 12)
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=150, spacing_at_root=spacing)
        xyz, cols = _cloud()
        with swz.Tiler(ctx, UNIT[0], UNIT[1], params) as t:
            t.add_batch(xyz, cols)
            t.finalize()
            info = t.info()
            dirs = {}
            for fmt in FORMATS:
                dirs[fmt] = str(root / fmt)
                attrs = WRITTEN[fmt]
                extra = dict(ept=dict(bounds=UNIT, conforming_bounds=UNIT, points=int(info["num_points"]), attrs=attrs, span=128.0,
                                      srs=dict(authority="EPSG", horizontal="25832", wkt="wkt"), version="1.0.0")) if fmt == "ENTWINE_LAS" else {}
                t.write_output(dirs[fmt], fmt, attrs=attrs, **extra)
                if fmt != "ENTWINE_LAS":
                    t.write_properties(dirs[fmt])
        yield dict(swz=swz, ctx=ctx, dirs=dirs, root=root)


def _raster(D, fmt, box=UNIT, value="z", region=None, filter=None, directory=None, **kwargs):
    swz = D["swz"]
    kwargs.setdefault("chunk_points", CHUNK)
    return swz.dataset_rasterize(D["ctx"], directory or D["dirs"][fmt], box[0], box[1], NX, NY, value=value, region=R.as_region(swz, region),
                                 filter=F.as_filter(swz, filter), lossy_source=fmt == "3DTILES", **kwargs)


def _expect(D, fmt, box=UNIT, value="z", region=None, filter=None, max_depth=None):
    """raster_ref over the rows of the filtered query"""
    swz = D["swz"]
    q = swz.dataset_query_filtered(D["ctx"], D["dirs"][fmt], box[0], box[1], R.as_region(swz, region), F.as_filter(swz, filter), max_depth=max_depth,
                                   attrs=[] if value == "z" else [value], lossy_source=fmt == "3DTILES", chunk_points=CHUNK)
    xyz = q["xyz"].cpu().numpy()
    column = None if value == "z" else q[value].cpu().numpy()
    frame, table = RR.raster(box, NX, NY, xyz, value, column)
    assert int(table["count"].sum()) == q["count"]          # (the query's rows are the box's)
    return frame, table, q


def _same(got, frame, table, q):
    assert RR.same_table(got, frame, table)
    fin = RR.finish(frame, table)
    assert np.array_equal(got["mean"], fin["mean"], equal_nan=True)
    for k in ("x0", "y0", "cw", "ch", "v0", "scale"):
        assert got["frame"][k] == frame[k], k
    assert got["stats"]["points_out"] == q["count"] == int(got["count"].sum())
    for k in ("nodes_scanned", "nodes_read", "points_read", "bytes_read", "chunks"):
        assert got["stats"][k] == q["stats"][k] or k == "bytes_read", k      # (the raster unpacks fewer columns, not fewer files)


@pytest.mark.parametrize("fmt", FORMATS)
def test_raster_is_the_reference_over_the_querys_rows(D, fmt):
    filter = FILTER_LOSSY if fmt == "3DTILES" else FILTER
    selections = {"unit": dict(), "sub": dict(box=SUB), "polygon": dict(region=("polygon", BIG_L)), "filter": dict(filter=filter),
                  "polygon+filter": dict(region=("polygon", BIG_L), filter=filter), "depth": dict(max_depth=1)}
    counts = {}
    for name, sel in selections.items():
        got = _raster(D, fmt, **sel)
        frame, table, q = _expect(D, fmt, **sel)
        _same(got, frame, table, q)
        counts[name] = q["count"]
        assert got["count"].shape == (NY, NX) and got["stats"]["chunks"] >= (2 if name != "depth" else 1), name
    assert fmt not in ("BIN", "BINZ") or counts["unit"] == 8000    # (the other formats round what they store)
    assert counts["unit"] > counts["sub"] > 0 and counts["unit"] > counts["polygon"] > counts["polygon+filter"] > 0
    assert counts["unit"] > counts["filter"] > 0 and counts["unit"] > counts["depth"] > 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_value_intensity(D, fmt):
    for sel in (dict(), dict(region=("polygon", BIG_L))):
        got = _raster(D, fmt, value="intensity", **sel)
        frame, table, q = _expect(D, fmt, value="intensity", **sel)
        _same(got, frame, table, q)
    assert got["frame"]["scale"] == 1.0 and got["max"].max() <= 65535.0


@pytest.mark.parametrize("fmt", FORMATS)
def test_value_classification(D, fmt):
    swz = D["swz"]
    if fmt == "3DTILES":
        with pytest.raises(swz.SwzError) as e:
            _raster(D, fmt, value="classification")
        assert e.value.code == ERR_BAD_ARG and "swz_dataset_rasterize: the value is SWZ_ATTR_CLASSIFICATION, which .pnts files do not carry" in str(e.value)
        return
    got = _raster(D, fmt, value="classification", filter=FILTER)
    frame, table, q = _expect(D, fmt, value="classification", filter=FILTER)
    _same(got, frame, table, q)
    held = got["count"] > 0
    assert held.any() and np.all(got["min"][held] == 2.0) and np.all(got["sum"][held] == 2 * got["count"][held].astype(np.int64))
    got = _raster(D, fmt, SUB, value="scan_angle_rank")
    frame, table, q = _expect(D, fmt, SUB, value="scan_angle_rank")
    _same(got, frame, table, q)
    assert got["min"].min() < 0.0


@pytest.mark.parametrize("fmt", FORMATS)
def test_box_alone_is_the_compacting_path(D, fmt):
    """a plane that keeps every row sends the same rows through the selection first: the same bytes.  The plane is z + 1 >= 0:
    the library refuses (0, 0, 0, 1), a plane with a = b = c = 0, for every region call."""
    for value in ("z", "intensity"):
        alone = _raster(D, fmt, SUB, value=value)
        compacted = _raster(D, fmt, SUB, value=value, region=("planes", [[0.0, 0.0, 1.0, 1.0]]))
        assert alone["stats"]["points_out"] == compacted["stats"]["points_out"] > 0
        assert alone["cells"].tobytes() == compacted["cells"].tobytes()
        as_box_region = _raster(D, fmt, SUB, value=value, region=("box",))
        assert as_box_region["cells"].tobytes() == alone["cells"].tobytes()


@pytest.mark.parametrize("fmt", ("BIN", "LAS", "3DTILES"))
def test_chunking_does_not_show(D, fmt):
    filter = FILTER_LOSSY if fmt == "3DTILES" else FILTER
    for sel in (dict(), dict(region=("polygon", BIG_L), filter=filter)):
        small = _raster(D, fmt, **sel)
        whole = _raster(D, fmt, chunk_points=0, **sel)
        assert small["stats"]["chunks"] > whole["stats"]["chunks"] >= 1
        assert small["cells"].tobytes() == whole["cells"].tobytes()


def test_summaries_let_a_narrow_filter_skip_nodes(D):
    swz, ctx = D["swz"], D["ctx"]
    directory = str(D["root"] / "summarized")
    shutil.copytree(D["dirs"]["BIN"], directory)
    before = _raster(D, "BIN", filter=NARROW, directory=directory)
    ctx.dataset_summarize(directory, chunk_points=CHUNK)
    after = _raster(D, "BIN", filter=NARROW, directory=directory)
    assert after["cells"].tobytes() == before["cells"].tobytes() and before["stats"]["points_out"] > 0
    assert after["stats"]["nodes_read"] < before["stats"]["nodes_read"] and after["stats"]["points_read"] < before["stats"]["points_read"]
    flags = swz.dataset_query_filtered_nodes(directory, UNIT[0], UNIT[1], None, F.as_filter(swz, NARROW))
    assert after["stats"]["nodes_read"] == int(flags["read"].sum())
    # the box alone never looks at the sidecar
    assert _raster(D, "BIN", directory=directory)["cells"].tobytes() == _raster(D, "BIN")["cells"].tobytes()


def test_a_truncated_node_file_is_named(D):
    swz = D["swz"]
    directory = str(D["root"] / "truncated")
    shutil.copytree(D["dirs"]["BIN"], directory)
    scan = swz.dataset_scan(directory)
    k = len(scan["nodes"]["key"]) // 2
    path = os.path.join(directory, swz.node_name(int(scan["nodes"]["level"][k]), int(scan["nodes"]["key"][k])) + ".bin")
    size = os.path.getsize(path)
    with open(path, "r+b") as f:
        f.truncate(size - 40)
    for sel in (dict(), dict(filter=FILTER)):
        with pytest.raises(swz.SwzError) as e:
            _raster(D, "BIN", directory=directory, **sel)
        assert e.value.code == ERR_BAD_ARG and "swz_dataset_rasterize: cannot read the arrays of " + path in str(e.value), str(e.value)
    # the context goes on
    assert _raster(D, "BIN")["stats"]["points_out"] == 8000


def test_what_the_call_refuses_and_defaults(D):
    swz, ctx = D["swz"], D["ctx"]
    directory = D["dirs"]["BIN"]
    for kwargs, words in ((dict(nx=0), "swz_dataset_rasterize: nx or ny is 0"), (dict(value="gps_time"), "SWZ_ATTR_GPS_TIME is not a value the raster takes"),
                          (dict(box_max=[1.0, 0.0, 1.0], nx=4), "the box is flat along y (box_min == box_max) and ny is not 1")):
        args = dict(box_min=UNIT[0], box_max=UNIT[1], nx=NX, ny=NY)
        args.update(kwargs)
        with pytest.raises(swz.SwzError) as e:
            swz.dataset_rasterize(ctx, directory, **args)
        assert e.value.code == ERR_BAD_ARG and words in str(e.value), str(e.value)
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_rasterize(ctx, D["dirs"]["3DTILES"], UNIT[0], UNIT[1], NX, NY)
    assert "a 3DTILES source is converted only with" in str(e.value)
    # a source without the value's column: a BIN data set of positions and colours
    bare = str(D["root"] / "bare")
    swz.convert_dataset(ctx, directory, bare, "BIN", attrs=("rgb",))
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_rasterize(ctx, bare, UNIT[0], UNIT[1], NX, NY, value="intensity")
    assert "swz_dataset_rasterize: the value is SWZ_ATTR_INTENSITY, which the source does not hold (its attribute mask is 0x1)" in str(e.value), str(e.value)
    assert swz.dataset_rasterize(ctx, bare, UNIT[0], UNIT[1], NX, NY)["cells"].tobytes() == _raster(D, "BIN")["cells"].tobytes()
    # no box: the root box; a polygon without a box: its x-y bounds and the root's z
    whole = ctx.dataset_rasterize(directory, None, None, NX, NY, chunk_points=CHUNK)
    assert whole["cells"].tobytes() == _raster(D, "BIN")["cells"].tobytes()
    outline = R.L_SHAPE
    derived = ctx.dataset_rasterize(directory, None, None, NX, NY, region=swz.Region.polygon(outline), chunk_points=CHUNK)
    given = _raster(D, "BIN", ([0.25, 0.25, 0.0], [0.75, 0.75, 1.0]), region=("polygon", outline))
    assert derived["cells"].tobytes() == given["cells"].tobytes() and derived["stats"]["points_out"] > 0
