"""swz_dataset_query_region: the points of a polygon or of a frustum at a chosen depth, streamed from a written data set and
selected on the device.

The truth per format is tests/region_ref.py (the formulas of include/swz_gpu.h in numpy) over EVERY node file of the data
set, read with the host readers in scan order -- not over the files the call keeps, so a node rule that drops too much shows
as a missing point.  Everything compares exactly."""
import os

import numpy as np
import pytest

import region_ref as R

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ERR_BAD_ARG = 2
COLUMNS = ("rgb", "intensity", "classification", "gps_time")
FORMATS = ("BIN", "LAS", "3DTILES")
POISON = 0xA5


def _cloud():
    """about 20 000 points, half of them on a lattice of 1/16: the outlines' vertices and edges hold points"""
    rng = np.random.default_rng(31415)
    lattice = rng.integers(0, 16, (10000, 3), endpoint=True) / 16.0
    xyz = np.concatenate([lattice, rng.random((10000, 3))])
    n = len(xyz)
    cols = {"rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
            "intensity": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16),
            "classification": rng.integers(0, 31, n, endpoint=True).astype(np.uint8),
            "gps_time": rng.random(n) * 1e9}
    return xyz, cols


def _read_all(swz, directory, fmt):
    """every node file in scan order: positions, columns, per point its node's index in the scan and its depth"""
    scan = swz.dataset_scan(directory)
    ext = {"BIN": ".bin", "LAS": ".las", "3DTILES": ".pnts"}[fmt]
    xyz, cols, node, depth = [], {}, [], []
    for k, (level, key) in enumerate(zip(scan["nodes"]["level"], scan["nodes"]["key"])):
        path = os.path.join(directory, swz.node_name(int(level), int(key)) + ext)
        got = swz.bin_read_node(path, False) if fmt == "BIN" else swz.pnts_read_node(path) if fmt == "3DTILES" else swz.las_read_node(path)
        xyz.append(got[0])
        for name, v in got[1].items():
            cols.setdefault(name, []).append(v)
        node.append(np.full(len(got[0]), k))
        depth.append(np.full(len(got[0]), int(level) + 1))
    return dict(scan=scan, xyz=np.concatenate(xyz), cols={k: np.concatenate(v) for k, v in cols.items()}, node=np.concatenate(node),
                depth=np.concatenate(depth))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    import schwarzwald_amd as swz
    root = tmp_path_factory.mktemp("query_region")
    with swz.Context(0) as ctx:
        spacing = swz.spacing_from_diagonal(*UNIT, 12)
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=400, spacing_at_root=spacing)
        xyz, cols = _cloud()
        with swz.Tiler(ctx, UNIT[0], UNIT[1], params) as t:
            t.add_batch(xyz, cols)
            t.finalize()
            nodes = t.node_table()
            assert int(nodes["level"].max()) >= 1 and 20 <= len(nodes["count"])
            dirs = {}
            for fmt in FORMATS:
                dirs[fmt] = str(root / fmt)
                t.write_output(dirs[fmt], fmt, attrs=COLUMNS)
                t.write_properties(dirs[fmt])
        truth = {fmt: _read_all(swz, dirs[fmt], fmt) for fmt in FORMATS}   # read once, shared, never changed
        yield dict(ctx=ctx, dirs=dirs, truth=truth)


def _frustum():
    import schwarzwald_amd as swz
    return swz.frustum_planes(R.look_at_view_proj((-0.6, -0.4, 1.2), (0.5, 0.5, 0.3)))


# name -> (box, region): outlines on the lattice of the cloud, in both the plain and the awkward kinds
def _queries():
    return {"L": (UNIT, ("polygon", R.L_SHAPE)), "bow_tie": (([0.0, 0.0, 0.25], [1.0, 1.0, 0.625]), ("polygon", R.BOW_TIE)),
            "circle": (UNIT, ("polygon", R.circle(1024))), "frustum": (UNIT, ("planes", _frustum())),
            "dyadic_planes": (UNIT, ("planes", [[1.0, 0.0, 0.0, -0.5], [1.0, 1.0, 0.0, -1.0]]))}


def _expect(T, box, region, max_depth, kept):
    sel = R.region_mask(T["xyz"], box, region)
    if max_depth is not None:
        sel &= T["depth"] <= max_depth
    scan = T["scan"]["nodes"]
    index = {(int(l), int(k)): i for i, (l, k) in enumerate(zip(kept["level"], kept["key"]))}
    at = np.array([index.get((int(l), int(k)), -1) for l, k in zip(scan["level"], scan["key"])])
    return sel, at[T["node"][sel]]


def _query_and_compare(S, fmt, box, region, max_depth, chunk_points, attrs=None):
    import schwarzwald_amd as swz
    T = S["truth"][fmt]
    lossy = fmt == "3DTILES"
    rg = R.as_region(swz, region)
    kept = swz.dataset_query_region_nodes(S["dirs"][fmt], box[0], box[1], rg, max_depth, lossy_source=lossy)
    got = swz.dataset_query_region(S["ctx"], S["dirs"][fmt], box[0], box[1], rg, max_depth=max_depth, attrs=attrs, lossy_source=lossy,
                                   chunk_points=chunk_points, return_nodes=True)
    sel, node = _expect(T, box, region, max_depth, kept)
    assert (node >= 0).all(), "a node that holds a point of the region was dropped"
    assert got["count"] == int(sel.sum()) == got["stats"]["points_out"]
    assert got["xyz"].cpu().numpy().tobytes() == T["xyz"][sel].tobytes()
    names = list(T["cols"]) if attrs is None else list(attrs)
    assert sorted(k for k in got if k not in ("xyz", "node", "count", "stats")) == sorted(names)
    for name in names:
        assert got[name].cpu().numpy().tobytes() == T["cols"][name][sel].tobytes(), name
    assert np.array_equal(got["node"].cpu().numpy(), node.astype(np.int32))
    st = got["stats"]
    assert st["nodes_read"] == len(kept["count"]) <= st["nodes_scanned"] and st["points_read"] == kept["points_bound"]
    return got


@pytest.mark.parametrize("max_depth", [0, 1, None])
@pytest.mark.parametrize("chunk_points", [0, 700])
@pytest.mark.parametrize("fmt", FORMATS)
def test_polygons_and_frustum_at_every_depth(S, fmt, chunk_points, max_depth):
    for name, (box, region) in _queries().items():
        got = _query_and_compare(S, fmt, box, region, max_depth, chunk_points)
        if max_depth is None:
            assert 100 < got["count"] < len(S["truth"][fmt]["xyz"]), name
            assert (got["stats"]["chunks"] > 2) if chunk_points else (got["stats"]["chunks"] == 1)


# an L along two faces of the root: its notch, x and y in (1/4, 1], holds whole nodes of every level below the root
BIG_L = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.25], [0.25, 0.25], [0.25, 1.0], [0.0, 1.0]])


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_l_reads_fewer_nodes_than_its_bounding_box(S, fmt):
    import schwarzwald_amd as swz
    lossy = fmt == "3DTILES"
    got = _query_and_compare(S, fmt, UNIT, ("polygon", BIG_L), None, 0)
    by_box = swz.dataset_query(S["ctx"], S["dirs"][fmt], UNIT[0], UNIT[1], lossy_source=lossy)
    assert got["stats"]["nodes_read"] < by_box["stats"]["nodes_read"] and 100 < got["count"] < by_box["count"]
    # the polygon alone: its x-y bounds and the root's z are the same box
    if not lossy:
        alone = swz.dataset_query_region(S["ctx"], S["dirs"][fmt], None, None, swz.Region.polygon(BIG_L))
        assert alone["count"] == got["count"] and alone["xyz"].cpu().numpy().tobytes() == got["xyz"].cpu().numpy().tobytes()


def test_box_region_and_none_are_the_box_query(S):
    import schwarzwald_amd as swz
    box = ([0.0, 0.25, 0.125], [0.5, 1.0, 0.875])
    want = swz.dataset_query(S["ctx"], S["dirs"]["BIN"], box[0], box[1], chunk_points=700, return_nodes=True)
    for region in (None, swz.Region.box()):
        got = swz.dataset_query_region(S["ctx"], S["dirs"]["BIN"], box[0], box[1], region, chunk_points=700, return_nodes=True)
        assert got["count"] == want["count"] > 100
        for k in ("xyz", "node") + COLUMNS:
            assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("fmt", FORMATS)
def test_attrs_subset(S, fmt):
    box, region = _queries()["circle"]
    got = _query_and_compare(S, fmt, box, region, None, 700, attrs=("intensity",))
    assert "rgb" not in got and got["intensity"].shape[0] == got["count"]


@pytest.mark.parametrize("chunk_points", [0, 700])
@pytest.mark.parametrize("name", ["L", "frustum"])
def test_capacity_one_short(S, name, chunk_points):
    import ctypes as C
    import torch
    import schwarzwald_amd as swz
    from schwarzwald_amd import api
    box, region = _queries()[name]
    rg = R.as_region(swz, region)
    T = S["truth"]["BIN"]
    sel, _ = _expect(T, box, region, None, swz.dataset_query_region_nodes(S["dirs"]["BIN"], box[0], box[1], rg))
    want = int(sel.sum())
    cap, guard = want - 1, 64
    dev = torch.device("cuda", 0)
    xyz = torch.full(((cap + guard) * 24,), POISON, dtype=torch.uint8, device=dev)
    cls = torch.full((cap + guard,), POISON, dtype=torch.uint8, device=dev)
    node = torch.full(((cap + guard) * 4,), POISON, dtype=torch.uint8, device=dev)
    p = api._query_params(box[0], box[1], None, ("classification",), False, chunk_points)
    cols = api.device_columns({"classification": cls.data_ptr()})
    count, stats = C.c_uint64(), api._QueryStats()
    ctx = S["ctx"]
    raw = rg._struct()
    st = ctx._lib.swz_dataset_query_region(ctx._ctx, os.fsencode(S["dirs"]["BIN"]), C.byref(p), C.byref(raw), cap, C.c_void_p(xyz.data_ptr()),
                                           C.byref(cols), C.c_void_p(node.data_ptr()), C.byref(count), C.byref(stats))
    torch.cuda.synchronize()
    text = ctx._lib.swz_last_error(ctx._ctx).decode()
    assert st == ERR_BAD_ARG and "capacity" in text and "swz_dataset_query_region" in text
    assert cap < count.value <= want and (chunk_points or count.value == want)
    # nothing at or beyond capacity rows
    assert (xyz.cpu().numpy()[cap * 24:] == POISON).all() and (cls.cpu().numpy()[cap:] == POISON).all()
    assert (node.cpu().numpy()[cap * 4:] == POISON).all()
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_region(ctx, S["dirs"]["BIN"], box[0], box[1], rg, chunk_points=chunk_points, capacity=cap)
    assert "capacity" in str(e.value)
    assert swz.dataset_query_region(ctx, S["dirs"]["BIN"], box[0], box[1], rg, chunk_points=chunk_points, capacity=want)["count"] == want


def test_a_refused_region_reads_nothing(S):
    import schwarzwald_amd as swz
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_region(S["ctx"], str(os.path.join(S["dirs"]["BIN"], "missing")), UNIT[0], UNIT[1], swz.Region.planes([[0.0, 0.0, 0.0, 1.0]]))
    assert e.value.code == ERR_BAD_ARG and "swz_dataset_query_region" in str(e.value) and "a = b = c = 0" in str(e.value)
