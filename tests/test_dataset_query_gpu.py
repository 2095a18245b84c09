"""swz_dataset_query: the points of a box at a chosen depth, streamed from a written data set and selected on the device.

The truth per format is numpy over EVERY node file of the data set, read with the host readers in scan order -- not over
the files the call keeps, so a node box that is widened too little shows as a missing point.  Everything compares exactly."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ERR_BAD_ARG = 2
COLUMNS = ("rgb", "intensity", "classification", "gps_time")
FORMATS = ("BIN", "BINZ", "LAS", "ENTWINE_LAS", "3DTILES")
POISON = 0xA5


def _cloud():
    """about 20 000 points, half of them on a lattice of 1/16: octant faces, node faces and the root's faces hold points"""
    rng = np.random.default_rng(2718)
    lattice = rng.integers(0, 16, (10000, 3), endpoint=True) / 16.0
    xyz = np.concatenate([lattice, rng.random((10000, 3))])
    n = len(xyz)
    cols = {"rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
            "intensity": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16),
            "classification": rng.integers(0, 31, n, endpoint=True).astype(np.uint8),
            "gps_time": rng.random(n) * 1e9}
    return xyz, cols


def _node_file(swz, directory, fmt, level, key):
    if fmt == "ENTWINE_LAS":
        return os.path.join(directory, "ept-data", swz.node_name_entwine(level, key) + ".las")
    return os.path.join(directory, swz.node_name(level, key) + {"BIN": ".bin", "BINZ": ".binz", "LAS": ".las", "3DTILES": ".pnts"}[fmt])


def _read_all(swz, directory, fmt):
    """every node file in scan order: positions, columns, per point its node's index in the scan and its depth"""
    scan = swz.dataset_scan(directory)
    xyz, cols, node, depth = [], {}, [], []
    for k, (level, key) in enumerate(zip(scan["nodes"]["level"], scan["nodes"]["key"])):
        path = _node_file(swz, directory, fmt, int(level), int(key))
        got = swz.bin_read_node(path, fmt == "BINZ") if fmt in ("BIN", "BINZ") else swz.pnts_read_node(path) if fmt == "3DTILES" \
            else swz.las_read_node(path)
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
    root = tmp_path_factory.mktemp("query")
    with swz.Context(0) as ctx:
        spacing = swz.spacing_from_diagonal(*UNIT, 12)
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=400, spacing_at_root=spacing)
        xyz, cols = _cloud()
        with swz.Tiler(ctx, UNIT[0], UNIT[1], params) as t:
            t.add_batch(xyz, cols)
            t.finalize()
            info, nodes = t.info(), t.node_table()
            assert int(nodes["level"].max()) >= 1 and 20 <= len(nodes["count"])    # three or more levels, a few dozen nodes
            dirs = {}
            for fmt in FORMATS:
                dirs[fmt] = str(root / fmt)
                extra = dict(ept=dict(bounds=UNIT, conforming_bounds=UNIT, points=int(info["num_points"]), attrs=COLUMNS, span=128.0,
                                      srs=dict(authority="EPSG", horizontal="25832", wkt="wkt"), version="1.0.0")) if fmt == "ENTWINE_LAS" else {}
                t.write_output(dirs[fmt], fmt, attrs=COLUMNS, **extra)
                if fmt != "ENTWINE_LAS":
                    t.write_properties(dirs[fmt])
        truth = {fmt: _read_all(swz, dirs[fmt], fmt) for fmt in FORMATS}   # read once, shared, never changed
        yield dict(ctx=ctx, dirs=dirs, truth=truth, nodes=nodes)


def _boxes(S):
    """name -> (min, max)"""
    import schwarzwald_amd as swz
    nodes = S["nodes"]
    out = {"root": UNIT, "far": ([5.0, 5.0, 5.0], [6.0, 6.0, 6.0]), "slab": ([0.0, 0.0, 0.40625], [1.0, 1.0, 0.40625 + 2.0 ** -12])}
    for o in range(8):
        lo = [0.5 * ((o >> a) & 1) for a in range(3)]
        out["octant%d" % o] = (lo, [v + 0.5 for v in lo])
    deepest = int(np.argmax(nodes["level"]))
    out["leaf"] = swz.node_bounds(int(nodes["level"][deepest]), int(nodes["key"][deepest]), *UNIT)
    out["leaf"] = (list(out["leaf"][0]), list(out["leaf"][1]))
    p = S["truth"]["BIN"]["xyz"][12345 % len(S["truth"]["BIN"]["xyz"])]
    out["point"] = ((p - 1e-9).tolist(), (p + 1e-9).tolist())
    return out


BOX_NAMES = ["root", "far", "slab", "leaf", "point"] + ["octant%d" % o for o in range(8)]


def _expect(T, box, max_depth, kept):
    """the rows of the truth inside the box, and per row the index of its node in the kept table"""
    lo, hi = np.asarray(box[0]), np.asarray(box[1])
    sel = ((T["xyz"] >= lo) & (T["xyz"] <= hi)).all(axis=1)
    if max_depth is not None:
        sel &= T["depth"] <= max_depth
    scan = T["scan"]["nodes"]
    index = {(int(l), int(k)): i for i, (l, k) in enumerate(zip(kept["level"], kept["key"]))}
    at = np.array([index.get((int(l), int(k)), -1) for l, k in zip(scan["level"], scan["key"])])
    return sel, at[T["node"][sel]]


def _query_and_compare(S, fmt, box, max_depth, chunk_points, attrs=None):
    import schwarzwald_amd as swz
    T = S["truth"][fmt]
    lossy = fmt == "3DTILES"
    kept = swz.dataset_query_nodes(S["dirs"][fmt], box[0], box[1], max_depth, lossy_source=lossy)
    got = swz.dataset_query(S["ctx"], S["dirs"][fmt], box[0], box[1], max_depth=max_depth, attrs=attrs, lossy_source=lossy,
                            chunk_points=chunk_points, return_nodes=True)
    sel, node = _expect(T, box, max_depth, kept)
    assert (node >= 0).all(), "a node that holds a point of the box was dropped"
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
def test_boxes_and_depths(S, fmt, chunk_points, max_depth):
    boxes = _boxes(S)
    for name in BOX_NAMES:
        got = _query_and_compare(S, fmt, boxes[name], max_depth, chunk_points)
        st = got["stats"]
        if name == "root" and max_depth is None:
            assert got["count"] == len(S["truth"][fmt]["xyz"]) and st["nodes_read"] == st["nodes_scanned"]
            assert (st["chunks"] > 4) if chunk_points else (st["chunks"] == 1)
        if name == "far":
            assert got["count"] == 0 and st["nodes_read"] == 0
        if name == "slab" and max_depth is None:
            assert st["nodes_read"] < st["nodes_scanned"]
        if name in ("leaf", "point") and max_depth is None:
            assert got["count"] >= 1
        if name.startswith("octant") and max_depth is None:
            assert got["count"] > 1000


def test_octants_share_the_points_on_their_faces(S):
    boxes, T = _boxes(S), S["truth"]["BIN"]
    total = sum(int(((T["xyz"] >= np.asarray(boxes["octant%d" % o][0])) & (T["xyz"] <= np.asarray(boxes["octant%d" % o][1]))).all(axis=1).sum())
                for o in range(8))
    assert total > len(T["xyz"])


@pytest.mark.parametrize("fmt", ["BIN", "LAS", "3DTILES"])
def test_attrs_subset(S, fmt):
    got = _query_and_compare(S, fmt, _boxes(S)["octant5"], None, 700, attrs=("intensity",))
    assert "rgb" not in got and got["intensity"].shape[0] == got["count"]


def test_3dtiles_needs_the_lossy_flag(S):
    import schwarzwald_amd as swz
    for call in (lambda: swz.dataset_query(S["ctx"], S["dirs"]["3DTILES"], *UNIT), lambda: swz.dataset_query_nodes(S["dirs"]["3DTILES"], *UNIT)):
        with pytest.raises(swz.SwzError) as e:
            call()
        assert e.value.code == ERR_BAD_ARG and "a 3DTILES source is converted only with SWZ_CONVERT_LOSSY_SOURCE in source_flags" in str(e.value)
        assert "swz_dataset_query" in str(e.value)


@pytest.mark.parametrize("chunk_points", [0, 700])
def test_capacity_one_short(S, chunk_points):
    import ctypes as C
    import torch
    import schwarzwald_amd as swz
    from schwarzwald_amd import api
    box = _boxes(S)["octant3"]
    T = S["truth"]["BIN"]
    sel, _ = _expect(T, box, None, swz.dataset_query_nodes(S["dirs"]["BIN"], *box))
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
    st = ctx._lib.swz_dataset_query(ctx._ctx, os.fsencode(S["dirs"]["BIN"]), C.byref(p), cap, C.c_void_p(xyz.data_ptr()), C.byref(cols),
                                    C.c_void_p(node.data_ptr()), C.byref(count), C.byref(stats))
    torch.cuda.synchronize()
    assert st == ERR_BAD_ARG and "capacity" in ctx._lib.swz_last_error(ctx._ctx).decode()
    assert cap < count.value <= want and (chunk_points or count.value == want)
    # nothing at or beyond capacity rows; what lies in front of it is the truth's
    assert (xyz.cpu().numpy()[cap * 24:] == POISON).all() and (cls.cpu().numpy()[cap:] == POISON).all()
    assert (node.cpu().numpy()[cap * 4:] == POISON).all()
    # and the Python call refuses in the same words
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query(ctx, S["dirs"]["BIN"], box[0], box[1], chunk_points=chunk_points, capacity=cap)
    assert "capacity" in str(e.value)
    assert swz.dataset_query(ctx, S["dirs"]["BIN"], box[0], box[1], chunk_points=chunk_points, capacity=want)["count"] == want
