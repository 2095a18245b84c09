"""swz_dataset_query_filtered: the points of a region that pass a filter over the attribute columns, streamed from a written
data set and selected on the device.

The truth per format is tests/filter_ref.py on tests/region_ref.py (the contract of include/swz_gpu.h in numpy) over EVERY
node file of the data set, read with the host readers in scan order -- not over the files the call keeps.  The filter sees the
values the source's own readers yield.  Everything compares exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_ref as F
import region_ref as R

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ERR_BAD_ARG = 2
POISON = 0xA5
COLUMNS = ("rgb",) + F.SCALARS
FORMATS = ("BIN", "BINZ", "LAS", "ENTWINE_LAS", "3DTILES")
WRITTEN = {fmt: COLUMNS for fmt in FORMATS[:4]}
WRITTEN["3DTILES"] = ("rgb", "intensity")
CHUNK = 500
# an L along two faces of the root: its notch is x and y in (1/4, 1]
BIG_L = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.25], [0.25, 0.25], [0.25, 1.0], [0.0, 1.0]])
REGIONS = {"box": None, "polygon": ("polygon", BIG_L), "planes": ("planes", [[-1.0, -1.0, 0.0, 1.2]])}
# The columns follow the positions, so a filter takes and leaves whole nodes: the strip (point source id) and the intensity
# grow with x, the GPS time with y, and the ground (class 2) lies below z = 0.35.
FILTERS = {"box": [("range", "point_source_id", 1, 2), ("none_of", "classification", [7, 18])],
           "polygon": [("any_of", "classification", [2]), ("range", "return_number", 1, 3)],
           "planes": [("range", "gps_time", -float("inf"), 4.5e4), ("not_range", "scan_angle_rank", 100, 127)]}
LOSSY_FILTER = [("range", "intensity", 0, 22000)]           # all a .pnts file carries beside RGB


def _cloud():
    rng = np.random.default_rng(1618)
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
            "scan_angle_rank": rng.integers(-90, 90, n, endpoint=True).astype(np.int8),
            "user_data": rng.integers(0, 255, n, endpoint=True).astype(np.uint8)}
    return xyz, cols


def _node_file(swz, directory, fmt, level, key):
    if fmt == "ENTWINE_LAS":
        return os.path.join(directory, "ept-data", swz.node_name_entwine(level, key) + ".las")
    return os.path.join(directory, swz.node_name(level, key) + {"BIN": ".bin", "BINZ": ".binz", "LAS": ".las", "3DTILES": ".pnts"}[fmt])


def _read_all(swz, directory, fmt):
    """every node file in scan order: positions, columns, per point its node's index in the scan"""
    scan = swz.dataset_scan(directory)
    xyz, cols, node = [], {}, []
    for k, (level, key) in enumerate(zip(scan["nodes"]["level"], scan["nodes"]["key"])):
        path = _node_file(swz, directory, fmt, int(level), int(key))
        got = swz.bin_read_node(path, fmt == "BINZ") if fmt in ("BIN", "BINZ") else swz.pnts_read_node(path) if fmt == "3DTILES" \
            else swz.las_read_node(path)
        xyz.append(got[0])
        for name, v in got[1].items():
            cols.setdefault(name, []).append(v)
        node.append(np.full(len(got[0]), k))
    return dict(scan=scan, xyz=np.concatenate(xyz), cols={k: np.concatenate(v) for k, v in cols.items()}, node=np.concatenate(node))


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    import schwarzwald_amd as swz
    root = tmp_path_factory.mktemp("query_filtered")
    with swz.Context(0) as ctx:
        spacing = swz.spacing_from_diagonal(*UNIT, 12)
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=150, spacing_at_root=spacing)
        xyz, cols = _cloud()
        with swz.Tiler(ctx, UNIT[0], UNIT[1], params) as t:
            t.add_batch(xyz, cols)
            t.finalize()
            info, nodes = t.info(), t.node_table()
            assert int(nodes["level"].max()) >= 1 and 20 <= len(nodes["count"])    # three or more levels
            dirs = {}
            for fmt in FORMATS + ("FEW",):
                dirs[fmt] = str(root / fmt)
                attrs = WRITTEN.get(fmt, ("rgb", "intensity"))                     # FEW: a BIN data set without most columns
                extra = dict(ept=dict(bounds=UNIT, conforming_bounds=UNIT, points=int(info["num_points"]), attrs=attrs, span=128.0,
                                      srs=dict(authority="EPSG", horizontal="25832", wkt="wkt"), version="1.0.0")) if fmt == "ENTWINE_LAS" else {}
                t.write_output(dirs[fmt], "BIN" if fmt == "FEW" else fmt, attrs=attrs, **extra)
                if fmt != "ENTWINE_LAS":
                    t.write_properties(dirs[fmt])
        truth = {fmt: _read_all(swz, dirs[fmt], fmt) for fmt in FORMATS}   # read once, shared, never changed
        yield dict(ctx=ctx, dirs=dirs, truth=truth)


def _expect(swz, T, region, filter, kept):
    """the selected rows of the whole scan, their nodes as indices into `kept`, and per kept node how many of its rows pass"""
    sel = F.select_mask(T["xyz"], T["cols"], UNIT, region, filter)
    scan = T["scan"]["nodes"]
    index = {(int(l), int(k)): i for i, (l, k) in enumerate(zip(kept["level"], kept["key"]))}
    at = np.array([index.get((int(l), int(k)), -1) for l, k in zip(scan["level"], scan["key"])])
    node = at[T["node"][sel]]
    return sel, node, np.bincount(node[node >= 0], minlength=len(kept["count"]))


@pytest.mark.parametrize("kind", list(REGIONS))
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_source_by_box_polygon_and_planes(S, fmt, kind):
    import schwarzwald_amd as swz
    T = S["truth"][fmt]
    lossy = fmt == "3DTILES"
    region, filter = REGIONS[kind], LOSSY_FILTER if lossy else FILTERS[kind]
    rg, fl = R.as_region(swz, region), F.as_filter(swz, filter)
    kept = swz.dataset_query_region_nodes(S["dirs"][fmt], UNIT[0], UNIT[1], rg, lossy_source=lossy)
    sel, node, per_node = _expect(swz, T, region, filter, kept)
    # the numpy side first: the case is what it is meant to be
    n = len(T["xyz"])
    assert 6000 <= n <= 9000 and 0.05 * n < sel.sum() < 0.95 * n
    first = swz.output_chunks(kept["count"], CHUNK)
    assert len(first) - 1 >= 4
    per_chunk = [int(per_node[int(first[j]):int(first[j + 1])].sum()) for j in range(len(first) - 1)]
    assert min(per_chunk) == 0, "no chunk selects nothing"
    assert ((per_node == kept["count"]) & (kept["count"] > 0)).any(), "no node passes whole"
    assert (node >= 0).all()
    # the columns asked back: all the source holds, or (polygon) one column that the filter does not read
    attrs = ("rgb",) if kind == "polygon" else None
    got = swz.dataset_query_filtered(S["ctx"], S["dirs"][fmt], UNIT[0], UNIT[1], rg, fl, attrs=attrs, lossy_source=lossy, chunk_points=CHUNK,
                                     return_nodes=True)
    assert got["count"] == int(sel.sum()) == got["stats"]["points_out"]
    assert got["xyz"].cpu().numpy().tobytes() == T["xyz"][sel].tobytes()
    names = list(WRITTEN[fmt]) if attrs is None else list(attrs)
    assert sorted(k for k in got if k not in ("xyz", "node", "count", "stats")) == sorted(names)
    for name in names:
        assert got[name].cpu().numpy().tobytes() == T["cols"][name][sel].tobytes(), name
    assert np.array_equal(got["node"].cpu().numpy(), node.astype(np.int32))
    # no node is dropped for a filter: the table and the stats are the region query's
    st = got["stats"]
    assert st["nodes_read"] == len(kept["count"]) and st["points_read"] == kept["points_bound"] and st["chunks"] == len(first) - 1
    assert st["points_read"] - st["points_out"] > 0


def test_no_filter_is_the_region_query(S):
    import schwarzwald_amd as swz
    rg = R.as_region(swz, REGIONS["polygon"])
    want = swz.dataset_query_region(S["ctx"], S["dirs"]["BIN"], UNIT[0], UNIT[1], rg, chunk_points=CHUNK, return_nodes=True)
    for filter in (None, swz.Filter()):
        got = swz.dataset_query_filtered(S["ctx"], S["dirs"]["BIN"], UNIT[0], UNIT[1], rg, filter, chunk_points=CHUNK, return_nodes=True)
        assert got["count"] == want["count"] > 100
        for k in ("xyz", "node") + COLUMNS:
            assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k


def test_an_attribute_the_source_lacks_is_refused_by_name(S):
    import schwarzwald_amd as swz
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_filtered(S["ctx"], S["dirs"]["FEW"], UNIT[0], UNIT[1], None, swz.Filter().any_of("classification", [2]))
    text = str(e.value)
    assert e.value.code == ERR_BAD_ARG and "swz_dataset_query_filtered" in text and "the filter names SWZ_ATTR_CLASSIFICATION," in text and "0x5" in text, text
    # the columns it holds are in order
    got = swz.dataset_query_filtered(S["ctx"], S["dirs"]["FEW"], UNIT[0], UNIT[1], None, swz.Filter().range("intensity", 0, 22000), attrs=("rgb",))
    assert 0 < got["count"] < len(S["truth"]["BIN"]["xyz"])


def test_classification_on_a_3dtiles_source_is_refused(S):
    import schwarzwald_amd as swz
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_filtered(S["ctx"], S["dirs"]["3DTILES"], UNIT[0], UNIT[1], None, swz.Filter().any_of("classification", [2]),
                                   lossy_source=True)
    text = str(e.value)
    assert e.value.code == ERR_BAD_ARG and "the filter names SWZ_ATTR_CLASSIFICATION," in text and ".pnts" in text, text


def test_a_refused_filter_reads_nothing(S):
    import schwarzwald_amd as swz
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_filtered(S["ctx"], os.path.join(S["dirs"]["BIN"], "missing"), UNIT[0], UNIT[1], None, swz.Filter().range("rgb", 0, 1))
    assert e.value.code == ERR_BAD_ARG and "clause 0" in str(e.value) and "SWZ_ATTR_RGB is not a scalar" in str(e.value)
    # through the C call itself, which does its own check
    from schwarzwald_amd import api
    ctx = S["ctx"]
    p = api._query_params(UNIT[0], UNIT[1], None, (), False, 0)
    bad = swz.Filter().range("intensity", 2, 1)._struct()
    count = C.c_uint64()
    st = ctx._lib.swz_dataset_query_filtered(ctx._ctx, os.fsencode(os.path.join(S["dirs"]["BIN"], "missing")), C.byref(p), None, C.byref(bad), 0,
                                             None, None, None, C.byref(count), None)
    text = ctx._lib.swz_last_error(ctx._ctx).decode()
    assert st == ERR_BAD_ARG and "swz_dataset_query_filtered: clause 0: a RANGE with lo > hi" in text, text


def test_capacity_refusal_in_mid_stream(S):
    import torch
    import schwarzwald_amd as swz
    from schwarzwald_amd import api
    region, filter = REGIONS["planes"], FILTERS["planes"]
    rg, fl = R.as_region(swz, region), F.as_filter(swz, filter)
    T = S["truth"]["BIN"]
    kept = swz.dataset_query_region_nodes(S["dirs"]["BIN"], UNIT[0], UNIT[1], rg)
    sel, node, per_node = _expect(swz, T, region, filter, kept)
    want = int(sel.sum())
    first = swz.output_chunks(kept["count"], CHUNK)
    upto = np.cumsum([int(per_node[int(first[j]):int(first[j + 1])].sum()) for j in range(len(first) - 1)])
    cap = int(upto[len(upto) // 2 - 1]) - 1                      # one short of what the first half of the chunks selects
    stops = int(upto[np.argmax(upto > cap)])                     # the total up to and including the chunk that passes it
    assert 0 < cap < stops <= want and stops - cap <= CHUNK + 150
    guard = 64
    dev = torch.device("cuda", 0)
    xyz = torch.full(((cap + guard) * 24,), POISON, dtype=torch.uint8, device=dev)
    inten = torch.full(((cap + guard) * 2,), POISON, dtype=torch.uint8, device=dev)
    nodes = torch.full(((cap + guard) * 4,), POISON, dtype=torch.uint8, device=dev)
    p = api._query_params(UNIT[0], UNIT[1], None, ("intensity",), False, CHUNK)
    cols = api.device_columns({"intensity": inten.data_ptr()})
    count, stats = C.c_uint64(), api._QueryStats()
    ctx = S["ctx"]
    raw_region, raw_filter = rg._struct(), fl._struct()
    st = ctx._lib.swz_dataset_query_filtered(ctx._ctx, os.fsencode(S["dirs"]["BIN"]), C.byref(p), C.byref(raw_region), C.byref(raw_filter), cap,
                                             C.c_void_p(xyz.data_ptr()), C.byref(cols), C.c_void_p(nodes.data_ptr()), C.byref(count),
                                             C.byref(stats))
    torch.cuda.synchronize()
    text = ctx._lib.swz_last_error(ctx._ctx).decode()
    assert st == ERR_BAD_ARG and "capacity" in text and "swz_dataset_query_filtered" in text
    assert count.value == stops
    # nothing at or beyond capacity rows
    assert (xyz.cpu().numpy()[cap * 24:] == POISON).all() and (inten.cpu().numpy()[cap * 2:] == POISON).all()
    assert (nodes.cpu().numpy()[cap * 4:] == POISON).all()
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_filtered(ctx, S["dirs"]["BIN"], UNIT[0], UNIT[1], rg, fl, chunk_points=CHUNK, capacity=cap)
    assert "capacity" in str(e.value)
    assert swz.dataset_query_filtered(ctx, S["dirs"]["BIN"], UNIT[0], UNIT[1], rg, fl, chunk_points=CHUNK, capacity=want)["count"] == want
