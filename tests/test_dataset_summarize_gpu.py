"""swz_dataset_summarize and what swz_dataset_query_filtered does with its sidecar, on small data sets in all five formats.

The sidecar is tests/summary_ref.py over every node file read back with the host readers.  A filtered query returns the same
bytes before and after the sidecar is written and reads fewer nodes afterwards: those swz_dataset_query_filtered_nodes flags.
A filter every node passes reads what it read before.  A node file replaced by one with another count makes the sidecar stale.
The region and box queries never look at it."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import filter_ref as F
import region_ref as R
import summary_ref as S

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ERR_BAD_ARG = 2
COLUMNS = ("rgb",) + F.SCALARS
FORMATS = ("BIN", "BINZ", "LAS", "ENTWINE_LAS", "3DTILES")
WRITTEN = {fmt: COLUMNS for fmt in FORMATS[:4]}
WRITTEN["3DTILES"] = ("rgb", "intensity")
CHUNK = 500
BIG_L = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.25], [0.25, 0.25], [0.25, 1.0], [0.0, 1.0]])
# narrow filters: one flight strip, one class below a height, one time window; the columns follow the positions
NARROW = {"strip": [("range", "point_source_id", 1, 1)], "ground": [("any_of", "classification", [2]), ("range", "gps_time", 0, 3e4)],
          "not_range": [("not_range", "intensity", 5000, 65535), ("none_of", "classification", [7])]}
NARROW_LOSSY = [("range", "intensity", 0, 9000)]           # all a .pnts file carries beside RGB
EVERY_NODE = [("range", "intensity", 0, 65535)]


def _cloud():
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


def _node_file(swz, directory, fmt, level, key):
    if fmt == "ENTWINE_LAS":
        return os.path.join(directory, "ept-data", swz.node_name_entwine(level, key) + ".las")
    return os.path.join(directory, swz.node_name(level, key) + {"BIN": ".bin", "BINZ": ".binz", "LAS": ".las", "3DTILES": ".pnts"}[fmt])


def _read_all(swz, directory, fmt):
    """every node file in scan order with the host readers: the columns, and the node table over their rows"""
    scan = swz.dataset_scan(directory)
    cols, count = {}, []
    for level, key in zip(scan["nodes"]["level"], scan["nodes"]["key"]):
        path = _node_file(swz, directory, fmt, int(level), int(key))
        got = swz.bin_read_node(path, fmt == "BINZ") if fmt in ("BIN", "BINZ") else swz.pnts_read_node(path) if fmt == "3DTILES" \
            else swz.las_read_node(path)
        for name, v in got[1].items():
            cols.setdefault(name, []).append(v)
        count.append(len(got[0]))
    count = np.array(count, dtype=np.uint64)
    return dict(scan=scan, cols={k: np.concatenate(v) for k, v in cols.items()}, count=count,
                offset=np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.uint64))


@pytest.fixture(scope="module")
def D(tmp_path_factory):
    import schwarzwald_amd as swz
    root = tmp_path_factory.mktemp("summarize")
    with swz.Context(0) as ctx:
        spacing = swz.spacing_from_diagonal(*UNIT, 12)
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=150, spacing_at_root=spacing)
        xyz, cols = _cloud()
        with swz.Tiler(ctx, UNIT[0], UNIT[1], params) as t:
            t.add_batch(xyz, cols)
            t.finalize()
            info = t.info()
            dirs = {}
            for fmt in FORMATS + ("NO_SCALARS",):
                dirs[fmt] = str(root / fmt)
                attrs = WRITTEN.get(fmt, ("rgb",))                                 # NO_SCALARS: a BIN data set of positions and colours
                extra = dict(ept=dict(bounds=UNIT, conforming_bounds=UNIT, points=int(info["num_points"]), attrs=attrs, span=128.0,
                                      srs=dict(authority="EPSG", horizontal="25832", wkt="wkt"), version="1.0.0")) if fmt == "ENTWINE_LAS" else {}
                t.write_output(dirs[fmt], "BIN" if fmt == "NO_SCALARS" else fmt, attrs=attrs, **extra)
                if fmt != "ENTWINE_LAS":
                    t.write_properties(dirs[fmt])
        yield dict(ctx=ctx, dirs=dirs, root=root)


def _same_outputs(a, b, names):
    assert a["count"] == b["count"]
    for k in ("xyz", "node") + tuple(names):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def _count_only(swz, ctx, directory, region, filter, lossy):
    from schwarzwald_amd import api
    p = api._query_params(UNIT[0], UNIT[1], None, (), lossy, CHUNK)
    rg, fl = (None if region is None else region._struct()), filter._struct()
    count, stats = C.c_uint64(), api._QueryStats()
    ctx._check(ctx._lib.swz_dataset_query_filtered(ctx._ctx, os.fsencode(directory), C.byref(p), None if rg is None else C.byref(rg), C.byref(fl), 0, None,
                                                   None, None, C.byref(count), C.byref(stats)))
    return int(count.value), stats


@pytest.mark.parametrize("fmt", FORMATS)
def test_summarize_then_query(D, fmt):
    import schwarzwald_amd as swz
    ctx, directory, lossy = D["ctx"], D["dirs"][fmt], fmt == "3DTILES"
    names = list(WRITTEN[fmt])
    scalars = [k for k in names if k != "rgb"]
    filters = {"lossy": NARROW_LOSSY} if lossy else NARROW
    regions = {"strip": None, "lossy": None, "ground": R.as_region(swz, ("polygon", BIG_L)), "not_range": R.as_region(swz, ("planes", [[-1.0, -1.0, 0.0, 1.2]]))}
    query = lambda which, filter: swz.dataset_query_filtered(ctx, directory, UNIT[0], UNIT[1], regions[which], F.as_filter(swz, filter), lossy_source=lossy,  # noqa: E731
                                                             chunk_points=CHUNK, return_nodes=True)
    assert swz.dataset_summaries_read(directory) is None
    before = {which: query(which, f) for which, f in filters.items()}
    before_all = query("strip" if not lossy else "lossy", EVERY_NODE)
    plain_region = swz.dataset_query_region(ctx, directory, UNIT[0], UNIT[1], regions["ground"], lossy_source=lossy, chunk_points=CHUNK, return_nodes=True)
    plain_box = swz.dataset_query(ctx, directory, UNIT[0], UNIT[1], lossy_source=lossy, chunk_points=CHUNK, return_nodes=True)

    stats = ctx.dataset_summarize(directory, lossy_source=lossy, chunk_points=CHUNK)
    T = _read_all(swz, directory, fmt)
    scan = T["scan"]
    assert stats["nodes"] == len(T["count"]) >= 20 and stats["points"] == int(T["count"].sum()) == scan["points"] and stats["chunks"] >= 8
    assert stats["bytes_read"] > 0

    # the sidecar is the reference over the files read back
    side = swz.dataset_summaries_read(directory)
    assert side["format"] == fmt and side["attrs"] == S.ordered(scalars) and side["points"] == scan["points"]
    for k in ("level", "key", "count"):
        assert np.array_equal(side["nodes"][k], scan["nodes"][k])
    want = S.summaries(T["cols"], scalars, T["offset"], T["count"])
    for k in range(len(T["count"])):
        assert S.same(side["entries"][k], want[k]), (k, side["entries"][k], want[k])
    after_scan = swz.dataset_scan(directory)
    assert after_scan["points"] == scan["points"] and np.array_equal(after_scan["nodes"]["key"], scan["nodes"]["key"])

    # the same bytes, fewer nodes
    for which, filter in filters.items():
        flags = swz.dataset_query_filtered_nodes(directory, UNIT[0], UNIT[1], regions[which], F.as_filter(swz, filter), lossy_source=lossy)
        table = swz.dataset_query_region_nodes(directory, UNIT[0], UNIT[1], regions[which], lossy_source=lossy)
        assert np.array_equal(flags["key"], table["key"]) and np.array_equal(flags["level"], table["level"])
        index = {(int(l), int(k)): i for i, (l, k) in enumerate(zip(scan["nodes"]["level"], scan["nodes"]["key"]))}
        at = np.array([index[(int(l), int(k))] for l, k in zip(table["level"], table["key"])])
        assert np.array_equal(flags["read"], S.reads(want, scalars, filter)[at]), which
        after = query(which, filter)
        assert after["count"] > 0
        _same_outputs(before[which], after, names)
        b, a = before[which]["stats"], after["stats"]
        assert a["nodes_read"] == int(flags["read"].sum()) < b["nodes_read"] == len(table["key"]), which
        assert a["points_read"] == flags["points_bound"] < b["points_read"] and a["bytes_read"] < b["bytes_read"] and a["chunks"] <= b["chunks"]
        assert a["points_out"] == b["points_out"] and a["nodes_scanned"] == b["nodes_scanned"]
        count, st = _count_only(swz, ctx, directory, regions[which], F.as_filter(swz, filter), lossy)
        assert count == after["count"] and st.nodes_read == a["nodes_read"] and st.points_read == a["points_read"]

    # a filter every node passes reads what it read without the sidecar
    after_all = query("strip" if not lossy else "lossy", EVERY_NODE)
    _same_outputs(before_all, after_all, names)
    for k in ("nodes_read", "points_read", "bytes_read", "chunks", "points_out"):
        assert after_all["stats"][k] == before_all["stats"][k], k

    # the region and box queries ignore the sidecar
    again = swz.dataset_query_region(ctx, directory, UNIT[0], UNIT[1], regions["ground"], lossy_source=lossy, chunk_points=CHUNK, return_nodes=True)
    _same_outputs(plain_region, again, names)
    assert again["stats"]["nodes_read"] == plain_region["stats"]["nodes_read"] and again["stats"]["bytes_read"] == plain_region["stats"]["bytes_read"]
    again = swz.dataset_query(ctx, directory, UNIT[0], UNIT[1], lossy_source=lossy, chunk_points=CHUNK, return_nodes=True)
    _same_outputs(plain_box, again, names)
    assert again["stats"]["nodes_read"] == plain_box["stats"]["nodes_read"] == len(T["count"])


def test_a_replaced_node_file_makes_the_sidecar_stale(D):
    import schwarzwald_amd as swz
    ctx = D["ctx"]
    directory = str(D["root"] / "stale")
    shutil.copytree(D["dirs"]["BIN"], directory)
    if swz.dataset_summaries_read(directory) is None:
        ctx.dataset_summarize(directory, chunk_points=CHUNK)
    scan = swz.dataset_scan(directory)
    k = len(scan["nodes"]["key"]) // 2
    name = swz.node_name(int(scan["nodes"]["level"][k]), int(scan["nodes"]["key"][k]))
    path = os.path.join(directory, name + ".bin")
    xyz, cols = swz.bin_read_node(path)
    had = len(xyz)
    assert had > 3
    swz.bin_write_node(path, xyz[:-3], {n: v[:-3] for n, v in cols.items()})
    filter = swz.Filter().range("point_source_id", 1, 1)
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_filtered(ctx, directory, UNIT[0], UNIT[1], None, filter, chunk_points=CHUNK)
    text = str(e.value)
    assert e.value.code == ERR_BAD_ARG and "swz_dataset_query_filtered: node-summaries.swz is stale: node %s holds %d points, the summary %d" % (
        name, had - 3, had) in text and "run swz_dataset_summarize again" in text, text
    # the queries without a filter go on; summarising again mends it
    assert swz.dataset_query(ctx, directory, UNIT[0], UNIT[1], chunk_points=CHUNK)["count"] == scan["points"] - 3
    ctx.dataset_summarize(directory, chunk_points=CHUNK)
    assert swz.dataset_query_filtered(ctx, directory, UNIT[0], UNIT[1], None, filter, chunk_points=CHUNK)["count"] > 0


def test_a_source_without_scalar_columns_gets_an_empty_sidecar(D):
    import schwarzwald_amd as swz
    ctx, directory = D["ctx"], D["dirs"]["NO_SCALARS"]
    stats = ctx.dataset_summarize(directory)
    side = swz.dataset_summaries_read(directory)
    scan = swz.dataset_scan(directory)
    assert side["attribute_mask"] == 0 and side["entries"].shape == (len(scan["nodes"]["key"]), 0) and stats["nodes"] == len(scan["nodes"]["key"])
    assert np.array_equal(side["nodes"]["count"], scan["nodes"]["count"])


def test_what_summarize_refuses(D):
    import schwarzwald_amd as swz
    ctx = D["ctx"]
    for directory, kwargs, words in ((D["dirs"]["3DTILES"], {}, "a 3DTILES source is converted only with"), (D["dirs"]["BIN"], dict(source_flags=2), "an unknown bit in source_flags"),
                                     (str(D["root"] / "nowhere"), {}, "cannot read the directory")):
        with pytest.raises(swz.SwzError) as e:
            ctx.dataset_summarize(directory, **kwargs)
        assert e.value.code == ERR_BAD_ARG and "swz_dataset_summarize" in str(e.value) and words in str(e.value), str(e.value)
