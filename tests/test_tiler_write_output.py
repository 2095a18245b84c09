"""swz_tiler_write_output: the node files of a multi-batch tiler, and the format's metadata, written in one call.

The expected directory is built the long way, with the calls a caller had to chain before: export_device, node_table,
pools_device, gather_payload_device, then per node the HOST producers bin_write_node / pnts_write_node_rows /
las_write_node_rows, and tileset_build + tileset_write or ept_hierarchy_write for the metadata.  Those producers are held
against the reference's formats by the existing suites; nothing expected comes from the pack kernels or the streamed writer.
Directories are compared by their sorted listings (so a leftover or a missing file fails) and file by file, byte by byte;
.binz files after bin_read_node, because zlib's output is not pinned.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ERR_BAD_ARG, ERR_TILER_FAILED = 2, 8
COLUMNS = ("rgb", "intensity", "classification", "gps_time")
FORMATS = ("BIN", "BINZ", "3DTILES", "LAS", "ENTWINE_LAS")
GLOBAL_OFFSET = (1000.5, -20.25, 3.0)
CONFIGS = {"min_distance_accurate": ("MIN_DISTANCE", "ACCURATE"), "random_grid_fast": ("RANDOM_GRID", "FAST")}


def _batches():
    """three batches of about 4 000 points; the third is cut out of the middle of the cloud, so it reaches existing files"""
    rng = np.random.default_rng(2718)
    parts = [rng.random((4000, 3)), rng.random((4100, 3)), 0.25 + 0.5 * rng.random((3900, 3))]
    cols = []
    for p in parts:
        n = len(p)
        cols.append({"rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
                     "intensity": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16),
                     "classification": rng.integers(0, 31, n, endpoint=True).astype(np.uint8),
                     "gps_time": rng.random(n) * 1e9})
    return parts, cols


def _params(config):
    import schwarzwald_amd as swz
    sampler, strategy = CONFIGS[config]
    return swz.TileParams(sampler=swz.SAMPLERS[sampler], max_points_per_node=96, spacing_at_root=swz.spacing_from_diagonal(*UNIT, 12),
                          strategy=getattr(swz, strategy), fast_concurrency=2)


def _tile(ctx, config):
    import schwarzwald_amd as swz
    parts, cols = _batches()
    t = swz.Tiler(ctx, UNIT[0], UNIT[1], _params(config))
    for p, c in zip(parts, cols):
        t.add_batch(p, c)
    t.finalize()
    return t


def _rows_the_long_way(ctx, t):
    """(node table, positions and columns of every stored point in file order) through the calls of the parent recipe"""
    import torch
    info = t.info()
    ns = int(info["num_stored"])
    nodes = t.node_table()
    dev = torch.device("cuda:0")
    d_ids = torch.empty(ns, dtype=torch.int32, device=dev)
    t.export_device(None, d_ids.data_ptr(), None)
    pool_xyz, pool_attrs = t.pools_device()
    assert sorted(pool_attrs) == sorted(COLUMNS)
    from schwarzwald_amd.api import ATTRIBUTES
    d_xyz = torch.empty((ns, 3), dtype=torch.float64, device=dev)
    d_out = {a: torch.empty(ns * np.dtype(ATTRIBUTES[a][1]).itemsize * ATTRIBUTES[a][2], dtype=torch.uint8, device=dev) for a in COLUMNS}
    ctx.gather_payload_device(d_ids.data_ptr(), None, ns, pool_xyz, pool_attrs, d_xyz.data_ptr(), {a: v.data_ptr() for a, v in d_out.items()})
    torch.cuda.synchronize()
    xyz = d_xyz.cpu().numpy()
    cols = {}
    for a in COLUMNS:
        _, dt, width = ATTRIBUTES[a]
        arr = d_out[a].cpu().numpy().view(dt)
        cols[a] = arr.reshape(ns, width) if width > 1 else arr
    return info, nodes, xyz, cols


@pytest.fixture(scope="module", params=list(CONFIGS))
def tiled(request):
    import schwarzwald_amd as swz
    with swz.Context(0) as ctx:
        t = _tile(ctx, request.param)
        info, nodes, xyz, cols = _rows_the_long_way(ctx, t)
        counts = nodes["count"].astype(np.int64)
        print("%s: %d points, %d stored, %d nodes of %d..%d points" % (request.param, info["num_points"], info["num_stored"],
                                                                        len(counts), counts.min(), counts.max()))
        assert len(counts) >= 100 and counts.min() >= 1 and counts.max() <= 500
        if CONFIGS[request.param][1] == "FAST":
            assert info["num_stored"] > info["num_points"]  # copies of points in reconstructed ancestors
        yield dict(config=request.param, ctx=ctx, t=t, info=info, nodes=nodes, xyz=xyz, cols=cols)
        t.close()


def _expected(S, directory, fmt, names, rgb_from=0, global_offset=None):
    """the directory write_output must produce, from the host producers"""
    import schwarzwald_amd as swz
    nodes, xyz, cols = S["nodes"], S["xyz"], S["cols"]
    os.makedirs(directory)
    data = directory
    if fmt == "ENTWINE_LAS":
        swz.ept_create_dirs(directory)
        data = os.path.join(directory, "ept-data")
    for k in range(len(nodes["count"])):
        lv, key, o, c = int(nodes["level"][k]), int(nodes["key"][k]), int(nodes["offset"][k]), int(nodes["count"][k])
        rows = slice(o, o + c)
        sub = {a: cols[a][rows] for a in names}
        name = swz.node_name(lv, key)
        if fmt in ("BIN", "BINZ"):
            swz.bin_write_node(os.path.join(data, name + ".bin"), xyz[rows], sub)  # (.binz is compared as rows)
        elif fmt == "3DTILES":
            write = [a for a in ("rgb", "intensity") if a in names]
            if rgb_from and "rgb" not in write:
                write.append("rgb")
            swz.pnts_write_node_rows(os.path.join(data, name + ".pnts"), xyz[rows], sub, write=write, rgb_from=rgb_from,
                                     rtc_center=global_offset)
        else:
            mn, mx = swz.node_bounds(lv, key, *UNIT)
            if fmt == "ENTWINE_LAS":
                name = swz.node_name_entwine(lv, key)
            swz.las_write_node_rows(os.path.join(data, name + ".las"), xyz[rows], sub, mn, mx, swz.las_scale_from_bounds(mn, mx),
                                    write=list(names))
    if fmt == "3DTILES":
        swz.tileset_write(swz.tileset_build(nodes["level"], nodes["key"], *UNIT, _params(S["config"]).spacing_at_root, global_offset),
                          directory)
    if fmt == "ENTWINE_LAS":
        swz.ept_hierarchy_write(directory, nodes)


def _listing(directory):
    out = []
    for dirpath, dirs, files in os.walk(directory):
        rel = os.path.relpath(dirpath, directory)
        out += [os.path.normpath(os.path.join(rel, d)) + "/" for d in dirs]
        out += [os.path.normpath(os.path.join(rel, f)) for f in files]
    return sorted(out)


def _assert_same(got_dir, want_dir, fmt):
    import schwarzwald_amd as swz
    got, want = _listing(got_dir), _listing(want_dir)
    if fmt == "BINZ":
        want = sorted(w + "z" if w.endswith(".bin") else w for w in want)
    assert got == want
    assert len([g for g in got if not g.endswith("/")]) >= 100
    for rel in got:
        if rel.endswith("/"):
            continue
        if fmt == "BINZ":
            gx, gc = swz.bin_read_node(os.path.join(got_dir, rel), True)
            wx, wc = swz.bin_read_node(os.path.join(want_dir, rel[:-1]), False)
            assert np.array_equal(gx, wx) and sorted(gc) == sorted(wc), rel
            for a in wc:
                assert np.array_equal(gc[a], wc[a]), (rel, a)
        else:
            assert open(os.path.join(got_dir, rel), "rb").read() == open(os.path.join(want_dir, rel), "rb").read(), rel


def _check(S, tmp_path, fmt, names=COLUMNS, t=None, **kw):
    want_dir, got_dir = str(tmp_path / "want"), str(tmp_path / "got")
    extra = dict(global_offset=GLOBAL_OFFSET) if fmt == "3DTILES" else {}
    _expected(S, want_dir, fmt, names, kw.get("rgb_from", 0), extra.get("global_offset"))
    stats = (t or S["t"]).write_output(got_dir, fmt, attrs=names, **extra, **kw)
    print(fmt, stats)
    _assert_same(got_dir, want_dir, fmt)
    assert stats["nodes"] == len(S["nodes"]["count"]) and stats["stored_points"] == S["info"]["num_stored"]
    assert stats["bytes_written"] > 0 and stats["wall_ms"] > 0
    return stats


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_with_the_default_chunk(tiled, tmp_path, fmt):
    stats = _check(tiled, tmp_path, fmt)
    assert stats["chunks"] == 1


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_in_chunks_capped_by_the_largest_node(tiled, tmp_path, fmt):
    import schwarzwald_amd as swz
    stats = _check(tiled, tmp_path, fmt, chunk_points=1)
    assert stats["chunks"] >= 5
    assert stats["chunks"] == len(swz.output_chunks(tiled["nodes"]["count"], 1)) - 1


def test_a_chunk_that_ends_exactly_behind_the_root(tiled, tmp_path):
    import schwarzwald_amd as swz
    counts = tiled["nodes"]["count"]
    assert int(tiled["nodes"]["level"][0]) == -1
    root = int(counts[0])
    first = swz.output_chunks(counts, root)
    assert int(first[1]) == 1, "the root (%d points, largest node %d) is not a chunk of its own" % (root, counts.max())
    stats = _check(tiled, tmp_path, "LAS", chunk_points=root)
    assert stats["chunks"] == len(first) - 1 >= 2


def test_rgb_from_intensity_log_without_a_colour_column(tiled, tmp_path):
    _check(tiled, tmp_path, "3DTILES", names=("intensity",), rgb_from=2, chunk_points=700)


@pytest.mark.parametrize("fmt,names", [("BIN", ("rgb",)), ("LAS", ("intensity", "gps_time")), ("3DTILES", ("rgb",)),
                                       ("BINZ", ()), ("ENTWINE_LAS", ("classification",))])
def test_a_mask_that_is_a_strict_subset_of_the_columns(tiled, tmp_path, fmt, names):
    _check(tiled, tmp_path, fmt, names=names, chunk_points=1000)


def test_spilled_pools_are_read_in_place(tiled, tmp_path):
    import schwarzwald_amd as swz
    with swz.Context(0) as ctx:
        ctx.set_option("SWZ_TILER_SPILL", "host")
        t = _tile(ctx, tiled["config"])
        try:
            dev, host = t.pool_residency()
            assert host > 0 and dev == 0
            _check(tiled, tmp_path, "LAS", t=t, chunk_points=500)
        finally:
            t.close()


def test_entwine_with_ept_json(tiled, tmp_path):
    import schwarzwald_amd as swz
    ept = dict(bounds=UNIT, conforming_bounds=([0.01, 0.02, 0.03], [0.9, 0.8, 0.7]), points=int(tiled["info"]["num_points"]),
               attrs=COLUMNS, span=128.0, srs=dict(authority="EPSG", horizontal="25832", wkt="w\"kt"), version="1.0.0")
    want_dir = str(tmp_path / "want")
    _expected(tiled, want_dir, "ENTWINE_LAS", COLUMNS)
    swz.ept_json_write(os.path.join(want_dir, "ept.json"), **ept)
    tiled["t"].write_output(str(tmp_path / "got"), "ENTWINE_LAS", attrs=COLUMNS, ept=ept, chunk_points=2000)
    _assert_same(str(tmp_path / "got"), want_dir, "ENTWINE_LAS")


def test_refusals_leave_the_directory_empty_and_the_tiler_usable(tiled, tmp_path):
    import schwarzwald_amd as swz
    t = tiled["t"]
    out = tmp_path / "out"
    out.mkdir()
    refused = [
        dict(format="LAS", attrs=("rgb", "normal")),                  # a column never staged
        dict(format="BIN", attrs=1 << 12),                             # a bit that does not exist
        dict(format=7, attrs=()),                                      # an unknown format
        dict(format="3DTILES", attrs=("rgb",), rgb_from=1),            # a mapping without intensities
        dict(format="3DTILES", attrs=("rgb",), global_offset=(0.0, float("nan"), 0.0)),
    ]
    for kw in refused:
        with pytest.raises(swz.SwzError) as e:
            t.write_output(str(out), **kw)
        assert e.value.code == ERR_BAD_ARG, kw
        assert os.listdir(str(out)) == [], kw
    # a directory that cannot be created: its parent is a file
    (tmp_path / "file").write_bytes(b"x")
    for fmt in ("BIN", "ENTWINE_LAS"):
        with pytest.raises(swz.SwzError) as e:
            t.write_output(str(tmp_path / "file" / "sub"), fmt, attrs=COLUMNS)
        assert e.value.code == ERR_BAD_ARG
    assert sorted(os.listdir(str(tmp_path))) == ["file", "out"]
    # a file that cannot be written: the name of one node's file is taken by a directory
    name = swz.node_name(int(tiled["nodes"]["level"][3]), int(tiled["nodes"]["key"][3]))
    blocked = tmp_path / "blocked"
    (blocked / (name + ".bin")).mkdir(parents=True)
    with pytest.raises(swz.SwzError) as e:
        t.write_output(str(blocked), "BIN", attrs=COLUMNS)
    assert name + ".bin" in str(e.value)
    # none of this poisons the tiler: it writes the same files twice
    assert t.info()["num_stored"] == tiled["info"]["num_stored"]
    _check(tiled, tmp_path / "a", "BIN")
    t.write_output(str(tmp_path / "again"), "BIN", attrs=COLUMNS)
    _assert_same(str(tmp_path / "again"), str(tmp_path / "a" / "want"), "BIN")


def test_a_poisoned_tiler_is_refused(tmp_path):
    import schwarzwald_amd as swz
    out = tmp_path / "out"
    out.mkdir()
    with swz.Context(0) as ctx:
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=100, spacing_at_root=swz.spacing_from_diagonal(*UNIT, 12))
        with swz.Tiler(ctx, UNIT[0], UNIT[1], params) as t:
            t.add_batch(np.random.default_rng(1).random((500, 3)))
            t.finalize()
            t.poison("test")
            with pytest.raises(swz.SwzError) as e:
                t.write_output(str(out), "BIN")
            assert e.value.code == ERR_TILER_FAILED
    assert os.listdir(str(out)) == []
