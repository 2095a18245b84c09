"""swz_convert_dataset_world: a written data set converted to georeferenced 3D Tiles -- positions in ECEF, every .pnts file
relative to its node's own origin, tile volumes as oriented boxes.

The yardsticks are existing code: a node file must be, byte for byte, pnts_write_node_rows(proj - m, rtc_center=m) with proj
= srs_transform_device of the source file's rows and m its per-axis minimum; the boxes are tileset_oriented_boxes of
tileset_build of the scanned table, compared with ==.  Accuracy is checked against the mpmath reference of srs_ref.py:
|rtc + float - reference| <= the node's ECEF extent x 2^-24 (half an ulp of float of the largest offset from the origin, per
axis) + TOL_M of test_srs_gpu.py (the projection's existing bound)."""
import json
import os

import numpy as np
import pytest

import srs_ref as R

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
TOL_M = 1e-6
UTM32 = R.utm_definition(32, False)
ROOT = ([500000.0, 5400000.0, 200.0], [500400.0, 5400400.0, 600.0])
NAMES = ("rgb", "intensity")
CHUNK = 1500
PROPS = "properties.json"


def _cloud():
    """4 500 points of millimetre-quantised UTM 32N coordinates: a tilted sheet of terrain and a stack of one point 30 times"""
    rng = np.random.default_rng(2718)
    n = 4500
    xy = rng.random((n, 2)) * 400.0
    z = 40.0 + 0.2 * xy[:, 0] + 0.05 * xy[:, 1] + rng.random(n) * 3.0
    xyz = np.array(ROOT[0]) + np.round(np.column_stack([xy, z]), 3)
    xyz[4470:] = xyz[4470]
    cols = {"rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
            "intensity": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)}
    return xyz, cols


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    import torch
    import schwarzwald_amd as swz
    root = tmp_path_factory.mktemp("world")
    with swz.Context(0) as ctx:
        spacing = swz.spacing_from_diagonal(*ROOT, 16)
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=64, spacing_at_root=spacing)
        xyz, cols = _cloud()
        with swz.Tiler(ctx, ROOT[0], ROOT[1], params) as t:
            t.add_batch(xyz, cols)
            t.finalize()
            nodes = t.node_table()
            assert int(nodes["level"].max()) >= 1                                     # three levels: r, r?, r??
            assert len(swz.output_chunks(nodes["count"], CHUNK)) - 1 >= 3
            src = {}
            for fmt in ("BIN", "LAS"):
                src[fmt] = str(root / ("src_" + fmt))
                t.write_output(src[fmt], fmt, attrs=NAMES)
                t.write_properties(src[fmt])
        yield dict(ctx=ctx, src=src, nodes=nodes, spacing=spacing, root=root)


def _project(ctx, srs, rows):
    import torch
    if srs is None:
        return rows.copy()
    t = torch.from_numpy(np.ascontiguousarray(rows)).to("cuda:0")
    ctx.srs_transform_device(srs, t)
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _read_source(directory, fmt, name):
    import schwarzwald_amd as swz
    if fmt == "BIN":
        return swz.bin_read_node(os.path.join(directory, name + ".bin"))
    return swz.las_read_node(os.path.join(directory, name + ".las"))


def _walk(tile, out):
    out.setdefault(tile["content"]["uri"].rsplit(".", 1)[0], tile["boundingVolume"]["box"])
    for child in tile.get("children", []):
        _walk(child, out)


def _boxes(directory):
    """node name -> boundingVolume.box, from every tileset JSON of the directory (a file's root repeats its parent's entry)"""
    out = {}
    for f in sorted(os.listdir(directory)):
        if f.endswith(".json") and f != PROPS:
            doc = json.load(open(os.path.join(directory, f)))
            seen = {}
            _walk(doc["root"], seen)
            for name, box in seen.items():
                assert out.setdefault(name, box) == box
    return out


def _check_directory(S, out, fmt, srs, want_dir):
    """files, bytes and boxes of a world conversion of S's source `fmt`"""
    import schwarzwald_amd as swz
    scan = swz.dataset_scan(S["src"][fmt])
    table = scan["nodes"]
    names = [swz.node_name(int(l), int(k)) for l, k in zip(table["level"], table["key"])]
    os.mkdir(want_dir)
    for name in names:
        rows, cols = _read_source(S["src"][fmt], fmt, name)
        proj = _project(S["ctx"], srs, rows)
        m = proj.min(axis=0)
        swz.pnts_write_node_rows(os.path.join(want_dir, name + ".pnts"), proj - m, cols, write=list(NAMES), rtc_center=m)
        got = open(os.path.join(out, name + ".pnts"), "rb").read()
        assert got == open(os.path.join(want_dir, name + ".pnts"), "rb").read(), name
    tiles = swz.tileset_build(table["level"], table["key"], scan["root_min"], scan["root_max"], scan["spacing_at_root"])
    swz.tileset_write(tiles, want_dir)                                               # (for the names of the JSON files)
    assert sorted(os.listdir(out)) == sorted(os.listdir(want_dir) + [PROPS])
    obb = swz.tileset_oriented_boxes(srs, tiles)
    boxes = _boxes(out)
    assert len(boxes) == len(tiles)
    for t, row in zip(tiles, obb):
        assert boxes[swz.node_name(t["level"], t["key"])] == list(row), (t["level"], t["key"])
    props = swz.properties_json_read(out)
    assert props["root_min"].tolist() == ROOT[0] and props["root_max"].tolist() == ROOT[1]
    assert np.float32(props["spacing_at_root"]) == np.float32(S["spacing"]) and props["processed_points"] == int(table["count"].sum())
    return names


@pytest.mark.parametrize("fmt", ["BIN", "LAS"])
@pytest.mark.parametrize("srs", [UTM32, None])
def test_files_and_boxes(S, tmp_path, fmt, srs):
    import schwarzwald_amd as swz
    out = str(tmp_path / "out")
    stats = swz.convert_dataset_world(S["ctx"], S["src"][fmt], out, srs, attrs=NAMES, chunk_points=CHUNK)
    print(fmt, srs, stats)
    names = _check_directory(S, out, fmt, srs, str(tmp_path / "want"))
    assert stats["chunks"] >= 3 and stats["nodes"] == len(names) > 20 and stats["points"] == int(S["nodes"]["count"].sum())
    if srs is not None:
        rtc = swz.pnts_read_node(os.path.join(out, "r.pnts"))[2]
        assert 6.3e6 < np.linalg.norm(rtc) < 6.4e6


def test_an_srs_object_and_one_chunk_give_the_same_directory(S, tmp_path):
    import schwarzwald_amd as swz
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    swz.convert_dataset_world(S["ctx"], S["src"]["BIN"], a, UTM32, attrs=NAMES, chunk_points=CHUNK)
    stats = S["ctx"].convert_dataset_world(S["src"]["BIN"], b, swz.Srs(UTM32), attrs=NAMES)
    assert stats["chunks"] == 1 and sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in os.listdir(a):
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.mark.parametrize("srs", [UTM32, None])
def test_tight_bounds_enclose_the_points(S, tmp_path, srs):
    import schwarzwald_amd as swz
    out = str(tmp_path / "out")
    swz.convert_dataset_world(S["ctx"], S["src"]["BIN"], out, srs, attrs=NAMES, chunk_points=CHUNK, tight_bounds=True)
    table = S["nodes"]
    tiles = swz.tileset_build(table["level"], table["key"], *ROOT, S["spacing"])
    boxes = _boxes(out)
    name_of = [swz.node_name(t["level"], t["key"]) for t in tiles]
    checked = 0
    for i, t in enumerate(tiles):
        if not t["has_content"]:
            continue
        xyz, _, rtc = swz.pnts_read_node(os.path.join(out, name_of[i] + ".pnts"))
        pts = np.array(rtc) + xyz
        j = i
        while j >= 0:                                                                # its own tile, then every ancestor
            box = np.array(boxes[name_of[j]])
            assert (box[3:].reshape(3, 3) == np.diag(np.diag(box[3:].reshape(3, 3)))).all()   # axis-aligned: half-axes
            centre, half = box[:3], np.diag(box[3:].reshape(3, 3))
            assert (pts >= centre - half).all() and (pts <= centre + half).all(), (name_of[i], name_of[j])
            j = tiles[j]["parent"]
            checked += 1
    assert checked > 3 * 20
    # the node files are those without the flag
    plain = str(tmp_path / "plain")
    swz.convert_dataset_world(S["ctx"], S["src"]["BIN"], plain, srs, attrs=NAMES, chunk_points=CHUNK)
    for f in os.listdir(plain):
        if f.endswith(".pnts"):
            assert open(os.path.join(out, f), "rb").read() == open(os.path.join(plain, f), "rb").read(), f
    assert _boxes(plain) != boxes


def test_max_depth_zero_writes_the_root_alone(S, tmp_path):
    import schwarzwald_amd as swz
    out = str(tmp_path / "out")
    stats = swz.convert_dataset_world(S["ctx"], S["src"]["BIN"], out, UTM32, attrs=NAMES, max_depth=0)
    assert sorted(os.listdir(out)) == [PROPS, "r.json", "r.pnts"] and stats["nodes"] == 1
    rows, cols = swz.bin_read_node(os.path.join(S["src"]["BIN"], "r.bin"))
    proj = _project(S["ctx"], UTM32, rows)
    want = str(tmp_path / "want.pnts")
    swz.pnts_write_node_rows(want, proj - proj.min(axis=0), cols, write=list(NAMES), rtc_center=proj.min(axis=0))
    assert open(os.path.join(out, "r.pnts"), "rb").read() == open(want, "rb").read()


def test_accuracy_against_the_reference(S, tmp_path):
    """one UTM group of srs_ref.py as a one-node data set: point for point against its high/low ECEF reference"""
    import schwarzwald_amd as swz
    g = next(x for x in R.points() if x["definition"] == UTM32)
    xyz = g["xyz"]
    n = len(xyz)
    rng = np.random.default_rng(1)
    cols = {"rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8), "intensity": np.arange(n, dtype=np.uint16)}
    src, out = str(tmp_path / "src"), str(tmp_path / "out")
    os.mkdir(src)
    swz.bin_write_node(os.path.join(src, "r.bin"), xyz, cols)
    lo = xyz.min(axis=0)
    side = float((xyz.max(axis=0) - lo).max())
    swz.properties_json_write(src, lo, lo + side, side / 100, n)
    swz.convert_dataset_world(S["ctx"], src, out, UTM32, attrs=NAMES)
    got, got_cols, rtc = swz.pnts_read_node(os.path.join(out, "r.pnts"))
    assert np.array_equal(got_cols["intensity"], cols["intensity"])                  # the rows are in the file's order
    ref = g["ecef_hi"] + g["ecef_lo"]
    extent = ref.max(axis=0) - ref.min(axis=0)
    err = R.errors(np.array(rtc) + got, g["ecef_hi"], g["ecef_lo"])
    print("world conversion: max |error| per axis %s m, bound %s m" % (err.max(axis=0), extent * 2.0 ** -24 + TOL_M))
    assert (err <= extent * 2.0 ** -24 + TOL_M).all()
    assert np.abs(np.array(rtc) - ref.min(axis=0)).max() <= TOL_M


def _snapshot(directory):
    return {f: open(os.path.join(directory, f), "rb").read() for f in sorted(os.listdir(directory))}


def test_refusals_leave_dst_empty(S, tmp_path):
    import schwarzwald_amd as swz
    src, out = S["src"]["BIN"], str(tmp_path / "out")
    before = _snapshot(src)
    for dst, word, kw in ((out, "only 3DTILES", dict(format="LAS")), (out, "global_offset must be 0", dict(global_offset=(0.0, 1.0, 0.0))),
                          (src, "dst_dir is src_dir", {}), (out, "the source does not hold", dict(attrs=("rgb", "normal"))),
                          (out, "unknown flag bit", dict(flags=2))):
        with pytest.raises(swz.SwzError) as e:
            swz.convert_dataset_world(S["ctx"], src, dst, UTM32, **kw)
        assert e.value.code == ERR_BAD_ARG and word in str(e.value) and "swz_convert_dataset_world" in str(e.value), str(e.value)
        assert not os.path.exists(out) or os.listdir(out) == []
    with pytest.raises(swz.SwzError) as e:
        swz.convert_dataset_world(S["ctx"], src, out, "+proj=merc +datum=WGS84")
    assert "+proj=merc" in str(e.value) and not os.path.exists(out)
    assert _snapshot(src) == before
