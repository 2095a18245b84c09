"""swz_convert_dataset / swz_convert_dataset_world with a 3DTILES source (lossy_source=True): .pnts node files unpacked
on the device.

The yardsticks are byte identity and existing host code: 3DTILES -> 3DTILES must reproduce the source ((float)(double)f == f);
every other target file must be what the host writer of that format makes of pnts_read_node of the source file; the world
conversion must give, file for file, what it gives for a BIN source built on the host from the same pnts_read_node rows.  No
tolerance anywhere."""
import os
import shutil

import numpy as np
import pytest

import srs_ref as R

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
UTM32 = R.utm_definition(32, False)
ROOT = ([500000.0, 5400000.0, 200.0], [500400.0, 5400400.0, 600.0])
NAMES = ("rgb", "intensity")
GLOBAL_OFFSET = (1000.5, -20.25, 3.0)
CHUNK = 5000
PROPS = "properties.json"


def _cloud():
    """20 000 points in UTM 32N coordinates: a tilted sheet of terrain and a stack of one point 30 times"""
    rng = np.random.default_rng(1618)
    n = 20000
    xy = rng.random((n, 2)) * 400.0
    z = 40.0 + 0.2 * xy[:, 0] + 0.05 * xy[:, 1] + rng.random(n) * 3.0
    xyz = np.array(ROOT[0]) + np.round(np.column_stack([xy, z]), 3)
    xyz[n - 30:] = xyz[n - 30]
    cols = {"rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
            "intensity": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)}
    return xyz, cols


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    import schwarzwald_amd as swz
    root = tmp_path_factory.mktemp("convert_pnts")
    with swz.Context(0) as ctx:
        spacing = swz.spacing_from_diagonal(*ROOT, 16)
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=96, spacing_at_root=spacing)
        xyz, cols = _cloud()
        src = str(root / "src")
        with swz.Tiler(ctx, ROOT[0], ROOT[1], params) as t:
            t.add_batch(xyz, cols)
            t.finalize()
            t.write_output(src, "3DTILES", attrs=NAMES, global_offset=GLOBAL_OFFSET)
            t.write_properties(src)
        scan = swz.dataset_scan(src)
        nodes = scan["nodes"]
        assert scan["format"] == "3DTILES" and scan["attrs"] == list(NAMES) and scan["points"] >= 20000
        assert int(nodes["level"].max()) >= 1 and len(nodes["count"]) >= 50          # three levels or more: r, r?, r??
        assert len(swz.output_chunks(nodes["count"], CHUNK)) - 1 >= 3 and (nodes["count"] % 2 == 1).any()
        names = [swz.node_name(int(l), int(k)) for l, k in zip(nodes["level"], nodes["key"])]
        rows = {name: swz.pnts_read_node(os.path.join(src, name + ".pnts")) for name in names}   # read once, shared, never changed
        assert all(r[2] == list(GLOBAL_OFFSET) for r in rows.values())
        yield dict(ctx=ctx, src=src, scan=scan, nodes=nodes, names=names, rows=rows, spacing=spacing, root=root)


def _listing(directory, without=()):
    out = []
    for dirpath, dirs, files in os.walk(directory):
        rel = os.path.relpath(dirpath, directory)
        out += [os.path.normpath(os.path.join(rel, d)) + "/" for d in dirs]
        out += [os.path.normpath(os.path.join(rel, f)) for f in files]
    return sorted(o for o in out if o not in without)


def _snapshot(directory, without=()):
    return {rel: open(os.path.join(directory, rel), "rb").read() for rel in _listing(directory, without) if not rel.endswith("/")}


def _assert_same(got_dir, want_dir, min_files=50):
    got, want = _snapshot(got_dir, (PROPS,)), _snapshot(want_dir, (PROPS,))
    assert sorted(got) == sorted(want) and len(got) >= min_files
    for rel in got:
        assert got[rel] == want[rel], rel


def _assert_properties(directory, S, points):
    import schwarzwald_amd as swz
    got = swz.properties_json_read(directory)
    assert got["root_min"].tolist() == ROOT[0] and got["root_max"].tolist() == ROOT[1]
    assert np.float32(got["spacing_at_root"]) == np.float32(S["spacing"]) and got["processed_points"] == points


def _kept(S, depth):
    nodes = S["nodes"]
    keep = np.ones(len(nodes["count"]), bool) if depth is None else nodes["level"].astype(np.int64) + 1 <= depth
    return {k: nodes[k][keep] for k in ("level", "key", "count")}, [n for n, k in zip(S["names"], keep) if k]


def _expected(S, directory, fmt, attrs=NAMES, depth=None, global_offset=GLOBAL_OFFSET):
    """the directory the conversion must produce, from pnts_read_node of every source file and the host writers"""
    import schwarzwald_amd as swz
    kept, names = _kept(S, depth)
    os.makedirs(directory)
    data = directory
    if fmt == "ENTWINE_LAS":
        swz.ept_create_dirs(directory)
        data = os.path.join(directory, "ept-data")
    for name, lv, key in zip(names, kept["level"], kept["key"]):
        xyz, cols, _ = S["rows"][name]
        sub = {a: cols[a] for a in attrs}
        if fmt == "BIN":
            swz.bin_write_node(os.path.join(data, name + ".bin"), xyz, sub)
        elif fmt == "3DTILES":
            swz.pnts_write_node_rows(os.path.join(data, name + ".pnts"), xyz, sub, write=list(attrs), rtc_center=global_offset)
        else:
            mn, mx = swz.node_bounds(int(lv), int(key), *ROOT)
            out = swz.node_name_entwine(int(lv), int(key)) if fmt == "ENTWINE_LAS" else name
            swz.las_write_node_rows(os.path.join(data, out + ".las"), xyz, sub, mn, mx, swz.las_scale_from_bounds(mn, mx), write=list(attrs))
    if fmt == "3DTILES":
        swz.tileset_write(swz.tileset_build(kept["level"], kept["key"], *ROOT, S["spacing"], global_offset), directory)
    if fmt == "ENTWINE_LAS":
        swz.ept_hierarchy_write(directory, kept)
    return int(kept["count"].sum()), len(names)


def test_without_the_flag_the_source_is_refused(S, tmp_path):
    import schwarzwald_amd as swz
    out = str(tmp_path / "out")
    before = _snapshot(S["src"])
    for kw in (dict(), dict(lossy_source=False)):
        with pytest.raises(swz.SwzError) as e:
            swz.convert_dataset(S["ctx"], S["src"], out, "BIN", **kw)
        assert e.value.code == ERR_BAD_ARG and "3DTILES source" in str(e.value) and "source_flags" in str(e.value)
    with pytest.raises(swz.SwzError) as e:
        swz.convert_dataset_world(S["ctx"], S["src"], out, UTM32)
    assert "3DTILES source" in str(e.value)
    assert _snapshot(S["src"]) == before and not os.path.exists(out)


def test_3dtiles_to_3dtiles_reproduces_the_source(S, tmp_path):
    import schwarzwald_amd as swz
    out = str(tmp_path / "out")
    stats = swz.convert_dataset(S["ctx"], S["src"], out, "3DTILES", global_offset=GLOBAL_OFFSET, chunk_points=CHUNK, lossy_source=True)
    print(stats)
    _assert_same(out, S["src"])
    _assert_properties(out, S, S["scan"]["points"])
    assert stats["nodes"] == len(S["names"]) and stats["points"] == S["scan"]["points"]
    assert stats["chunks"] == len(swz.output_chunks(S["nodes"]["count"], CHUNK)) - 1 >= 3
    assert stats["bytes_read"] >= sum(os.path.getsize(os.path.join(S["src"], n + ".pnts")) for n in S["names"]) and stats["bytes_written"] > 0


@pytest.mark.parametrize("dst", ["BIN", "LAS", "ENTWINE_LAS"])
def test_every_node_file_is_the_host_writers_of_pnts_read_node(S, tmp_path, dst):
    import schwarzwald_amd as swz
    want, out = str(tmp_path / "want"), str(tmp_path / "out")
    points, _ = _expected(S, want, dst)
    stats = swz.convert_dataset(S["ctx"], S["src"], out, dst, chunk_points=CHUNK, lossy_source=True)   # attrs None: all the source has
    _assert_same(out, want)
    _assert_properties(out, S, points)
    assert stats["points"] == points == S["scan"]["points"] and stats["chunks"] >= 3
    assert swz.dataset_scan(out)["nodes"]["count"].tolist() == S["nodes"]["count"].tolist()


def test_output_does_not_depend_on_chunk_points(S, tmp_path):
    import schwarzwald_amd as swz
    want = str(tmp_path / "want")
    _expected(S, want, "BIN")
    for name, cp in (("one", 0), ("largest", int(S["nodes"]["count"].max()))):
        out = str(tmp_path / name)
        stats = swz.convert_dataset(S["ctx"], S["src"], out, "BIN", chunk_points=cp, lossy_source=True)
        _assert_same(out, want)
        assert (stats["chunks"] == 1) == (cp == 0)


@pytest.mark.parametrize("depth", [0, 1])
def test_max_depth(S, tmp_path, depth):
    import schwarzwald_amd as swz
    for dst in ("3DTILES", "ENTWINE_LAS"):
        want, out = str(tmp_path / ("want_" + dst)), str(tmp_path / ("out_" + dst))
        points, files = _expected(S, want, dst, depth=depth)
        assert files == (1 if depth == 0 else 1 + int((S["nodes"]["level"] == 0).sum())) < len(S["names"])
        stats = swz.convert_dataset(S["ctx"], S["src"], out, dst, max_depth=depth, global_offset=GLOBAL_OFFSET if dst == "3DTILES" else None,
                                    chunk_points=CHUNK, lossy_source=True)
        _assert_same(out, want, min_files=1)
        _assert_properties(out, S, points)
        assert stats["nodes"] == files and stats["points"] == points


def test_attribute_mask_of_rgb_only_drops_the_intensity(S, tmp_path):
    import schwarzwald_amd as swz
    for dst in ("3DTILES", "BIN"):
        want, out = str(tmp_path / ("want_" + dst)), str(tmp_path / ("out_" + dst))
        _expected(S, want, dst, attrs=("rgb",), global_offset=None)
        swz.convert_dataset(S["ctx"], S["src"], out, dst, attrs=("rgb",), chunk_points=CHUNK, lossy_source=True)
        _assert_same(out, want)
    assert sorted(swz.bin_read_node(os.path.join(out, "r.bin"))[1]) == ["rgb"]


def _refused(S, src, dst, word, world=False, **kw):
    import schwarzwald_amd as swz
    before = _snapshot(src)
    with pytest.raises(swz.SwzError) as e:
        if world:
            swz.convert_dataset_world(S["ctx"], src, dst, UTM32, **kw)
        else:
            swz.convert_dataset(S["ctx"], src, dst, "BIN", **kw)
    assert e.value.code == ERR_BAD_ARG and word in str(e.value), str(e.value)
    assert _snapshot(src) == before
    assert not os.path.exists(dst) or os.listdir(dst) == []


def test_refusals_leave_source_and_destination_alone(S, tmp_path):
    import schwarzwald_amd as swz
    out = str(tmp_path / "out")
    _refused(S, S["src"], out, "the source does not hold", attrs=("rgb", "classification"), lossy_source=True)
    _refused(S, S["src"], out, "source_flags", source_flags=2)
    _refused(S, S["src"], out, "source_flags", source_flags=swz.CONVERT_LOSSY_SOURCE | 0x80000000)
    # the second file with another RTC_CENTER: what convert_dataset_world writes; the file is named
    other = str(tmp_path / "other")
    shutil.copytree(S["src"], other)
    second = S["names"][1]
    xyz, cols, rtc = S["rows"][second]
    swz.pnts_write_node_rows(os.path.join(other, second + ".pnts"), xyz, cols, write=list(NAMES), rtc_center=(1000.5, -20.25, 3.5))
    assert swz.dataset_scan(other)["points"] == S["scan"]["points"]                   # the scan takes it as before
    for world in (False, True):
        _refused(S, other, out, second + ".pnts", world=world, lossy_source=True)
        _refused(S, other, out, "RTC_CENTER", world=world, lossy_source=True)
    # a file cut short after it was written: its lengths no longer add up (the header of a .pnts file says all the readers
    # check, so the scan at the head of the call already names it)
    bad = str(tmp_path / "bad")
    shutil.copytree(S["src"], bad)
    k = int(np.argmax(S["nodes"]["count"][5:])) + 5
    path = os.path.join(bad, S["names"][k] + ".pnts")
    blob = open(path, "rb").read()
    open(path, "wb").write(blob[:len(blob) - len(blob) // 3])
    _refused(S, bad, out, S["names"][k] + ".pnts", lossy_source=True)
    # the flag on a source of another format does nothing; and the next call on the good directory works
    as_bin, again = str(tmp_path / "as_bin"), str(tmp_path / "again")
    swz.convert_dataset(S["ctx"], S["src"], as_bin, "BIN", chunk_points=CHUNK, lossy_source=True)
    swz.convert_dataset(S["ctx"], as_bin, again, "3DTILES", global_offset=GLOBAL_OFFSET, chunk_points=CHUNK, lossy_source=True)
    _assert_same(again, S["src"])


def test_world_conversion_equals_that_of_the_host_built_bin_source(S, tmp_path):
    import schwarzwald_amd as swz
    as_bin = str(tmp_path / "as_bin")
    _expected(S, as_bin, "BIN")
    shutil.copy(os.path.join(S["src"], PROPS), os.path.join(as_bin, PROPS))
    want, out = str(tmp_path / "want"), str(tmp_path / "out")
    swz.convert_dataset_world(S["ctx"], as_bin, want, UTM32, chunk_points=CHUNK)
    stats = swz.convert_dataset_world(S["ctx"], S["src"], out, UTM32, chunk_points=CHUNK, lossy_source=True)
    _assert_same(out, want)
    assert _snapshot(out)[PROPS] == _snapshot(want)[PROPS] and stats["chunks"] >= 3
    # and the result is a data set of per-node origins: it is not converted back
    _refused(S, out, str(tmp_path / "back"), "RTC_CENTER", lossy_source=True)
