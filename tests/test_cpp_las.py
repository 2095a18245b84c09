"""LASSink and EntwineSink of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp), driven by tests/cpp/test_las_sink.cpp.

The program writes directories of LAS node files and Entwine hierarchy files through the sinks and dumps its inputs; the
expected directories are built here from those inputs with the Python binding's host writers (which
tests/test_las_persistence.py checks against hand-written bytes) -- and, for the GPU case, from the rows the oracle assigns
to every node.  Node files are compared byte for byte, hierarchy files by parsed value."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
NAMES = ["r", "r3", "r30", "r301", "r3011", "r5"]
COUNTS = [5, 1, 2, 3, 300, 7]


def _build(tmpdir):
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    exe = os.path.join(tmpdir, "test_las_sink")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_las_sink.cpp"), "-o", exe,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _node(name):
    key = 0
    for l, ch in enumerate(name[1:]):
        key |= int(ch) << (3 * (20 - l))
    return len(name) - 2, key


def _same_files(got, want):
    assert sorted(os.listdir(got)) == sorted(os.listdir(want))
    for f in os.listdir(want):
        a, b = open(os.path.join(got, f), "rb").read(), open(os.path.join(want, f), "rb").read()
        if f.endswith(".json"):
            assert json.loads(a) == json.loads(b), f
        else:
            assert a == b, f


def _same_ept(got, want):
    assert sorted(os.listdir(got)) == sorted(os.listdir(want)) == ["ept-data", "ept-hierarchy", "ept-sources"]
    for sub in ("ept-data", "ept-hierarchy", "ept-sources"):
        _same_files(os.path.join(got, sub), os.path.join(want, sub))


def _write_node(swz, directory, name, xyz, attrs, entwine):
    lv, key = _node(name)
    b_min, b_max = swz.node_bounds(lv, key, *UNIT)
    path = os.path.join(directory, "ept-data", swz.node_name_entwine(lv, key) + ".las") if entwine else os.path.join(directory, name + ".las")
    swz.las_write_node_rows(path, xyz, attrs, b_min, b_max, swz.las_scale_from_bounds(b_min, b_max))


def test_sinks_write_what_the_host_writers_write(tmp_path):
    import schwarzwald_amd as swz
    exe = _build(str(tmp_path))
    for d in ("input", "las", "want_las"):
        (tmp_path / d).mkdir()
    for d in ("want_ept", "want_plain"):
        swz.ept_create_dirs(str(tmp_path / d))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sink ok: 3 directories of 6 nodes" in r.stdout
    xyz = np.fromfile(tmp_path / "input" / "xyz.f64", np.float64).reshape(-1, 3)
    rgb = np.fromfile(tmp_path / "input" / "rgb.u8", np.uint8).reshape(-1, 3)
    inten = np.fromfile(tmp_path / "input" / "intensity.u16", np.uint16)
    gps = np.fromfile(tmp_path / "input" / "gps.f64", np.float64)
    assert len(xyz) == sum(COUNTS)
    at = 0
    for name, c in zip(NAMES, COUNTS):
        s = slice(at, at + c)
        attrs = {"rgb": rgb[s], "intensity": inten[s], "gps_time": gps[s]}
        _write_node(swz, str(tmp_path / "want_las"), name, xyz[s], attrs, False)
        _write_node(swz, str(tmp_path / "want_ept"), name, xyz[s], attrs, True)
        _write_node(swz, str(tmp_path / "want_plain"), name, xyz[s], {}, True)
        at += c
    levels, keys = zip(*[_node(n) for n in NAMES])
    for d in ("want_ept", "want_plain"):
        swz.ept_hierarchy_write(str(tmp_path / d), dict(level=levels, key=keys, count=COUNTS))
    _same_files(str(tmp_path / "las"), str(tmp_path / "want_las"))
    _same_ept(str(tmp_path / "ept"), str(tmp_path / "want_ept"))
    _same_ept(str(tmp_path / "plain"), str(tmp_path / "want_plain"))        # its hierarchy was written by the destructor
    assert sorted(os.listdir(tmp_path / "ept" / "ept-hierarchy")) == ["0-0-0-0.json"]      # the deepest node has four octants
    assert swz.las_read_header(str(tmp_path / "las" / "r3011.las"))["point_format"] == 3
    assert swz.las_read_header(str(tmp_path / "plain" / "ept-data" / "0-0-0-0.las"))["point_format"] == 0


@pytest.mark.gpu
def test_tiling_algorithm_with_the_entwine_sink_writes_the_oracles_nodes(tmp_path):
    import schwarzwald_amd as swz
    from test_pnts_persistence import _oracle_node_rows
    exe = _build(str(tmp_path))
    (tmp_path / "input").mkdir()
    swz.ept_create_dirs(str(tmp_path / "want"))
    r = subprocess.run([exe, str(tmp_path), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    xyz = np.fromfile(tmp_path / "input" / "xyz_gpu.f64", np.float64).reshape(-1, 3)
    spacing = float(np.float32(np.sqrt(3.0) / 16.0))
    o = O.tile(xyz, *UNIT, O.GRID_CENTER, 500, spacing)
    assert o["status"] == 0
    want = _oracle_node_rows(o)
    assert "sink ok: %d nodes" % len(want) in r.stdout
    for name, rows in want.items():
        _write_node(swz, str(tmp_path / "want"), name, xyz[rows], {}, True)
    levels, keys = zip(*[_node(n) for n in want])
    swz.ept_hierarchy_write(str(tmp_path / "want"), dict(level=levels, key=keys, count=[len(v) for v in want.values()]))
    _same_ept(str(tmp_path / "gpu"), str(tmp_path / "want"))
