"""swz_host::convert_dataset of the C++ host adapter with its lossy_source switch, driven by tests/cpp/test_convert_pnts.cpp: a
3DTILES data set written by TilingAlgorithmGPU::write_output (+ write_properties) is refused without the switch, with the
library's text; with it, it is converted to BIN, and BIN converted back must be the first directory byte for byte."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build") / "test_convert_pnts")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_convert_pnts.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def _tree(top):
    out = {}
    for base, _, files in os.walk(top):
        for f in files:
            path = os.path.join(base, f)
            out[os.path.relpath(path, top)] = path
    return out


def test_convert_pnts_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_round_trip_through_bin_gives_the_source_and_the_default_refuses(tmp_path, exe):
    import schwarzwald_amd as swz
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "convert ok: " in r.stdout and "refused: swz_convert_dataset: a 3DTILES source" in r.stdout, r.stdout
    want, got = _tree(str(tmp_path / "tiles")), _tree(str(tmp_path / "tiles_again"))
    assert sorted(got) == sorted(want) and len(want) > 20
    for rel in sorted(want):
        with open(want[rel], "rb") as a, open(got[rel], "rb") as b:
            assert a.read() == b.read(), rel
    # the BIN directory in between holds the stored floats, widened
    scan = swz.dataset_scan(str(tmp_path / "bin"))
    assert scan["format"] == "BIN" and scan["attrs"] == ["rgb", "intensity"] and scan["points"] >= 9000
    xyz, _ = swz.bin_read_node(str(tmp_path / "bin" / "r.bin"))
    assert np.array_equal(xyz, xyz.astype(np.float32).astype(np.float64))
