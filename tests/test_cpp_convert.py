"""swz_host::convert_dataset of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp), driven by tests/cpp/test_convert.cpp:
a BIN data set written by TilingAlgorithmGPU::write_output (+ write_properties) is converted to ENTWINE_LAS and must be the
directory write_output writes directly, byte for byte, plus properties.json; a refusal surfaces as the adapter's exception with
the library's text."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build") / "test_convert")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_convert.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def _tree(top):
    out = {}
    for base, _, files in os.walk(top):
        for f in files:
            path = os.path.join(base, f)
            out[os.path.relpath(path, top)] = path
    return out


def test_convert_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_converted_directory_is_the_direct_one(tmp_path, exe):
    import schwarzwald_amd as swz
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "convert ok: " in r.stdout and "refused: swz_convert_dataset: dst_dir is src_dir" in r.stdout, r.stdout
    want, got = _tree(str(tmp_path / "ept_direct")), _tree(str(tmp_path / "ept_converted"))
    assert sorted(got) == sorted(list(want) + ["properties.json"])
    assert len(want) > 20
    for rel in sorted(want):
        with open(want[rel], "rb") as a, open(got[rel], "rb") as b:
            assert a.read() == b.read(), rel
    props = swz.properties_json_read(str(tmp_path / "ept_converted"))
    assert props["processed_points"] == 9000 and props["root_min"].tolist() == [0, 0, 0] and props["root_max"].tolist() == [1, 1, 1]
    # the refused call wrote nothing into its source
    assert sorted(f for f in _tree(str(tmp_path / "bin")) if not f.endswith(".bin")) == ["properties.json"]
