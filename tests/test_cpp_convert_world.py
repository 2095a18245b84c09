"""swz_host::convert_dataset_world of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp), driven by
tests/cpp/test_convert_world.cpp: a BIN data set in UTM 32N is converted to georeferenced 3D Tiles once through the adapter and
once through the C call with the same parameters; the two directories must agree byte for byte, and the refusals surface as the
adapter's exception with the library's text."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build") / "test_convert_world")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_convert_world.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def _tree(top):
    out = {}
    for base, _, files in os.walk(top):
        for f in files:
            path = os.path.join(base, f)
            out[os.path.relpath(path, top)] = path
    return out


def test_convert_world_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_adapter_writes_the_directory_of_the_c_call(tmp_path, exe):
    import schwarzwald_amd as swz
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "convert world ok: " in r.stdout, r.stdout
    assert "refused: swz_convert_dataset_world: only 3DTILES" in r.stdout and "refused: swz_convert_dataset_world: dst_dir is src_dir" in r.stdout
    want, got = _tree(str(tmp_path / "world_c")), _tree(str(tmp_path / "world_adapter"))
    assert sorted(got) == sorted(want) and len(want) > 20
    assert "properties.json" in want and "r.json" in want and "r.pnts" in want
    for rel in sorted(want):
        with open(want[rel], "rb") as a, open(got[rel], "rb") as b:
            assert a.read() == b.read(), rel
    _, _, rtc = swz.pnts_read_node(got["r.pnts"])
    assert 6.3e6 < sum(v * v for v in rtc) ** 0.5 < 6.4e6                            # on the globe
    # the refused calls wrote nothing
    assert not os.path.exists(str(tmp_path / "refused")) or os.listdir(str(tmp_path / "refused")) == []
    assert sorted(f for f in _tree(str(tmp_path / "bin")) if not f.endswith(".bin")) == ["properties.json"]
