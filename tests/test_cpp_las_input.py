"""TilingAlgorithmGPU::add_las_files of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp), driven by
tests/cpp/test_las_input.cpp: two LAS files (LAS 1.2 format 3 with an extra byte, LAS 1.4 format 7) read, decoded and tiled
through the adapter in batches that cross the file boundary; the files handed to the sink are the oracle's (orc_tiler_* over
orc_las_decode of the same records and the same cuts): names, ids in file order, positions bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmpdir):
    exe = os.path.join(tmpdir, "test_las_input")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    orc_dir = os.path.join(ROOT, "oracle")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_las_input.cpp"), "-o", exe,
                    "-L" + lib_dir, "-lswz_gpu", "-L" + orc_dir, "-loracle",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + orc_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_las_input_adapter_compiles_against_the_abi(tmp_path):
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_adapter_reads_las_files_like_the_oracle(tmp_path):
    exe = _build(str(tmp_path))
    (tmp_path / "files").mkdir()
    r = subprocess.run([exe, str(tmp_path / "files")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "las input ok:" in r.stdout and "[gpu == oracle]" in r.stdout
