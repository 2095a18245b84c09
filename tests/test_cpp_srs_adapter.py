"""swz_host::SourceProjection of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp), driven by
tests/cpp/test_srs_adapter.cpp: the constructor throws the reference's "Source projection ... not recognized!" with the token
the library names, transformAABBsTo is the min / max of the eight corners that transformPositionsTo maps.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_source_projection_adapter(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    exe = os.path.join(str(tmp_path), "test_srs_adapter")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_srs_adapter.cpp"), "-o", exe, "-L" + lib_dir,
                    "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok") == 3
