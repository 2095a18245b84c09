"""Builds and runs the C++ host adapter tests (tests/cpp/): the reference-shaped C++ interface over the C ABI
(schwarzwald_amd/host/swz_tiling.hpp), checked with the invariants of the reference's own (disabled) tiler tests and
against the oracle.

test_adapter.cpp        TilingAlgorithmGPU on one uniform cloud (the original test)
test_adapter_seams.cpp  the free functions: index_points, sort_indexed_points, sample_points, octant boxes, names
test_adapter_tiler.cpp  TilingAlgorithmGPU on FAST, outliers, odd batches, terminal and re-rooted nodes, export chunks,
                        refusals, spilled pools

The two new executables take --oracle-only: every input is built, the oracle side and the pure-host checks run, and
each input is shown to hold its hard case -- without a GPU.  Both modes print the same "<case> ok:" lines, one per
case of the table, so the counts below are the whole table in either mode."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test_adapter_seams.cpp: index_points 6 sizes x 2 bounds, lattice, Abort; sort 3 kinds x 7 sizes; sample_points
# 2 clouds x 4 samplers x 2 behaviours x 6 ranges, known answer, JITTERED refusal; boxes x 2 bounds, names, factory
SEAMS_CASES = 6 * 2 + 2 + 3 * 7 + 2 * 4 * 2 * 6 + 2 + 2 + 1 + 1
# test_adapter_tiler.cpp: samplers x strategies; duplicates 2 x 2; terminal 2; re-rooted 3 x 2; chunks 2 x 6; empty
# batch; FAST refusals 2; nothing to hand over 2; after finalize; spill 2; set_option
TILER_CASES = 4 * 2 + 2 * 2 + 2 + 3 * 2 + 2 * 6 + 1 + 2 + 2 + 1 + 2 + 1


def _build(tmpdir, name="test_adapter"):
    exe = os.path.join(tmpdir, name)
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    orc_dir = os.path.join(ROOT, "oracle")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe,
                    "-L" + lib_dir, "-lswz_gpu", "-L" + orc_dir, "-loracle",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + orc_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _make_library():
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)


def test_adapter_compiles_against_the_abi(tmp_path):
    _make_library()
    assert os.path.exists(_build(str(tmp_path)))


def test_adapter_seams_compiles_against_the_abi(tmp_path):
    _make_library()
    assert os.path.exists(_build(str(tmp_path), "test_adapter_seams"))


def test_adapter_tiler_compiles_against_the_abi(tmp_path):
    _make_library()
    assert os.path.exists(_build(str(tmp_path), "test_adapter_tiler"))


@pytest.mark.parametrize("name,cases", [("test_adapter_seams", SEAMS_CASES), ("test_adapter_tiler", TILER_CASES)])
def test_adapter_case_tables_hold_their_hard_cases(tmp_path, name, cases):
    """--oracle-only: no swz_host::Context is created.  Every generator must produce what its case is there for
    (outliers beyond all six faces, keys on both sides of a cell edge, FAST copies, an overfull terminal node, a node
    below the first re-rooted level, a chunk size that names its nodes, a batch the oracle refuses too, no file read
    back out of order) -- before the table reaches a GPU."""
    _make_library()
    exe = _build(str(tmp_path), name)
    r = subprocess.run([exe, "--oracle-only"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert r.stdout.count(" ok: ") == cases
    assert r.stdout.count("[oracle only]") == cases


@pytest.mark.gpu
def test_adapter_tiles_like_the_oracle(tmp_path):
    exe = _build(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok: ") == 8


@pytest.mark.gpu
def test_adapter_seams_match_the_oracle(tmp_path):
    exe = _build(str(tmp_path), "test_adapter_seams")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert r.stdout.count(" ok: ") == SEAMS_CASES
    assert r.stdout.count("[gpu == oracle]") == SEAMS_CASES


@pytest.mark.gpu
def test_adapter_tiler_hands_over_the_oracles_files(tmp_path):
    exe = _build(str(tmp_path), "test_adapter_tiler")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr
    assert r.stdout.count(" ok: ") == TILER_CASES
    assert r.stdout.count("[gpu == oracle]") == TILER_CASES
