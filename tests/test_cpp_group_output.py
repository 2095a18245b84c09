"""swz_group_write_output, driven by tests/cpp/test_group_output.cpp: a data set tiled on a group of 1, 2, 4 or 8 shards (all on
device 0) is written in one call and must be the directory swz_tiler_write_output writes for a single tiler fed the same
batches in the same process -- the same relative paths, every file byte for byte, the JSON, ept-hierarchy and .binz files
included.  The program asserts that no two points share a Morton key, so the order inside every file is defined by the keys
alone.  What each shard count covers is listed at the program's legs; the 8-shard run adds the edge data sets, the refusals
and the leg through ShardedTilingAlgorithmGPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (shards, part of the program's legs) -> the directory pairs it announces.  8 shards: one case per leg, the FAST leg one per
# format (it writes 76 115 files per directory; see the program's head)
CASES = {(1, ""): 2, (2, ""): 2, (4, ""): 2,
         (8, "acc_md"): 5 + 1 + 1 + 6 + 1,  # five formats, chunk_points 0, log / UTM, a valid call after each of six refusals, re-opened
         (8, "acc_rg"): 5,
         (8, "fast_rg_bin"): 1, (8, "fast_rg_binz"): 1, (8, "fast_rg_3dtiles"): 1, (8, "fast_rg_las"): 1, (8, "fast_rg_ept"): 1,
         (8, "edges"): 3 + 5 + 1}  # one octant, take-all, the adapter


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the program, built once for all cases"""
    out = str(tmp_path_factory.mktemp("build") / "test_group_output")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_group_output.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def _tree(top):
    out = {}
    for base, _, files in os.walk(top):
        for f in files:
            path = os.path.join(base, f)
            out[os.path.relpath(path, top)] = path
    return out


def test_group_output_test_compiles_against_the_abi(exe):
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    assert os.path.exists(exe)


@pytest.mark.gpu
@pytest.mark.parametrize("shards,part", sorted(CASES))
def test_group_output_is_the_single_tilers_directory(tmp_path, exe, shards, part):
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work), str(shards)] + ([part] if part else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    pairs = [line.split()[1:] for line in r.stdout.splitlines() if line.startswith("pair ")]
    assert len(pairs) == CASES[shards, part] and "pairs %d" % CASES[shards, part] in r.stdout, r.stdout
    if part == "acc_md":
        assert r.stdout.count("refused: ") == 8, r.stdout
        assert not (work / "refused").exists()
    for want_dir, got_dir in pairs:
        want, got = _tree(want_dir), _tree(got_dir)
        assert sorted(got) == sorted(want), (got_dir, sorted(set(got) ^ set(want))[:10])
        assert len(want) >= 1
        for rel in sorted(want):
            with open(want[rel], "rb") as a, open(got[rel], "rb") as b:
                assert a.read() == b.read(), (got_dir, rel)
    if part == "acc_md":  # the main legs write a real tree, not a root alone
        assert len(_tree(str(work / "single_acc_md_bin"))) > 100
        assert "ept.json" in _tree(str(work / "single_acc_md_ept"))
