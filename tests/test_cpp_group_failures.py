"""Builds and runs tests/cpp/test_group_failures.cpp: shards of a swz_group that fail -- a FAST batch below
fast_concurrency (every shard refuses), calls refused before a shard thread starts, and one shard alone failing at the
MIN_DISTANCE root of a batch (swept by all shards at once, and taken in turns).  Every call must come back with the
first failure as "shard N: ...", and the group must be usable afterwards; a shard that strands the others at a barrier
shows up as the time limit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmpdir):
    exe = os.path.join(tmpdir, "test_group_failures")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_group_failures.cpp"), "-o", exe,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_group_failures_test_compiles_against_the_abi(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    assert os.path.exists(_build(str(tmp_path)))


@pytest.mark.gpu
def test_group_survives_failing_shards(tmp_path):
    exe = _build(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 2, 4 and 8 shards x (FAST refusal in a tile call, in a batch, refusals up front); 2 and 8 shards x (joint root, turns)
    assert r.stdout.count(" ok") == 13, r.stdout
