"""MIN_DISTANCE_FAST without a GPU: the expected-value helper (tests/md_fast_ref.py) against a brute-force greedy and, with
the stride forced to one, against the oracle's MIN_DISTANCE; the host functions of the ABI; the adapter's factories."""
import os
import subprocess

import numpy as np
import pytest

import md_fast_ref as R
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


def _brute_force(xyz, idx, n, spacing_node):
    """every n-th element offered in order; accepted when no accepted point is closer than the spacing:
    squared distance in doubles against (double)(float spacing * float spacing), strict <"""
    sq = float(np.float32(spacing_node) * np.float32(spacing_node))
    taken = np.zeros(len(idx), dtype=np.uint8)
    kept = []
    for k in range(0, len(idx), n):
        p = xyz[idx[k]]
        ok = True
        for q in kept:
            d = p - q
            if d[0] * d[0] + d[1] * d[1] + d[2] * d[2] < sq:
                ok = False
                break
        if ok:
            kept.append(p)
            taken[k] = 1
    return taken


@pytest.mark.parametrize("node_level,count", [(-1, 401), (-1, 400), (-1, 403), (0, 333), (0, 334), (1, 257)])
def test_helper_matches_a_brute_force_greedy(node_level, count):
    rng = np.random.default_rng(1000 + 10 * node_level + count)
    # points inside one node of that level: the first octant chain
    ext = 0.5 ** (node_level + 1)
    xyz = rng.random((count, 3)) * ext
    keys, xc = O.index_points(xyz, *UNIT)
    perm = O.sort_by_key(keys)
    spacing = 0.11
    t = R.sample_points(10, keys[perm], perm, xc, 0, node_level, *UNIT, spacing)
    n = R.stride(node_level)
    assert n == {-1: 4, 0: 2}.get(node_level, 1)
    expect = _brute_force(xc, perm, n, np.float32(spacing) / 2.0 ** (node_level + 1))
    assert np.array_equal(t, expect)
    assert t[0] == 1 and 1 < t.sum() < len(range(0, count, n))  # some candidates are rejected, some taken
    assert not t[np.arange(count) % n != 0].any()               # nobody else is ever taken


def test_helper_rules_one_and_two():
    rng = np.random.default_rng(3)
    xyz = rng.random((50, 3))
    keys, xc = O.index_points(xyz, *UNIT)
    perm = O.sort_by_key(keys)
    assert R.sample_points(50, keys[perm], perm, xc, 0, -1, *UNIT, 0.1).all()                          # count <= max_points
    assert R.sample_points(50, keys[perm], perm, xc, 0, -1, *UNIT, 0.1, O.ALWAYS_ADHERE).sum() < 14   # still strided
    first = R.sample_points(10, keys[perm], perm, xc, 0, -1, *UNIT, 0.51)                              # candidate level -1
    assert first[0] == 1 and first.sum() == 1
    assert R.sample_points(10, keys[perm], perm, xc, 0, -1, *UNIT, 0.49).sum() > 1
    assert R.candidate_level(1.0, 0.5, -1) == 0 and R.candidate_level(1.0, 1.0, 0) == 0
    assert R.candidate_level(1.0, 1.01, 0) == -1 and R.candidate_level(1.0, 0.99, 0) == 0


@pytest.mark.parametrize("strategy", [O.ACCURATE, O.FAST])
def test_helper_with_stride_one_is_the_oracles_min_distance(monkeypatch, strategy):
    """The restated recursion, start nodes and reconstruction carry no error of their own: with n = 1 everywhere (and no
    node at candidate level -1) they must give what the oracle gives for MIN_DISTANCE."""
    monkeypatch.setattr(R, "stride", lambda level: 1)
    rng = np.random.default_rng(17)
    xyz = rng.random((30000, 3))
    sp = O.spacing_from_diagonal(*UNIT, 24)
    ref = O.tile(xyz, *UNIT, O.MIN_DISTANCE, 150, sp, strategy=strategy, fast_concurrency=2)
    assert ref["status"] == 0
    got = R.tile(xyz, *UNIT, 150, sp, strategy=strategy, fast_start_level=ref["stats"]["fast_start_levels"])
    for name in ("keys", "perm", "level", "dup"):
        assert np.array_equal(got[name], ref[name]), name
    assert got["num_nodes"] == ref["stats"]["num_nodes"] and got["points_visited"] == ref["stats"]["points_visited"]


def test_multibatch_helper_with_stride_one_is_the_oracles_min_distance(monkeypatch):
    monkeypatch.setattr(R, "stride", lambda level: 1)
    rng = np.random.default_rng(18)
    xyz = rng.random((20000, 3))
    sp = O.spacing_from_diagonal(*UNIT, 24)
    parts = [xyz[:9000], xyz[9000:9000], xyz[9000:12000], xyz[12000:]]
    t = O.Tiler(*UNIT, O.MIN_DISTANCE, 150, sp)
    mb = R.MultiBatch(*UNIT, 150, sp)
    for p in parts:
        if len(p):
            assert t.add_batch(p) == 0
        mb.add_batch(p)
    assert t.finalize() == 0
    ex = t.export()
    got = R.files_table(mb.files)
    for name in ("level", "key", "offset", "count", "ids"):
        assert np.array_equal(got[name], ex[name]), name
    t.close()


def test_stride_function():
    import schwarzwald_amd as swz
    assert [swz.min_distance_fast_stride(l) for l in (-1, 0, 1, 20)] == [4, 2, 1, 1]
    assert all(swz.min_distance_fast_stride(l) == R.stride(l) for l in range(-1, 21))


def test_required_morton_index_depth_is_the_node_level():
    import schwarzwald_amd as swz
    for spacing in (0.5, 0.01, 1e-4):
        for l in range(-1, 21):
            assert swz.api.required_morton_index_depth(swz.MIN_DISTANCE_FAST, l, *UNIT, spacing) == l
            assert R.required_depth(l, *UNIT, spacing) == l


def test_sampler_tables():
    import schwarzwald_amd as swz
    assert swz.SAMPLERS == {"RANDOM_GRID": 0, "GRID_CENTER": 1, "MIN_DISTANCE": 2, "JITTERED": 3}
    assert swz.ALL_SAMPLERS == dict(swz.SAMPLERS, MIN_DISTANCE_FAST=4) and len(swz.ALL_SAMPLERS) == 5
    assert swz.MIN_DISTANCE_FAST == 4 and swz.api.ABI_VERSION == 3


def test_adapter_factories(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    exe = os.path.join(str(tmp_path), "test_md_fast_factory")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_md_fast_factory.cpp"), "-o", exe,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok: ") == 3
