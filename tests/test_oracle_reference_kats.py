"""Pins the oracle against every golden vector the reference's own unit tests hold for the hot path
(SURVEY.md section 8(c)), restated case by case, and against what oracle/_ref (the reference's stand-alone
headers compiled where they lie) computes: live when that build is present, as recorded in
tests/golden/ref_build_results.npz everywhere else.

Reference test files mirrored here (paths relative to /root/reference/schwarzwald/test/):
  TestMortonIndex.cpp:5-140, TestOctreeIndexing.cpp:72-600, TestAlgorithm.cpp:24-207.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import oracle_lib as O


def position_from_octant_indices(indices, bmin, bmax):
    """test/TestOctreeIndexing.cpp:19-43 (test helper of the reference), same operation order."""
    mn = [float(v) for v in bmin]
    mx = [float(v) for v in bmax]
    for octant in indices:
        for bit, axis in ((0b1, 2), (0b10, 1), (0b100, 0)):
            half = (mx[axis] - mn[axis]) / 2
            if octant & bit:
                mn[axis] += half
            else:
                mx[axis] -= half
    return [mn[a] + (mx[a] - mn[a]) / 2 for a in range(3)]


def key_from_octants(octants, levels):
    k = 0
    for lvl, o in enumerate(octants):
        k = O.lib().orc_set_octant_at_level(k, lvl, o, levels)
    return int(k)


# ------------------------------------------------------------------ TestMortonIndex.cpp
def test_position_helper_matches_reference_test():  # TestOctreeIndexing.cpp:45-70
    b = ([0, 0, 0], [8, 8, 8])
    assert position_from_octant_indices([0, 0], *b) == [1, 1, 1]
    assert position_from_octant_indices([3, 0], *b) == [1, 5, 5]
    assert position_from_octant_indices([0, 5], *b) == [3, 1, 3]
    assert position_from_octant_indices([2, 6], *b) == [3, 7, 1]


def test_level_constructor_and_truncate():  # TestMortonIndex.cpp:38-79
    levels = 4
    octs = [7, 6, 0, 3]
    k = key_from_octants(octs, levels)
    assert k == (7 << 9) | (6 << 6) | (0 << 3) | 3
    for lvl, o in enumerate(octs):
        assert O.lib().orc_get_octant_at_level(k, lvl, levels) == o
    assert O.lib().orc_truncate_to_level(k, 0, levels) == 7
    assert O.lib().orc_truncate_to_level(k, 1, levels) == (7 << 3 | 6)


def test_level_constructor_full_levels():  # TestMortonIndex.cpp:54-64
    octs = [5, 3, 7, 4, 0, 1, 6, 4, 3, 5, 3, 6, 7, 3, 2, 1, 4, 0, 2, 5, 6]
    k = key_from_octants(octs, 21)
    for lvl, o in enumerate(octs):
        assert O.lib().orc_get_octant_at_level(k, lvl, 21) == o


# ------------------------------------------------------------------ TestOctreeIndexing.cpp
def test_first_level_octants():  # :72-100
    pts = [[0.25, 0.25, 0.25], [0.25, 0.25, 0.75], [0.25, 0.75, 0.25], [0.75, 0.25, 0.25]]
    got = [O.lib().orc_get_octant_at_level(O.morton_index(p, [0, 0, 0], [1, 1, 1], 1), 0, 1) for p in pts]
    assert got == [0, 1, 2, 4]


EXPECTED_OCTANTS_20 = [5, 3, 7, 4, 0, 1, 6, 4, 3, 5, 3, 6, 7, 3, 2, 1, 4, 0, 2, 5]


def test_multi_level_key():  # :102-130
    b = ([0, 0, 0], [1 << 20] * 3)
    p = position_from_octant_indices(EXPECTED_OCTANTS_20, *b)
    k = O.morton_index(p, *b, levels=20)
    assert [O.lib().orc_get_octant_at_level(k, i, 20) for i in range(20)] == EXPECTED_OCTANTS_20


def test_smart_equals_naive():  # :584-600
    b = ([0, 0, 0], [1 << 20] * 3)
    p = position_from_octant_indices(EXPECTED_OCTANTS_20, *b)
    assert O.morton_index(p, *b, levels=20) == O.morton_index(p, *b, levels=20, naive=True)
    assert O.morton_index(p, *b, levels=20) == key_from_octants(EXPECTED_OCTANTS_20, 20)


def test_smart_equals_naive_random():
    rng = np.random.default_rng(7)
    b = ([-3.0, 2.0, 10.0], [5.0, 10.0, 18.0])
    for _ in range(2000):
        # dyadic positions: the naive descent and the scaled cast agree exactly on them
        p = [b[0][a] + rng.integers(0, 1 << 21) * (8.0 / (1 << 21)) + 8.0 / (1 << 22) for a in range(3)]
        assert O.morton_index(p, *b, levels=21) == O.morton_index(p, *b, levels=21, naive=True)


def test_random_grid_known_answer():  # :169-252: 32^3 lattice, spacing 32, node level 0 -> 8 points
    levels, side = 5, 32
    g = np.arange(side, dtype=np.float64) + 0.5
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)  # x outer, z inner
    bmin, bmax = [0, 0, 0], [side] * 3
    keys = np.array([O.morton_index(p, bmin, bmax, levels) for p in xyz], dtype=np.uint64)
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    taken, k2, i2 = O.sample_points(O.RANDOM_GRID, 16, keys[order], order, xyz, 0, 0, bmin, bmax, float(side),
                                    O.TAKE_ALL_WHEN_BELOW_MAX, levels=levels)
    assert taken == 8
    expected = [[0.5, 0.5, 0.5], [0.5, 0.5, 16.5], [0.5, 16.5, 0.5], [0.5, 16.5, 16.5],
                [16.5, 0.5, 0.5], [16.5, 0.5, 16.5], [16.5, 16.5, 0.5], [16.5, 16.5, 16.5]]
    assert xyz[i2[:8]].tolist() == expected
    # both halves stay Morton-sorted (:254-336)
    assert np.all(np.diff(k2[:8].astype(np.int64)) >= 0) and np.all(np.diff(k2[8:].astype(np.int64)) >= 0)


def test_random_grid_is_stable_on_random_input():  # :254-336 (seeded here)
    rng = np.random.default_rng(1234)
    xyz = rng.integers(1024, 2049, size=(1024, 3)).astype(np.float64)
    bmin, bmax = [1024] * 3, [2048] * 3
    keys, _ = O.index_points(xyz, bmin, bmax)
    order = O.sort_by_key(keys)
    taken, k2, i2 = O.sample_points(O.RANDOM_GRID, 16, keys[order], order, xyz, 0, 0, bmin, bmax, 1024.0)
    assert 0 < taken <= 1024
    assert np.all(np.diff(k2[:taken].astype(np.int64)) >= 0)
    assert np.all(np.diff(k2[taken:].astype(np.int64)) >= 0)
    assert sorted(i2.tolist()) == list(range(1024))


def test_partition_child_octants_root():  # :338-392
    pts = [[1, 1, 1], [1, 1, 3], [1, 3, 1], [1, 3, 3], [3, 1, 1], [3, 1, 3], [3, 3, 1], [3, 3, 3]]
    keys = [O.morton_index(p, [0, 0, 0], [4, 4, 4], 10) for p in pts]
    assert O.partition_child_octants(keys, 0, levels=10) == list(range(9))


def test_partition_child_octants_level4():  # :394-459
    octs = [[3, 4, 5, 2, 0], [3, 4, 5, 2, 0], [3, 4, 5, 2, 3], [3, 4, 5, 2, 5], [3, 4, 5, 2, 5], [3, 4, 5, 2, 6]]
    b = ([0, 0, 0], [32, 32, 32])
    keys = [O.morton_index(position_from_octant_indices(o, *b), *b, levels=5) for o in octs]
    assert keys == [key_from_octants(o, 5) for o in octs]
    off = O.partition_child_octants(keys, 4, levels=5)
    ranges = [(off[i], off[i + 1]) for i in range(8)]
    assert ranges == [(0, 2), (2, 2), (2, 2), (2, 3), (3, 3), (3, 5), (5, 6), (6, 6)]


def test_octant_bounds():  # :461-492
    exp = {0: ([0, 0, 0], [2, 2, 2]), 1: ([0, 0, 2], [2, 2, 4]), 2: ([0, 2, 0], [2, 4, 2]),
           3: ([0, 2, 2], [2, 4, 4]), 4: ([2, 0, 0], [4, 2, 2]), 5: ([2, 0, 2], [4, 2, 4]),
           6: ([2, 2, 0], [4, 4, 2]), 7: ([2, 2, 2], [4, 4, 4])}
    for o, (mn, mx) in exp.items():
        assert O.octant_bounds(o, [0, 0, 0], [4, 4, 4]) == (mn, mx)


def test_partition_members_inside_child_bounds():  # :494-554 (seeded here)
    rng = np.random.default_rng(99)
    xyz = rng.integers(1024, 2049, size=(1024, 3)).astype(np.float64)
    bmin, bmax = [1024] * 3, [2048] * 3
    keys = np.array([O.morton_index(p, bmin, bmax, 10) for p in xyz], dtype=np.uint64)
    order = np.argsort(keys, kind="stable")
    off = O.partition_child_octants(keys[order], 0, levels=10)
    for o in range(8):
        mn, mx = O.octant_bounds(o, bmin, bmax)
        pts = xyz[order[off[o]:off[o + 1]]]
        assert np.all(pts >= np.array(mn)) and np.all(pts <= np.array(mx))


def test_bounds_from_morton_index():  # :556-582
    k = O.lib().orc_set_octant_at_level(0, 0, 0, 21)
    assert O.bounds_from_morton_index(k, [0, 0, 0], [2, 2, 2], 1) == ([0, 0, 0], [1, 1, 1])
    k = key_from_octants([1, 4, 5], 21)
    assert O.bounds_from_morton_index(k, [0, 0, 0], [8, 8, 8], 3) == ([3, 0, 5], [4, 1, 6])


# ------------------------------------------------------------------ TestAlgorithm.cpp
@pytest.mark.parametrize("count", [1024, 1025])
def test_stable_partition_with_jumps(count):  # :24-80 (seeded here)
    rng = np.random.default_rng(count)
    v = np.sort(rng.integers(0, 1000, size=count).astype(np.int32))
    exp_matches = int(np.sum(v % 7 == 0))
    buf = v.copy()
    pivot = O.lib().orc_stable_partition_take_multiples(buf.ctypes.data_as(C.POINTER(C.c_int32)), count, 7)
    assert pivot == exp_matches
    assert np.all(np.diff(buf[:pivot]) >= 0) and np.all(np.diff(buf[pivot:]) >= 0)
    assert np.all(buf[:pivot] % 7 == 0) and np.all(buf[pivot:] % 7 != 0)
    R = O.ref()
    if R is not None:
        rbuf = v.copy()
        rp = R.ref_stable_partition_take_multiples(rbuf.ctypes.data_as(C.POINTER(C.c_int32)), count, 7)
        assert rp == pivot and np.array_equal(rbuf, buf)


def _merge(fn, lists):
    arrs = [np.array(l, dtype=np.int32) for l in lists]
    ptrs = (C.POINTER(C.c_int32) * len(arrs))(*[a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arrs])
    sizes = (C.c_int64 * len(arrs))(*[len(a) for a in arrs])
    out = np.zeros(sum(len(a) for a in arrs), dtype=np.int32)
    fn(ptrs, sizes, len(arrs), out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out.tolist()


MERGE_CASES = [  # TestAlgorithm.cpp:82-207
    ([[1, 2, 3, 4]], [1, 2, 3, 4]),
    ([[]], []),
    ([[1, 3, 7, 9], [2, 4, 6, 8]], [1, 2, 3, 4, 6, 7, 8, 9]),
    ([[1, 3, 7, 9, 11, 13], [2, 4, 24]], [1, 2, 3, 4, 7, 9, 11, 13, 24]),
    ([[1, 3, 7, 9], []], [1, 3, 7, 9]),
    ([[1, 3, 7, 9, 11, 13], [2, 4, 24], [5, 6, 13, 16, 99], [1, 3, 4, 5, 6, 8, 9, 44, 55, 66, 77, 88, 99]],
     [1, 1, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 8, 9, 9, 11, 13, 13, 16, 24, 44, 55, 66, 77, 88, 99, 99]),
]


@pytest.mark.parametrize("lists,expected", MERGE_CASES)
def test_merge_ranges(lists, expected):
    assert _merge(O.lib().orc_merge_ranges_i32, lists) == expected
    if O.ref() is not None:
        assert _merge(O.ref().ref_merge_ranges_i32, lists) == expected


# ------------------------------------------------------------------ oracle vs oracle/_ref
# What oracle/_ref computes on the inputs below is recorded in tests/golden/ref_build_results.npz (tools/gen_golden.py):
# the oracle is checked against the live build where oracle/_ref exists -- which must still give the recorded results --
# and against the record everywhere else.
REF_BUILD_RESULTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_build_results.npz")
PARTITION_CASES = ((0.2, -1), (0.05, -1), (0.01, -1), (0.05, 1))


def morton_ops_cases():
    """(key, level, octant, levels) rows, seeded"""
    rng = np.random.default_rng(5)
    rows = []
    for levels in (1, 2, 4, 5, 10, 20, 21):
        mask = (1 << (3 * levels)) - 1
        for _ in range(300):
            key = int(rng.integers(0, 1 << 63, dtype=np.uint64)) & mask
            lvl = int(rng.integers(0, levels))
            rows.append((key, lvl, int(rng.integers(0, 8)), levels))
    return np.array(rows, dtype=np.uint64)


def partition_input():
    """20 000 seeded points, Morton-sorted: (sorted keys, their point indices, the points)"""
    rng = np.random.default_rng(77)
    xyz = rng.random((20000, 3))
    keys, _ = O.index_points(xyz, [0, 0, 0], [1, 1, 1])
    order = O.sort_by_key(keys)
    return keys[order], order, xyz


def partition_candidate_level(spacing, node_level):
    return O.lib().orc_required_morton_index_depth(O.RANDOM_GRID, node_level, O._vec3([0, 0, 0]), O._vec3([1, 1, 1]),
                                                   C.c_float(spacing))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def reference_build_results(R):
    """What the reference build R gives on morton_ops_cases() and PARTITION_CASES (arrays of a partition as SHA-256)."""
    cases = morton_ops_cases()
    res = {"morton_cases": cases,
           "truncate_to_level": np.array([R.ref_truncate_to_level(int(k), int(l), int(n)) for k, l, _, n in cases], np.uint64),
           "get_octant_at_level": np.array([R.ref_get_octant_at_level(int(k), int(l), int(n)) for k, l, _, n in cases], np.uint8),
           "set_octant_at_level": np.array([R.ref_set_octant_at_level(int(k), int(l), int(o), int(n)) for k, l, o, n in cases],
                                           np.uint64),
           "morton_ctor_ff_2": np.uint64(R.ref_morton_ctor(0xFF, 2)),
           "morton_ctor_12345_20": np.uint64(R.ref_morton_ctor(12345, 20)),
           "morton_from_levels_7603": np.uint64(R.ref_morton_from_levels((C.c_uint8 * 4)(7, 6, 0, 3), 4))}
    buf = C.create_string_buffer(32)
    R.ref_morton64_to_string(key_from_octants(list(range(8)), 21), 8, buf, 32)
    res["morton64_to_string_01234567"] = np.array(buf.value.decode())
    res["morton64_from_string_r01234567"] = np.uint64(R.ref_morton64_from_string(b"r01234567"))
    skeys, sidx, _ = partition_input()
    taken, kd, id_ = [], [], []
    for spacing, node_level in PARTITION_CASES:
        rk, ri = skeys.copy(), sidx.copy()
        taken.append(R.ref_partition_first_of_cell(rk.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   ri.ctypes.data_as(C.POINTER(C.c_uint32)), len(rk),
                                                   partition_candidate_level(spacing, node_level)))
        kd.append(_sha(rk))
        id_.append(_sha(ri))
    res.update(partition_taken=np.array(taken, np.int64), partition_keys_sha256=np.array(kd), partition_idx_sha256=np.array(id_))
    return res


def recorded_reference_results():
    """the recorded results; where oracle/_ref is built it must still compute exactly those"""
    rec = np.load(REF_BUILD_RESULTS)
    rec = {k: rec[k] for k in rec.files}
    assert np.array_equal(rec["morton_cases"], morton_ops_cases())  # (a record of these very inputs)
    if O.ref() is not None:
        live = reference_build_results(O.ref())
        assert sorted(live) == sorted(rec)
        for k, v in live.items():
            assert np.array_equal(np.asarray(v), rec[k]), k
    return rec


def test_morton_index_ops_match_reference_build():
    R, L = recorded_reference_results(), O.lib()
    cases = morton_ops_cases()
    assert [L.orc_truncate_to_level(int(k), int(l), int(n)) for k, l, _, n in cases] == R["truncate_to_level"].tolist()
    assert [L.orc_get_octant_at_level(int(k), int(l), int(n)) for k, l, _, n in cases] == R["get_octant_at_level"].tolist()
    assert [L.orc_set_octant_at_level(int(k), int(l), int(o), int(n)) for k, l, o, n in cases] == R["set_octant_at_level"].tolist()
    # TestMortonIndex.cpp:26-36: the value constructor discards bits outside of range
    assert int(R["morton_ctor_ff_2"]) == 0x3F
    assert int(R["morton_ctor_12345_20"]) == 12345
    assert int(R["morton_from_levels_7603"]) == key_from_octants([7, 6, 0, 3], 4)
    assert str(R["morton64_to_string_01234567"]) == "01234567"  # TestMortonIndex.cpp:88-105
    assert int(R["morton64_from_string_r01234567"]) == key_from_octants(list(range(8)), 21)


def test_random_grid_core_matches_reference_partition_routine():
    """RandomSortedGridSampling's body is the reference's stable_partition_with_jumps + truncate_to_level +
    std::partition_point (Sampling.h:253-284); run exactly those through oracle/_ref and compare."""
    R = recorded_reference_results()
    skeys, sidx, xyz = partition_input()
    for i, (spacing, node_level) in enumerate(PARTITION_CASES):
        taken, k2, i2 = O.sample_points(O.RANDOM_GRID, 1, skeys, sidx, xyz, 0, node_level, [0, 0, 0], [1, 1, 1],
                                        spacing, O.ALWAYS_ADHERE)
        assert taken == int(R["partition_taken"][i])
        assert _sha(k2) == str(R["partition_keys_sha256"][i]) and _sha(i2) == str(R["partition_idx_sha256"][i])


# ------------------------------------------------------------------ SURVEY.md section 8(a) known answers
# Values recorded in SURVEY.md from a survey-session run of the reference's own calculate_morton_index
# (that probe used stand-in Boost headers, which this round does not allow, so they are kept as data).
SURVEY_KATS = [
    ((0, 0, 0), 0x0), ((1, 1, 1), 0x7FFFFFFFFFFFFFFF), ((.5, .5, .5), 0x7000000000000000),
    ((1, 0, 0), 0x4924924924924924), ((0, 1, 0), 0x2492492492492492), ((0, 0, 1), 0x1249249249249249),
    ((0.3, 0.6, 0.9), 0x3A56A56A56A56A56), ((0.999999999, 1e-9, 0.25), 0x4B24924924924924),
]


@pytest.mark.parametrize("p,key", SURVEY_KATS)
def test_survey_unit_cube_kats(p, key):
    assert O.morton_index(p, [0, 0, 0], [1, 1, 1]) == key


def test_survey_offset_cube_kat():
    mn = [-512.25, 1000.5, -3.125]
    mx = [v + 777.7 for v in mn]
    assert O.morton_index([-100, 1500.123456789, 400], mn, mx) == 0x7080F255F85E7F48


def test_survey_misc_kats():
    s = O.spacing_from_diagonal([0, 0, 0], [1, 1, 1], 250)
    assert np.float32(s).view(np.uint32) == 0x3BE305FB
    k = O.morton_index([0.3, 0.6, 0.9], [0, 0, 0], [1, 1, 1])
    mn, mx = O.bounds_from_morton_index(k, [0, 0, 0], [1, 1, 1], 7)
    assert (mn, mx) == ([0.296875, 0.59375, 0.8984375], [0.3046875, 0.6015625, 0.90625])
    g = (C.c_uint64 * 3)()
    O.lib().orc_to_grid_index((5 << 6) | (3 << 3) | 6, 3, g)  # to_grid_index([5,3,6]) = (5,3,6)
    assert list(g) == [5, 3, 6]
    # d=250 on a cube: grid samplers sample 7 levels below the node (128 cells per axis)
    for lvl in (-1, 0, 3):
        for smp in (O.RANDOM_GRID, O.GRID_CENTER, O.JITTERED):
            assert O.lib().orc_required_morton_index_depth(smp, lvl, O._vec3([0, 0, 0]), O._vec3([1, 1, 1]),
                                                           C.c_float(s)) == lvl + 7
        assert O.lib().orc_required_morton_index_depth(O.MIN_DISTANCE, lvl, O._vec3([0, 0, 0]),
                                                       O._vec3([1, 1, 1]), C.c_float(s)) == lvl
