"""MIN_DISTANCE_FAST on the data of tests/test_min_distance_adversarial.py -- lattices with pairs exactly at a level's spacing,
LAS records quantised to a millimetre at UTM offsets, stacks of hundreds of duplicates, non-cubic bounds -- and on one family of
its own for the "first point only" rule.  The sampler adds a candidate selection in front of MIN_DISTANCE (every 4th point of
the root, every 2nd of a level-0 node, counted from the node's own first point), so what can go wrong sits there: where the
stride starts, what it does inside a run of equal keys, candidates that are neighbours in space but not in the array, the
candidate level taken from the x extent alone, and node contents that change between the batches of a tiler.  Every
comparison is exact, point for point, with tests/md_fast_ref.py.

The CPU tests at the top check that each family really produces its hard case for THIS sampler (among the candidates, not
among all points), so that a change to a generator cannot quietly remove it.

Sizes: the reference recursion of md_fast_ref takes 0.1 to 0.9 s per single-batch ACCURATE case at full size, so no family is
cut for time.  'stacks' is cut by a few dozen points: in every level-0 octant the points in front of the first stack are left
out, so that the stride of the root and of every level-0 node starts counting inside a run of equal keys (the family's own
seed puts single points there).

Multi-batch legs: the library sorts a file whose re-keyed points are no longer ascending, the reference merges it as it is
(swz_tiler_info.rekey_inversions; test_multibatch.py::test_gpu_rekey_inversion_is_counted_and_confined).  Three batches of
the cloud shuffled with seed 0 are free of such files for five families; test_multi_batch_split_is_free_of_unsorted_files
asserts it.  Two families are left out of the multi-batch legs (MULTI_LEFT_OUT), because the reference reads files back out of
order for every split tried (seeds 0..4, two to four batches): 'lattice-0.001', whose points sit on key-cell boundaries by
construction (570 to 7900 such files per split), and 'las-aabb' (1 to 5 files per split).  'lattice', 'las-cubic', 'stacks',
'crowded-block' and 'quarter-x' stay in."""
import functools
import time

import numpy as np
import pytest

import md_fast_ref as R
import oracle_lib as O
from test_md_fast_gpu import PATHS, _compare_tables
from test_min_distance_adversarial import FAMILIES, SINGLE, _first_difference, _level_spacing, _sq_dist, _with, family

FAST4 = R.MIN_DISTANCE_FAST

# ----------------------------------------------------------------------------------------------------------- data families
# The family of this file: an AABB whose x extent (64) is a quarter of its y extent (256).  The candidate level comes from the
# x extent alone: with spacing_at_root = 32 the ratio extent.x / spacing is exactly 2 at the root, with 64 exactly 2 at level
# 0 -- one float above, the node keeps its first point only; one float below, it strides.  (The y extent would give candidate
# level 1 or 2 there.)
QUARTER = ([1000.0, 2000.0, 50.0], [1064.0, 2256.0, 178.0])
QUARTER_MAX_POINTS = 100


def _f32_neighbours(x):
    return float(np.nextafter(np.float32(x), np.float32(2 * x))), float(np.nextafter(np.float32(x), np.float32(0)))


# (spacing_at_root, the level L on whose edge it sits, first point only there?)
QUARTER_CASES = [(_f32_neighbours(32.0)[0], -1, True), (_f32_neighbours(32.0)[1], -1, False),
                 (_f32_neighbours(64.0)[0], 0, True), (_f32_neighbours(64.0)[1], 0, False)]


def _quarter_x(seed):
    """millimetre records, uniform in the box, with a few hundred of them repeated"""
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, [64001, 256001, 128001], size=(60000, 3))
    rec = np.vstack([rec, rec[rng.integers(0, 60000, 400)]])
    rec = rec[rng.permutation(rec.shape[0])]
    return rec.astype(np.float64) * 0.001 + np.array(QUARTER[0])


def _stacks_cut(xyz, bounds):
    """leaves out, in every level-0 octant, the points in front of the first position that occurs 8 times or more"""
    keys, _ = O.index_points(xyz, *bounds)
    uk, counts = np.unique(keys, return_counts=True)
    keep = np.ones(len(keys), dtype=bool)
    for o in range(8):
        stack_keys = uk[(uk >> np.uint64(60) == o) & (counts >= 8)]
        assert len(stack_keys)
        keep &= ~((keys >> np.uint64(60) == o) & (keys < stack_keys[0]))
    return xyz[keep]


@functools.lru_cache(maxsize=None)
def cloud(name):
    """name -> (xyz, bounds, [(spacing_at_root, max_points_per_node), ...])"""
    if name == "quarter-x":
        return _quarter_x(6), QUARTER, [(c[0], QUARTER_MAX_POINTS) for c in QUARTER_CASES]
    xyz, bounds, cases = family(name)
    if name == "stacks":
        xyz = _stacks_cut(xyz, bounds)
    return xyz, bounds, cases


ALL = FAMILIES + ["quarter-x"]
REFERENCE_SECONDS = {}


@functools.lru_cache(maxsize=None)
def _fast_start_level(name, concurrency):
    """The start level of FAST does not depend on the sampler, the spacing or max_points (estimate_start_node_level looks at
    the sorted keys and the concurrency): the oracle's MIN_DISTANCE run reports it, with a root that takes everything."""
    xyz, bounds, _ = cloud(name)
    o = O.tile(xyz, *bounds, O.MIN_DISTANCE, len(xyz), 1.0, strategy=O.FAST, fast_concurrency=concurrency)
    assert o["status"] == 0
    return o["stats"]["fast_start_levels"]


@functools.lru_cache(maxsize=None)
def _ref(name, case, strategy=O.ACCURATE, concurrency=0):
    xyz, bounds, cases = cloud(name)
    sp, mppn = cases[case]
    S = _fast_start_level(name, concurrency) if strategy == O.FAST else None
    t0 = time.perf_counter()
    r = R.tile(xyz, *bounds, mppn, sp, strategy=strategy, fast_start_level=S)
    if strategy == O.ACCURATE:
        REFERENCE_SECONDS[(name, case)] = time.perf_counter() - t0
    r["xyz_clamped"] = O.index_points(xyz, *bounds)[1]
    r["fast_start_level"] = S
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _nodes(r, node_level):
    """[(node_key, sorted positions)] of the nodes of a level (-1, 0 or 1) in a single-batch ACCURATE result: what the
    levels above left, split by the key prefix"""
    if node_level < 0:
        return [(0, np.arange(len(r["keys"])))]
    rest = np.flatnonzero(r["level"] >= node_level)
    sh = np.uint64(63 - 3 * (node_level + 1))
    prefix = r["keys"][rest] >> sh
    return [(int(p) << int(sh), rest[prefix == p]) for p in np.unique(prefix)]


def _sampled_nodes(name, case):
    """[(node_level, node_key, positions, candidates)] of the sampled root and level-0 nodes: more points than max_points;
    candidates are the positions the reference offers to the distance test (one, where the candidate level is -1)"""
    xyz, bounds, cases = cloud(name)
    sp, mppn = cases[case]
    r = _ref(name, case)
    out = []
    for node_level in (-1, 0):
        first_only = R.candidate_level(bounds[1][0] - bounds[0][0], sp, node_level) == -1
        for key, pos in _nodes(r, node_level):
            if len(pos) > mppn:
                out.append((node_level, key, pos, pos[:1] if first_only else pos[::R.stride(node_level)]))
    return out


def _lattice_pairs(P, units, v2):
    """Distinct positions P (doubles) with integer lattice coordinates units: the squared distances, as the reference computes
    them, of all pairs whose lattice offset v has v.v == v2."""
    units, first = np.unique(units, axis=0, return_index=True)
    P = P[first]
    r = int(np.floor(np.sqrt(v2)))
    g = np.arange(-r, r + 1)
    v = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    v = v[(v * v).sum(axis=1) == v2]
    v = v[(v[:, 0] > 0) | ((v[:, 0] == 0) & (v[:, 1] > 0)) | ((v[:, 0] == 0) & (v[:, 1] == 0) & (v[:, 2] > 0))]  # each pair once
    assert units.min() >= 0 and units.max() < 1024

    def code(u):
        return (u[:, 0] * 2048 + u[:, 1] + 512) * 2048 + u[:, 2] + 512
    codes = code(units)  # (sorted: np.unique sorts rows lexicographically)
    d2 = []
    for w in v:
        at = np.searchsorted(codes, code(units + w))
        at[at == len(codes)] = 0
        hit = codes[at] == code(units + w)
        d2.append(_sq_dist(P[hit], P[at[hit]]))
    return np.concatenate(d2) if d2 else np.zeros(0)


# --------------------------------------------------------------------------------------------------------- CPU: premises
@pytest.mark.parametrize("case", [0, 1])
def test_lattice_candidates_have_exact_ties(case):
    """pairs of CANDIDATES of one sampled node exactly at the node's spacing, d^2 == float(s^2): at least 100 in a node with
    stride 4 and in one with stride 2"""
    xyz, bounds, cases = cloud("lattice")
    r = _ref("lattice", case)
    P = r["xyz_clamped"][r["perm"]]
    best = {4: 0, 2: 0}
    for node_level, key, pos, cand in _sampled_nodes("lattice", case):
        s, sq = _level_spacing(cases[case][0], node_level)
        assert sq == int(sq), "the squared spacing of a lattice case is a whole number of squared pitches"
        units = P[cand].astype(np.int64)
        assert np.array_equal(units, P[cand])
        ties = int((_lattice_pairs(P[cand], units, int(sq)) == sq).sum())
        print("lattice case %d, level %d node %x: %d candidates, %d pairs exactly at the spacing %r" % (case, node_level, key, len(cand), ties, s))
        best[R.stride(node_level)] = max(best[R.stride(node_level)], ties)
    assert best[4] >= 100 and best[2] >= 100, best


def test_fine_lattice_candidates_have_near_ties():
    xyz, bounds, cases = cloud("lattice-0.001")
    r = _ref("lattice-0.001", 0)
    P = r["xyz_clamped"][r["perm"]]
    most = 0
    for node_level, key, pos, cand in _sampled_nodes("lattice-0.001", 0):
        s, sq = _level_spacing(cases[0][0], node_level)
        units = np.rint((P[cand] - np.array(bounds[0])) / 0.001).astype(np.int64)
        pitches = int(round(s / 0.001))
        d2 = _lattice_pairs(P[cand], units, pitches * pitches)
        near = int((np.abs(d2 / sq - 1.0) < 1e-6).sum())
        print("pitch-0.001 lattice, level %d node %x (stride %d): %d candidate pairs within 1e-6 of the spacing, %d exact ties"
              % (node_level, key, R.stride(node_level), near, int((d2 == sq).sum())))
        most = max(most, near)
    assert most >= 100


def test_stacks_put_many_candidates_at_distance_zero_and_the_stride_origin_inside_a_stack():
    xyz, bounds, cases = cloud("stacks")
    assert len(family("stacks")[0]) - len(xyz) < 1000 and len(xyz) <= 300000
    r = _ref("stacks", 0)
    P = r["xyz_clamped"][r["perm"]]
    most, origins = 0, []
    for node_level, key, pos, cand in _sampled_nodes("stacks", 0):
        _, counts = np.unique(P[cand], axis=0, return_counts=True)
        most = max(most, int(counts.max()))
        run = int(np.argmax(r["keys"][pos] != r["keys"][pos[0]]))  # length of the run of equal keys the node starts with
        in_stack = run >= 2 and np.all(P[pos[:run]] == P[pos[0]])
        origins.append((node_level, key >> 60, run if in_stack else 0))
    print("stacks: up to %d candidates of one node at one position; (level, octant, length of the stack a node starts in): %s" % (most, origins))
    assert most >= 8
    assert any(run >= 2 for _, _, run in origins)
    # a stack longer than the stride: the second candidate of the node lies in the same stack as the first
    assert any(run > R.stride(level) for level, _, run in origins)


def test_las_aabb_candidate_level_depends_on_the_x_extent():
    xyz, bounds, cases = cloud("las-aabb")
    ext = [h - l for l, h in zip(*bounds)]
    assert len({round(e, 3) for e in ext}) == 3
    split = []
    for case, (sp, mppn) in enumerate(cases):
        for node_level in range(-1, int(_ref("las-aabb", case)["level"].max()) + 1):
            cx, cy = R.candidate_level(ext[0], sp, node_level), R.candidate_level(ext[1], sp, node_level)
            if cx != cy:
                split.append((case, node_level, cx, cy))
    print("las-aabb: (case, node level, candidate level from x, from y) where they differ:", split)
    assert split


def test_quarter_x_sits_on_the_edge_of_the_first_point_only_rule():
    xyz, bounds, cases = cloud("quarter-x")
    ext = [h - l for l, h in zip(*bounds)]
    assert ext[0] * 4 == ext[1] and len(xyz) <= 300000
    for case, (sp, L, first_only) in enumerate(QUARTER_CASES):
        assert (R.candidate_level(ext[0], sp, L) == -1) == first_only
        assert R.candidate_level(ext[1], sp, L) >= 1  # (the y extent would never say "first point only")
        r = _ref("quarter-x", case)
        nodes = [(key, pos) for key, pos in _nodes(r, L) if len(pos) > QUARTER_MAX_POINTS]
        assert nodes, "level %d must be reached by a node with more than max_points points" % L
        taken = [int((r["level"][pos] == L).sum()) for key, pos in nodes]
        print("quarter-x spacing %r: level %d, %d sampled nodes keep %s points" % (sp, L, len(nodes), taken))
        assert all(t == 1 for t in taken) if first_only else all(t > 1 for t in taken)


@pytest.mark.parametrize("name", ALL)
def test_every_family_samples_the_root_and_level_zero(name):
    """a sampled node at level -1 and one at level 0 in every case; both strides at work in every family (in 'quarter-x' not
    in every case: that is its point)"""
    strides = set()
    for case in range(len(cloud(name)[2])):
        nodes = _sampled_nodes(name, case)
        assert {lv for lv, _, _, _ in nodes} == {-1, 0}, (name, case)
        at_work = {R.stride(lv) for lv, _, pos, cand in nodes if len(cand) > 1}
        print("%s case %d: %d points, reference %.1f s, sampled nodes (level, points, candidates): %s"
              % (name, case, len(cloud(name)[0]), REFERENCE_SECONDS[(name, case)], [(lv, len(pos), len(cand)) for lv, _, pos, cand in nodes]))
        assert name == "quarter-x" or at_work == {4, 2}, (name, case)
        strides |= at_work
    assert strides == {4, 2}
    assert len(cloud(name)[0]) <= 300000


# ------------------------------------------------------------------------------------------------ the multi-batch reference
CONCURRENCY = 4
# family -> (shuffle seed, batches)
MULTI = {name: (0, 3) for name in ALL}
MULTI_LEFT_OUT = ["lattice-0.001", "las-aabb"]


@functools.lru_cache(maxsize=None)
def _parts(name, seed=None, k=None):
    xyz = cloud(name)[0]
    if seed is None:
        seed, k = MULTI[name]
    parts = np.array_split(xyz[np.random.default_rng(seed).permutation(len(xyz))], k)
    for p in parts:
        keys, _ = O.index_points(p, *cloud(name)[1])
        assert np.any(keys[1:] < keys[:-1]), "a batch arrives sorted"
    return parts


def _multi_reference(name, case, strategy, seed=None, k=None):
    xyz, bounds, cases = cloud(name)
    sp, mppn = cases[case]
    parts = _parts(name, seed, k)
    S = 0
    if strategy == O.FAST:
        o = O.tile(parts[0], *bounds, O.MIN_DISTANCE, len(parts[0]), 1.0, strategy=O.FAST, fast_concurrency=CONCURRENCY)
        assert o["status"] == 0
        S = o["stats"]["fast_start_levels"]
    mb = R.MultiBatch(*bounds, mppn, sp, start_level=S, count_unsorted=True)
    for p in parts:
        mb.add_batch(p)
    files, unsorted = mb.files, []
    if S > 0:
        files = R.reconstruct_files(files, mb.xyz, *bounds, mppn, sp, S - 1, unsorted)
    return dict(table=R.files_table(files), start_level=S, unsorted=mb.unsorted_cached_nodes + len(unsorted))


@functools.lru_cache(maxsize=None)
def _multi_ref(name, case, strategy):
    return _multi_reference(name, case, strategy)


@pytest.mark.parametrize("strategy", [O.ACCURATE, O.FAST], ids=["ACCURATE", "FAST"])
@pytest.mark.parametrize("name", [n for n in ALL if n not in MULTI_LEFT_OUT])
def test_multi_batch_split_is_free_of_unsorted_files(name, strategy):
    """the reference reads no file back out of order: the library and the reference must then agree entry for entry"""
    for case in range(len(cloud(name)[2])):
        m = _multi_ref(name, case, strategy)
        print("%s case %d %s: %d files, %d entries, start level %d, files out of order %d"
              % (name, case, "FAST" if strategy == O.FAST else "ACCURATE", len(m["table"]["level"]), len(m["table"]["ids"]), m["start_level"], m["unsorted"]))
        assert m["unsorted"] == 0, (name, case)
        if strategy == O.FAST:
            assert m["start_level"] >= 1, "no level is rebuilt by finalize"
        else:
            assert len(m["table"]["ids"]) == len(cloud(name)[0])


def test_multi_batch_families_kept():
    assert len(MULTI_LEFT_OUT) <= 2 and "stacks" not in MULTI_LEFT_OUT
    assert "lattice" not in MULTI_LEFT_OUT or "lattice-0.001" not in MULTI_LEFT_OUT


def test_fast_batches_of_the_helper_with_stride_one_are_the_oracles_min_distance(monkeypatch):
    """MultiBatch(start_level=S) and reconstruct_files carry no error of their own: with n = 1 everywhere (and no node at
    candidate level -1) they give the files of the oracle's FAST MIN_DISTANCE tiler"""
    monkeypatch.setattr(R, "stride", lambda level: 1)
    unit = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    xyz = np.random.default_rng(19).random((30000, 3))
    sp = O.spacing_from_diagonal(*unit, 24)
    parts = np.array_split(xyz, 3)
    t = O.Tiler(*unit, O.MIN_DISTANCE, 150, sp, strategy=O.FAST, fast_concurrency=CONCURRENCY)
    for p in parts:
        assert t.add_batch(p) == 0
    assert t.finalize() == 0
    ex, S = t.export(), t.stats()["fast_start_levels"]
    assert t.counts()["unsorted_cached_nodes"] == 0 and S >= 1
    t.close()
    mb = R.MultiBatch(*unit, 150, sp, start_level=S)
    for p in parts:
        mb.add_batch(p)
    got = R.files_table(R.reconstruct_files(mb.files, mb.xyz, *unit, 150, sp, S - 1))
    for col in ("level", "key", "offset", "count", "ids"):
        assert np.array_equal(got[col], ex[col]), col


# ----------------------------------------------------------------------------------------------------------- GPU: the matrix
@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


SINGLE_LEGS = dict(PATHS)
SINGLE_LEGS["every compare exact"] = SINGLE["every compare exact"]
LEGS = list(SINGLE_LEGS) + ["FAST 2", "FAST 8", "sample_points", "multi-batch ACCURATE", "multi-batch FAST"]


def _params(max_points, spacing, **kw):
    import schwarzwald_amd as swz
    return swz.TileParams(sampler=swz.MIN_DISTANCE_FAST, max_points_per_node=max_points, spacing_at_root=spacing, **kw)


def _gpu_tiler(ctx, bounds, parts, params):
    import torch
    import schwarzwald_amd as swz
    with swz.Tiler(ctx, bounds[0], bounds[1], params) as t:
        for p in parts:
            d = torch.from_numpy(np.ascontiguousarray(p)).cuda()
            torch.cuda.synchronize()
            t.add_batch_device(d.data_ptr(), p.shape[0])
        t.finalize()
        info, table = t.info(), t.node_table()
        ns = int(info["num_stored"])
        d_ids = torch.empty(max(ns, 1), dtype=torch.int32, device="cuda")
        t.export_device(None, d_ids.data_ptr(), None)
        return info, table, d_ids.cpu().numpy().view(np.uint32)[:ns]


# (the families of MULTI_LEFT_OUT have no multi-batch legs: see the file's docstring)
MATRIX = [(name, leg) for name in ALL for leg in LEGS if not (leg.startswith("multi-batch") and name in MULTI_LEFT_OUT)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,leg", MATRIX)
def test_md_fast_adversarial_family_matches_reference(ctx, name, leg):
    xyz, bounds, cases = cloud(name)
    for case, (sp, mppn) in enumerate(cases):
        what = "%s, spacing %r, max_points %d, %s" % (name, sp, mppn, leg)
        if leg in SINGLE_LEGS:
            r = _ref(name, case)
            g = _with(ctx, SINGLE_LEGS[leg], lambda: ctx.tile(xyz, *bounds, _params(mppn, sp)))
            assert np.array_equal(g.keys, r["keys"]) and np.array_equal(g.perm, r["perm"]), what
            assert np.array_equal(g.level, r["level"]), what + ": " + _first_difference(g.level, r["level"])
            if leg == "default":
                assert g.stats["num_nodes"] == r["num_nodes"] and g.stats["points_visited"] == r["points_visited"], what
        elif leg.startswith("FAST"):
            conc = int(leg.split()[1])
            r = _ref(name, case, O.FAST, conc)
            g = ctx.tile(xyz, *bounds, _params(mppn, sp, strategy=O.FAST, fast_concurrency=conc))
            assert g.stats["fast_start_levels"] == r["fast_start_level"], what
            assert np.array_equal(g.perm, r["perm"]), what
            assert np.array_equal(g.level, r["level"]), what + ": " + _first_difference(g.level, r["level"])
            assert np.array_equal(g.dup, r["dup"]), what + ": " + _first_difference(g.dup, r["dup"])
        elif leg == "sample_points":
            r = _ref(name, case)
            for node_level in (0, 1):  # stride 2 and stride 1, with a node key that is not the root's
                key, pos = max(_nodes(r, node_level), key=lambda node: len(node[1]))
                k, i = r["keys"][pos], r["perm"][pos]
                for behaviour in (O.TAKE_ALL_WHEN_BELOW_MAX, O.ALWAYS_ADHERE):
                    expect = R.sample_points(mppn, k, i, r["xyz_clamped"], key, node_level, *bounds, sp, behaviour)
                    got = ctx.sample_points(FAST4, mppn, k, i, r["xyz_clamped"], key, node_level, *bounds, sp, behaviour)
                    assert np.array_equal(got, expect), "%s: level %d node %x (%d points), behaviour %d: %s" % (
                        what, node_level, key, len(pos), behaviour, _first_difference(got, expect))
        else:
            strategy = O.FAST if leg.endswith("FAST") else O.ACCURATE
            m = _multi_ref(name, case, strategy)
            assert m["unsorted"] == 0, what
            info, table, ids = _gpu_tiler(ctx, bounds, _parts(name), _params(mppn, sp, strategy=strategy, fast_concurrency=CONCURRENCY))
            assert info["rekey_inversions"] == 0, what
            if strategy == O.FAST:
                assert info["fast_start_levels"] == m["start_level"], what
            _compare_tables(table, ids, m["table"])
