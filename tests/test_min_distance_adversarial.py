"""Exact MIN_DISTANCE on the data that real point clouds are made of and random doubles never produce: lattices whose pairs sit
exactly at a level's spacing (ties, decided by the reference's strict '<' on the float-squared spacing), LAS records quantised
to a millimetre at UTM offsets, stacks of hundreds of duplicates, and a point with hundreds of earlier neighbours in the LDS
block path.  Every decision path -- key sweep, position sweep, LDS blocks, thread-per-point, FAST reconstruction, the
incremental subset of the multi-batch tiler -- must give the oracle's set point for point (property mode: its properties).

The CPU tests at the top check that each generator really produces its hard case, so that a later change to a generator
cannot quietly remove it."""
import functools

import numpy as np
import pytest

import oracle_lib as O

# ----------------------------------------------------------------------------------------------------------- data families
LATTICE = ([0.0, 0.0, 0.0], [256.0, 256.0, 256.0])
FINE_LATTICE_LO = np.array([0.5, 0.25, 0.125])
FINE_LATTICE = (FINE_LATTICE_LO.tolist(), (FINE_LATTICE_LO + 0.256).tolist())
LAS_OFFSET = np.array([500000.0, 5400000.0, 200.0])
UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


def _integer_lattice(seed):
    """A full lattice block of pitch 1 against the upper faces of [0, 256]^3 (coordinate 256 clamps to key 2^21 - 1) and
    scattered lattice points everywhere else."""
    rng = np.random.default_rng(seed)
    g = np.arange(193, 257, dtype=np.float64)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    scatter = rng.integers(0, 257, size=(30000, 3)).astype(np.float64)
    xyz = np.vstack([block, scatter])
    return xyz[rng.permutation(xyz.shape[0])]


def _fine_lattice(seed):
    """The same at pitch 0.001 and offset (0.5, 0.25, 0.125): integer * 0.001 + offset, as LAS decoding computes it."""
    return FINE_LATTICE_LO + _integer_lattice(seed) * 0.001


def _las_records(seed, n=250000):
    """LAS-style integer records (mm) of a surface: sloped ground, two walls, a roof and tree blobs, 200 m x 150 m x 25 m."""
    rng = np.random.default_rng(seed)
    k = n // 5
    x, y = rng.integers(0, 200000, k), rng.integers(0, 150000, k)
    ground = np.column_stack([x, y, 1000 + x // 50 + rng.integers(-30, 31, k)])
    wall1 = np.column_stack([rng.integers(60000, 90000, k // 2), np.full(k // 2, 40000), rng.integers(2000, 14000, k // 2)])
    wall2 = np.column_stack([np.full(k // 2, 60000), rng.integers(40000, 70000, k // 2), rng.integers(2000, 14000, k // 2)])
    roof = np.column_stack([rng.integers(60000, 90000, k), rng.integers(40000, 70000, k), np.full(k, 14000)])
    centres = rng.integers([10000, 10000, 5000], [190000, 140000, 20000], size=(40, 3))
    m = n - 3 * k
    trees = centres[rng.integers(0, 40, m)] + np.rint(1500 * rng.standard_normal((m, 3))).astype(np.int64)
    rec = np.vstack([ground, wall1, wall2, roof, trees])
    rec = rec[rng.permutation(rec.shape[0])]
    return rec


def _las_cloud(seed):
    return _las_records(seed).astype(np.float64) * 0.001 + LAS_OFFSET


def _cubic_bounds(xyz):
    lo = xyz.min(axis=0)
    return lo.tolist(), (lo + (xyz.max(axis=0) - lo).max()).tolist()


def _aabb(xyz):
    return xyz.min(axis=0).tolist(), xyz.max(axis=0).tolist()


STACK_POSITIONS = 1200


def _duplicate_stacks(seed):
    """STACK_POSITIONS positions, each repeated 1 to 400 times, shuffled into a uniform background."""
    rng = np.random.default_rng(seed)
    pos = rng.random((STACK_POSITIONS, 3))
    reps = rng.integers(1, 401, STACK_POSITIONS)
    reps[:10] = 400  # (the largest stack is always there)
    stacks = np.repeat(pos, reps, axis=0)
    xyz = np.vstack([stacks, rng.random((40000, 3))])
    return xyz[rng.permutation(xyz.shape[0])], reps


# Family d: one point J of a block of the LDS path with hundreds of earlier neighbours, the point behind it (J1) alone with J in
# the block and without any candidate.  Root level, unit bounds, spacing = diagonal / 250 (cells of 1/128: 7 cell levels, blocks
# of 1/16); the background fills the upper half of the box densely enough (> 128 points per occupied block) that the block path
# keeps its finest cells.  J sits just above the block face x = 1/2 (a block face for every cell level from 4 on), a clump of
# CLUMP points just below it: a block earlier in Morton order, within J's spacing.  J1 sits five cells further on, past J in
# every coordinate (later in Morton order), with nothing in the 27 cells around it.
CLUMP_D = 250
CLUMP = 330
SB_PEND = 63          # swz_mdblock.hip: in-band pairs a wavefront puts aside
SB_CNT_SAT_OLD = 200  # ... and where the search used to saturate its count before the fix


def _crowded_block(seed):
    rng = np.random.default_rng(seed)
    s = O.spacing_from_diagonal(*UNIT, CLUMP_D)
    j = np.array([0.5 + 0.2 * s, 0.3, 0.3])
    j1 = np.array([0.54, 0.31, 0.31])
    u = rng.standard_normal((CLUMP, 3))
    u *= (0.2 * s * rng.random(CLUMP) ** (1.0 / 3.0) / np.linalg.norm(u, axis=1))[:, None]
    clump = np.array([0.5 - 0.3 * s, 0.3, 0.3]) + u
    back = rng.random((280000, 3)) * np.array([1.0, 1.0, 0.5]) + np.array([0.0, 0.0, 0.5])
    xyz = np.vstack([back, clump, j, j1])
    perm = rng.permutation(xyz.shape[0])
    xyz = xyz[perm]
    inv = np.argsort(perm)
    return xyz, int(inv[-2]), int(inv[-1])  # (the input indices of J and J1)


@functools.lru_cache(maxsize=None)
def family(name):
    """name -> (xyz, bounds, [(spacing_at_root, max_points_per_node), ...])"""
    if name == "lattice":
        # powers of two reach the pitch exactly; float32(sqrt 3) squares to exactly 3 in float: ties by rounding
        return _integer_lattice(1), LATTICE, [(32.0, 500), (16.0 * float(np.float32(np.sqrt(3.0))), 500)]
    if name == "lattice-0.001":
        return _fine_lattice(2), FINE_LATTICE, [(float(np.float32(0.032)), 500)]
    if name in ("las-cubic", "las-aabb"):
        xyz = _las_cloud(3)
        bounds = _cubic_bounds(xyz) if name == "las-cubic" else _aabb(xyz)
        return xyz, bounds, [(O.spacing_from_diagonal(*bounds, 250), 2000), (O.spacing_from_diagonal(*bounds, 90), 500)]
    if name == "stacks":
        return _duplicate_stacks(4)[0], UNIT, [(O.spacing_from_diagonal(*UNIT, 250), 300)]
    if name == "crowded-block":
        return _crowded_block(5)[0], UNIT, [(O.spacing_from_diagonal(*UNIT, CLUMP_D), 20000)]
    raise KeyError(name)


FAMILIES = ["lattice", "lattice-0.001", "las-cubic", "las-aabb", "stacks", "crowded-block"]


def _level_spacing(spacing_at_root, L):
    """The reference's per-level spacing and its float square widened to double (Sampling.h:448-449, SparseGrid.cpp:13)."""
    s = np.float32(spacing_at_root) / np.float32(2.0 ** (L + 1))
    return float(s), float(np.float32(s) * np.float32(s))


def _sq_dist(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _node_pairs_at(o, spacing_at_root, L, radius_scale=1.0 + 1e-6):
    """Pairs (i, j) of sorted positions, both active at level L and in the same node, within the level's spacing (a little
    more), with their squared distances as the reference computes them."""
    from scipy.spatial import cKDTree
    s, sq = _level_spacing(spacing_at_root, L)
    keys, level, pos = o["keys"], o["level"], o["xyz_clamped"][o["perm"]]
    idx = np.flatnonzero(level >= L)
    shift = 63 - 3 * (L + 1)
    node = (keys >> np.uint64(shift)) if shift < 63 else np.zeros_like(keys)
    pairs = cKDTree(pos[idx]).query_pairs(s * radius_scale, output_type="ndarray")
    a, b = idx[pairs[:, 0]], idx[pairs[:, 1]]
    same = node[a] == node[b]
    a, b = a[same], b[same]
    return a, b, _sq_dist(pos[a], pos[b]), sq


@functools.lru_cache(maxsize=None)
def _oracle(name, case, strategy=O.ACCURATE, concurrency=8):
    xyz, bounds, cases = family(name)
    sp, mppn = cases[case]
    o = O.tile(xyz, *bounds, O.MIN_DISTANCE, mppn, sp, strategy=strategy, fast_concurrency=concurrency)
    assert o["status"] == 0
    return o


# --------------------------------------------------------------------------------------------------------- CPU: premises
def test_lattice_has_exact_ties():
    """Family a: at the levels whose spacing is the lattice pitch (1, and the float sqrt(3) whose square rounds to 3), many
    pairs of one sampled node are exactly at the spacing: d^2 == float(s^2)."""
    ties = {}
    for case, L in ((0, 4), (1, 3)):
        o = _oracle("lattice", case)
        _, _, d2, sq = _node_pairs_at(o, family("lattice")[2][case][0], L)
        ties[(case, L)] = int((d2 == sq).sum())
    print("exact ties (case, level) -> pairs:", ties)
    assert ties[(0, 4)] > 10000      # pitch-1 neighbours at level 4 (spacing 1)
    assert ties[(1, 3)] > 1000       # cube diagonals sqrt(3) at level 3: float32(sqrt 3)^2 rounds to exactly 3
    # the lattice reaches the upper faces: coordinate 256 is clamped to the last key cell
    assert (family("lattice")[0] == 256.0).any()


def test_fine_lattice_has_near_ties():
    """Family a at pitch 0.001: the level-4 spacing (float 0.032 / 32) is within 1e-6 of the lattice pitch, so every pair of
    neighbours lies deep inside any quantisation band and only the exact compare can decide it."""
    o = _oracle("lattice-0.001", 0)
    _, _, d2, sq = _node_pairs_at(o, family("lattice-0.001")[2][0][0], 4)
    near = np.abs(d2 / sq - 1.0) < 1e-6
    print("pitch-0.001 lattice, level 4: %d pairs within 1e-6 of the spacing, %d exact ties" % (int(near.sum()), int((d2 == sq).sum())))
    assert near.sum() > 10000


def test_las_cloud_is_quantised_at_utm_offsets():
    rec = _las_records(3)
    xyz = _las_cloud(3)
    assert xyz.shape[0] <= 300000
    assert np.array_equal(np.rint((xyz - LAS_OFFSET) / 0.001).astype(np.int64), rec)
    assert xyz[:, 0].min() >= 5e5 and xyz[:, 1].min() >= 5.4e6
    lo, hi = _aabb(xyz)
    assert len({round(h - l, 3) for l, h in zip(lo, hi)}) == 3  # the AABB is not cubic: it takes the position sweep
    assert np.unique(rec, axis=0).shape[0] < rec.shape[0]  # quantisation yields duplicates


def test_duplicate_stacks_exceed_a_node():
    """Family c: stacks bigger than max_points_per_node, and points with hundreds of earlier neighbours at distance 0."""
    xyz, reps = _duplicate_stacks(4)
    mppn = family("stacks")[2][0][1]
    assert xyz.shape[0] <= 300000 and reps.max() == 400 and (reps > mppn).sum() >= 10
    _, counts = np.unique(xyz, axis=0, return_counts=True)
    assert counts.max() == 400 and (counts > mppn).sum() == (reps > mppn).sum()


def test_crowded_block_premise():
    """Family d: at the root (every point active), J has >= 200 + SB_PEND exact-near earlier points of its node, so the
    search saturates its count and the pending pairs push it past a byte; J and J1 are alone in their block at every cell
    level from 4 to 7, J1 shares J's counter word and has no point at all in the 27 cells around it, and the default cell
    choice keeps 7 cell levels."""
    xyz, ij, ij1 = _crowded_block(5)
    assert xyz.shape[0] <= 300000
    keys, clamped = O.index_points(xyz, *UNIT)
    order = np.argsort(keys, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    s, sq = _level_spacing(O.spacing_from_diagonal(*UNIT, CLUMP_D), -1)
    d2 = _sq_dist(clamped, clamped[ij])
    earlier = rank < rank[ij]
    n_near = int(((d2 < sq) & earlier).sum())
    print("J: %d exact-near earlier points at the root (needs %d)" % (n_near, SB_CNT_SAT_OLD + SB_PEND))
    assert n_near >= SB_CNT_SAT_OLD + SB_PEND
    assert rank[ij1] == rank[ij] + 1
    assert int((_sq_dist(clamped, clamped[ij1]) < sq).sum()) == 1  # (itself)
    for cl in range(4, 8):
        block = keys >> np.uint64(63 - 3 * (cl - 3))
        members = np.flatnonzero(block == block[ij])
        assert sorted(members.tolist()) == sorted([ij, ij1]), cl
    # J is the block's own point 0 (its byte 0 of counter word 0), J1 point 1 of the same word
    cell = np.floor(clamped * 128.0).astype(np.int64)
    around = np.all(np.abs(cell - cell[ij1]) <= 1, axis=1)
    assert int(around.sum()) == 1
    # the cell choice of the block path (sb_run): 7 cell levels while a block holds 128 points or more on average
    s_root = O.spacing_from_diagonal(*UNIT, CLUMP_D)
    assert 1.0 / 128.0 >= s_root * (1.0 + 2.0 ** -20) and 1.0 / 256.0 < s_root
    assert xyz.shape[0] / np.unique(keys >> np.uint64(63 - 12)).size >= 128.0


# ----------------------------------------------------------------------------------------------------------- GPU: the matrix
@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _options_cleared(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        for k in ("SWZ_MD_KEYS", "SWZ_MD_SPARSE_LIMIT", "SWZ_SP_BLOCK", "SWZ_SP_BLOCK_WIDE", "SWZ_SP_FILTER_EPS",
                  "SWZ_SP_BLOCK_CAP_SCALE", "SWZ_SP_INCREMENTAL", "SWZ_SP_INCREMENTAL_MAX", "SWZ_DEBUG"):
            c.set_option(k, None)


SINGLE = {
    "default": {},
    "key sweep on every level": {"SWZ_MD_SPARSE_LIMIT": "0"},
    "position sweep": {"SWZ_MD_KEYS": "0"},
    "position sweep on every level": {"SWZ_MD_KEYS": "0", "SWZ_MD_SPARSE_LIMIT": "0"},
    "block path on every level": {"SWZ_MD_SPARSE_LIMIT": "1000"},
    "thread-per-point": {"SWZ_MD_SPARSE_LIMIT": "1000", "SWZ_SP_BLOCK": "0"},
    "wide block records": {"SWZ_MD_SPARSE_LIMIT": "1000", "SWZ_SP_BLOCK_WIDE": "1"},
    "every compare exact": {"SWZ_MD_SPARSE_LIMIT": "1000", "SWZ_SP_FILTER_EPS": "1e30"},
}
LEGS = list(SINGLE) + ["FAST 2", "FAST 8", "multi-batch ACCURATE", "multi-batch FAST", "property"]


def _with(ctx, options, fn):
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        return fn()
    finally:
        for k in options:
            ctx.set_option(k, None)


def _first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return "%d points differ, first at sorted position %d: %d, oracle %d" % (bad.size, bad[0], got[bad[0]], want[bad[0]]) if bad.size else ""


@pytest.mark.gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", FAMILIES)
def test_adversarial_family_matches_oracle(ctx, name, leg):
    import schwarzwald_amd as swz
    xyz, bounds, cases = family(name)
    for case, (sp, mppn) in enumerate(cases):
        what = "%s, spacing %r, max_points %d, %s" % (name, sp, mppn, leg)
        if leg in SINGLE:
            o = _oracle(name, case)
            p = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=mppn, spacing_at_root=sp)
            g = _with(ctx, SINGLE[leg], lambda: ctx.tile(xyz, *bounds, p))
            assert np.array_equal(g.keys, o["keys"]) and np.array_equal(g.perm, o["perm"]), what
            assert np.array_equal(g.level, o["level"]), what + ": " + _first_difference(g.level, o["level"])
        elif leg.startswith("FAST"):
            conc = int(leg.split()[1])
            o = _oracle(name, case, O.FAST, conc)
            p = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=mppn, spacing_at_root=sp, strategy=swz.FAST,
                               fast_concurrency=conc)
            g = ctx.tile(xyz, *bounds, p)
            assert np.array_equal(g.perm, o["perm"]), what
            assert np.array_equal(g.level, o["level"]), what + ": " + _first_difference(g.level, o["level"])
            assert np.array_equal(g.dup, o["dup"]), what
        elif leg.startswith("multi-batch"):
            from test_multibatch import _compare, _gpu_files, _oracle_files
            strategy = O.FAST if leg.endswith("FAST") else O.ACCURATE
            ex, c = _oracle_files(bounds, xyz, 3, O.MIN_DISTANCE, mppn, sp, strategy, 2)
            g = _gpu_files(ctx, bounds, xyz, 3, O.MIN_DISTANCE, mppn, sp, strategy, 2, staged=False)
            inversions = int(g["info"]["rekey_inversions"]), int(c["unsorted_cached_nodes"])
            print("%s: rekey inversions %d, oracle's unsorted cached nodes %d" % ((what,) + inversions))
            if inversions == (0, 0):
                _compare(g, ex, c)
            else:
                # quantised positions on key-cell boundaries: a node that re-reads its points against its own bounds may
                # order them differently from the root's keys, where the library sorts and the reference merges unsorted
                # (the documented divergence, see test_multibatch.py::test_gpu_rekey_inversion_is_counted_and_confined):
                # both must see it, and every point is still stored (ACCURATE: exactly once; FAST, whose copies depend on
                # the decisions: at least once)
                assert min(inversions) > 0, what
                if strategy == O.ACCURATE:
                    assert g["ids"].size == c["num_stored"] == xyz.shape[0], what
                ids = np.sort(g["ids"]) if strategy == O.ACCURATE else np.unique(g["ids"])
                assert np.array_equal(ids, np.arange(xyz.shape[0], dtype=np.uint32)), what
        else:
            from test_min_distance_property import _check_property
            p = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=mppn, spacing_at_root=sp,
                               flags=swz.FLAG_MIN_DISTANCE_PROPERTY)
            r = ctx.tile(xyz, *bounds, p)
            o = _oracle(name, case)
            assert np.array_equal(r.keys, o["keys"]) and np.array_equal(r.perm, o["perm"]), what
            a, b = _check_property(r.keys, r.level, r.xyz_clamped[r.perm], sp, mppn, _property_levels(name, r))
            assert a > 0 and b > 0, what


def _property_levels(name, r):
    # (stacks of duplicates reach the deepest key level, where a node keeps whatever it holds: the properties hold above it)
    return r.stats["max_level"] - 1 if name == "stacks" else r.stats["max_level"]


@pytest.mark.gpu
def test_crowded_block_reaches_the_block_path(ctx, capfd):
    """Family d runs its root on the block path with 7 cell levels (the geometry the CPU premise is built on), with every
    pair in reach on the exact compare: the pending list of J's wavefront fills with J's pairs alone."""
    import schwarzwald_amd as swz
    xyz, bounds, cases = family("crowded-block")
    sp, mppn = cases[0]
    o = _oracle("crowded-block", 0)
    p = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=mppn, spacing_at_root=sp)
    opts = {"SWZ_MD_SPARSE_LIMIT": "1000", "SWZ_SP_FILTER_EPS": "1e30", "SWZ_DEBUG": "1"}
    capfd.readouterr()
    g = _with(ctx, opts, lambda: ctx.tile(xyz, *bounds, p))
    err = capfd.readouterr().err
    assert np.array_equal(g.level, o["level"]), _first_difference(g.level, o["level"])
    root = [line for line in err.splitlines() if "MIN_DISTANCE level -1 block path" in line]
    assert root and "cell_levels 7" in root[-1], err[-2000:]


# ------------------------------------------------------------------------------------------- GPU: bytes charged by the block path
def _md_bytes(ctx, fn):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        fn()
        return ctx.profile_get()["sample_min_distance"]["algorithmic_bytes"]
    finally:
        ctx.profile_enable(False)


@pytest.mark.gpu
def test_block_path_charges_a_level_once_single_batch(ctx):
    """The roofline bytes of sample_min_distance are the algorithm's: repeated launches of a level (capacities estimated too
    small) read the same points again but do not charge them again."""
    import schwarzwald_amd as swz
    rng = np.random.default_rng(11)
    xyz = rng.random((300000, 3))  # (uniform: without the option no level needs a second launch)
    sp = O.spacing_from_diagonal(*UNIT, 250)
    p = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=2000, spacing_at_root=sp)
    base = {"SWZ_MD_SPARSE_LIMIT": "1000"}
    once = _with(ctx, base, lambda: _md_bytes(ctx, lambda: ctx.tile(xyz, *UNIT, p)))
    again = _with(ctx, dict(base, SWZ_SP_BLOCK_CAP_SCALE="0.3"), lambda: _md_bytes(ctx, lambda: ctx.tile(xyz, *UNIT, p)))
    assert once > 0
    assert again == once, (once, again)


@pytest.mark.gpu
@pytest.mark.parametrize("incremental", [False, True])
def test_block_path_charges_a_level_once_multi_batch(ctx, incremental):
    """The same for a MIN_DISTANCE tiler of three batches, with the incremental subset forced on (its pack pass and the
    block path must not both charge the selected points) and off."""
    from test_multibatch import _gpu_files, _points
    rng = np.random.default_rng(900)
    xyz = _points(rng, 300000, UNIT, clustered=False)
    sp = O.spacing_from_diagonal(*UNIT, 128)
    base = {"SWZ_MD_SPARSE_LIMIT": "1000"}
    if incremental:
        base.update({"SWZ_SP_INCREMENTAL": "0.001", "SWZ_SP_INCREMENTAL_MAX": "1.0"})
    else:
        base["SWZ_SP_INCREMENTAL"] = "0"

    def run():
        return _gpu_files(ctx, UNIT, xyz, 3, O.MIN_DISTANCE, 1000, sp, O.ACCURATE, 2, staged=False)
    once = _with(ctx, base, lambda: _md_bytes(ctx, run))
    again = _with(ctx, dict(base, SWZ_SP_BLOCK_CAP_SCALE="0.3"), lambda: _md_bytes(ctx, run))
    assert once > 0
    assert again == once, (once, again)
