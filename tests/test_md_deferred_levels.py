"""Chains of dense exact-MIN_DISTANCE levels on one active set (swz_session.hip: a level whose survivors stay where they are,
the next level on the same arrays with the taken bytes as ActiveSet::gone, one compaction that ends the chain).

Every case tiles the same cloud with SWZ_MD_DEFER=0 -- every level compacts, the code path of all other callers -- and with the
default, and asks for the same keys, permutation, levels and statistics, bit for bit, and for the oracle's.  The profile's
launch counts say whether the default run really left compactions out: a case that fell back to compacting fails.

The CPU tests check on the oracle that the constructed clouds hold the cases they are named after."""
import functools

import numpy as np
import pytest

import oracle_lib as O

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
MAX_POINTS = 2000
SPACING = O.spacing_from_diagonal(*UNIT, 12)   # root cells 1/4 wide, thousands of points each: root, level 0 and level 1 are dense
STATS = ("num_nodes", "points_visited", "max_level", "fast_start_levels", "num_levels", "min_distance_rounds")


def _uniform(seed=11, n=300007):
    """Odd, no multiple of 4 or of the 512-point tiles of the live counts."""
    return np.random.default_rng(seed).random((n, 3))


def _special(seed=12):
    """Six octants of uniform points, and two that the live counts must get right:
    octant 0 (x, y, z < 1/2) holds two points far apart, first in Morton order: the root takes both, no node at level 0;
    octant 7 holds MAX_POINTS + 3 points: the root takes some of them, so the node keeps all the rest at level 0."""
    rng = np.random.default_rng(seed)
    parts = [np.array([[0.1, 0.1, 0.1], [0.4, 0.4, 0.4]])]
    for o in range(1, 7):
        corner = np.array([(o >> 2) & 1, (o >> 1) & 1, o & 1]) * 0.5
        parts.append(corner + 0.5 * rng.random((45000, 3)))
    parts.append(0.5 + 0.5 * rng.random((MAX_POINTS + 3, 3)))
    xyz = np.vstack(parts)
    return xyz[rng.permutation(xyz.shape[0])]


def _stacks_on_lattice(seed=13):
    """200 k points: a lattice of pitch 1/64 with repeats (pairs exactly at the spacing of every level down to the pitch: ties
    and pairs inside the key band), stacks of up to 200 copies of one position, a uniform background."""
    rng = np.random.default_rng(seed)
    lattice = rng.integers(0, 65, size=(120000, 3)).astype(np.float64) / 64.0
    pos = rng.random((400, 3))
    reps = rng.integers(1, 201, 400)
    reps[:5] = 200
    stacks = np.repeat(pos, reps, axis=0)
    xyz = np.vstack([lattice, stacks, rng.random((200000 - lattice.shape[0] - stacks.shape[0], 3))])
    return xyz[rng.permutation(xyz.shape[0])]


@functools.lru_cache(maxsize=None)
def cloud(name):
    """name -> (xyz, spacing_at_root)"""
    if name == "uniform":
        return _uniform(), SPACING
    if name == "special":
        return _special(), SPACING
    if name == "stacks-lattice":
        return _stacks_on_lattice(), 0.25   # level spacings 1/4, 1/8, ... 1/64: the lattice's pitch and its multiples
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle(name):
    xyz, spacing = cloud(name)
    o = O.tile(xyz, *UNIT, O.MIN_DISTANCE, MAX_POINTS, spacing)
    assert o["status"] == 0
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


def _taken_share(o, level):
    """share of the points taken at `level` or above"""
    return float(np.count_nonzero(o["level"] <= level)) / o["level"].size


# ----------------------------------------------------------------------------------------------------------- CPU: the premises
def test_uniform_cloud_keeps_three_sampled_levels_below_the_default_bound():
    o = oracle("uniform")
    n = o["level"].size
    assert n % 2 == 1 and n % 512 != 0
    # root, level 0 and level 1 are sampled and together stay below 1/8 of the array: all three leave their survivors in
    # place.  At level 2 every node keeps what it holds: that level runs on the shared arrays as well, and its compaction
    # writes the codes of four levels.
    assert 0 < _taken_share(o, -1) < _taken_share(o, 0) < _taken_share(o, 1) < 0.125
    assert o["stats"]["max_level"] == 2


def test_special_cloud_holds_a_vanishing_node_and_a_node_that_live_counts_make_take_all():
    xyz, _ = cloud("special")
    o = oracle("special")
    octant = (o["keys"] >> np.uint64(60)).astype(np.int64)
    assert np.count_nonzero(octant == 0) == 2
    assert np.all(o["level"][octant == 0] == -1)              # no point left for the node at level 0
    lv7 = o["level"][octant == 7]
    assert lv7.size == MAX_POINTS + 3
    assert np.count_nonzero(lv7 == -1) >= 3                   # ... so the node holds at most MAX_POINTS open points
    assert np.all(lv7 <= 0) and np.count_nonzero(lv7 == 0) > 0  # and keeps them all
    for oc in range(1, 7):                                    # (the others are sampled: the level is dense all the same)
        assert o["level"][octant == oc].max() >= 1


def test_stacks_on_lattice_have_ties_and_dead_stretches():
    xyz, spacing = cloud("stacks-lattice")
    assert xyz.shape[0] == 200000
    o = oracle("stacks-lattice")
    assert _taken_share(o, -1) < 0.125
    # whole runs of equal keys (a stack) with one point taken early and the rest left for the deepest levels
    k = o["keys"]
    run = np.flatnonzero(np.diff(k) == 0)
    assert run.size > 30000
    assert 0 < _taken_share(o, -1) < _taken_share(o, 0) < _taken_share(o, 1) < 0.125


# ----------------------------------------------------------------------------------------------------------- GPU
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
        for k in ("SWZ_MD_DEFER", "SWZ_MD_DEFER_MAX_GONE"):
            c.set_option(k, None)
        c.profile_enable(False)


def _run(ctx, name, options):
    """tile_device on a fresh copy of the cloud -> (keys, perm, level, stats, compactions, live-count passes)"""
    import torch
    import schwarzwald_amd as swz
    xyz, spacing = cloud(name)
    n = xyz.shape[0]
    dev = torch.device("cuda:0")
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    d_xyz = torch.from_numpy(xyz).to(dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    level = torch.empty(n, dtype=torch.int8, device=dev)
    params = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=MAX_POINTS, spacing_at_root=spacing)
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.profile_enable(True)
        ctx.profile_reset()
        stats = ctx.tile_device(d_xyz.data_ptr(), n, *UNIT, params, keys.data_ptr(), perm.data_ptr(), level.data_ptr())
        torch.cuda.synchronize()
        prof = ctx.profile_get()
    finally:
        ctx.profile_enable(False)
        for k in options:
            ctx.set_option(k, None)
    compactions = prof.get("level_compact", {}).get("launches", 0) // 2   # (two launches each: tile sums, apply)
    counts = prof.get("level_live_count", {}).get("launches", 0)
    return (keys.cpu().numpy().view(np.uint64), perm.cpu().numpy().view(np.uint32), level.cpu().numpy(), stats, compactions, counts)


def _check(ctx, name, options=None, skipped=None):
    """The deferred run against SWZ_MD_DEFER=0 and the oracle; returns the number of compactions it left out."""
    o = oracle(name)
    ref = _run(ctx, name, {"SWZ_MD_DEFER": "0"})
    got = _run(ctx, name, dict(options or {}))
    print("%s %r: stats without chains %r, with %r; compactions %d -> %d, live-count passes %d -> %d" % (
        name, options, ref[3], got[3], ref[4], got[4], ref[5], got[5]))
    for what, a, b, c in (("keys", got[0], ref[0], o["keys"]), ("perm", got[1], ref[1], o["perm"]), ("level", got[2], ref[2], o["level"])):
        assert np.array_equal(b, c), "%s: %s without chains differs from the oracle" % (name, what)
        assert np.array_equal(a, b), "%s: %s differs, first at %d" % (name, what, int(np.flatnonzero(a != b)[0]))
    for k in STATS:
        assert got[3][k] == ref[3][k], (name, k, got[3], ref[3])
    for k in ("num_nodes", "points_visited", "max_level"):
        assert got[3][k] == o["stats"][k], (name, k, got[3], o["stats"])
    assert ref[5] == 0 and ref[4] == ref[3]["num_levels"]          # SWZ_MD_DEFER=0: every level compacts, nobody counts
    left_out = ref[4] - got[4]
    assert left_out >= 1, "%s: the default run compacted after every level" % name
    if skipped is not None:
        assert left_out == skipped, (name, left_out, skipped)
    return left_out


@pytest.mark.gpu
def test_three_level_chain_is_flushed_by_one_compaction(ctx):
    """Root, level 0 and level 1 are sampled on the sorted keys themselves (odd length, a last tile of 487 points) and none
    compacts; level 2, whose nodes all keep their points, takes them on the same arrays, and its compaction -- the only one of
    the call -- writes the levels -1, 0, 1 and 2."""
    assert _check(ctx, "uniform", skipped=3) == 3


@pytest.mark.gpu
def test_live_count_decides_the_node_mode_and_an_emptied_node_does_not_exist(ctx):
    """Octant 7 holds MAX_POINTS + 3 points of which the root takes at least 3: at level 0 the node counts its OPEN points and
    keeps them all.  Octant 0 holds two points, both taken by the root: no node, num_nodes as with SWZ_MD_DEFER=0 (and as the
    oracle's, which _check compares)."""
    _check(ctx, "special")


@pytest.mark.gpu
def test_stacks_and_lattice_ties_with_dead_points_at_cell_edges(ctx):
    _check(ctx, "stacks-lattice")


@pytest.mark.gpu
def test_bound_exceeded_at_level_0_ends_the_chain_after_one_level(ctx):
    o = oracle("uniform")
    bound = 0.5 * (_taken_share(o, -1) + _taken_share(o, 0))   # the root stays below it, level 0 does not
    _check(ctx, "uniform", {"SWZ_MD_DEFER_MAX_GONE": repr(bound)}, skipped=1)


@pytest.mark.gpu
def test_the_same_call_twice_gives_identical_bytes(ctx):
    a = _run(ctx, "stacks-lattice", {})
    b = _run(ctx, "stacks-lattice", {})
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert {k: a[3][k] for k in STATS} == {k: b[3][k] for k in STATS}
    assert a[4] == b[4] < a[3]["num_levels"]
