"""Cell tables built ahead (swz_mqbuild.hip, mq_prebuild_launch): while a dense level of a chain runs its rounds, the early
per-cell tables of the next level are built on a side stream for a GUESSED grid; the next level takes them when the guess was
right and builds everything itself when it was not.

Every case tiles a cloud with SWZ_MD_PREBUILD=0 and with the default and asks for the same keys, permutation, levels and
statistics, bit for bit, and for the oracle's.  The profile's launch counts say which way the default run went:
  mq_tables_ahead      kernels of the early tables on the side stream (two per level built ahead)
  mq_prebuild_taken    levels that found their tables built and ran only the late kernels (mq_tables_late, two per level)
  mq_prebuild_dropped  tables built ahead that no level could use
  mq_tables_at_setup   kernels of a directly numbered level that built all its tables itself (two per level)

The CPU tests check on the oracle that the constructed clouds hold the cases they are named after."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import test_md_deferred_levels as D

UNIT = D.UNIT
COUNTS = ("mq_tables_ahead", "mq_prebuild_taken", "mq_prebuild_dropped", "mq_tables_late", "mq_tables_at_setup")
# bytes of the early per-cell tables with records of 7 (the larger ones): bounds, adjacent cells, two records, slots, stall state
PER_CELL = 8 + 32 * 4 + 2 * 8 * 16 + 32 * 8 + 16


def _cells(xyz, width):
    """ids of the cubic cells of the given width that the points fall into"""
    g = int(round(1.0 / width))
    ijk = np.minimum((xyz * g).astype(np.int64), g - 1)
    return (ijk[:, 0] * g + ijk[:, 1]) * g + ijk[:, 2]


def _two_per_cell_lattice(seed=21):
    """One point in every cell of width 1/64 and a second one in three of four: 1.75 points per cell, spread perfectly evenly.
    Level 1's finest cells are these (spacing = diagonal / 48: root cells 1/16, level 0 1/32, level 1 1/64): with fewer than 2
    points per occupied cell the level is SPARSE -- the block kernel's --, while evenly spread RANDOM points at 1.75 per cell
    would leave every sixth cell empty and come to 2.1 per occupied cell: the guess says dense.
    (Level 0 takes a quarter of such a cloud: the case runs with SWZ_MD_DEFER_MAX_GONE = 1/2, or the chain would end there.)"""
    rng = np.random.default_rng(seed)
    g = 64
    ijk = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), axis=-1).reshape(-1, 3)
    second = ijk[rng.random(ijk.shape[0]) < 0.75]
    cells = np.vstack([ijk, second]).astype(np.float64)
    xyz = (cells + 0.05 + 0.9 * rng.random(cells.shape)) / g
    return xyz[rng.permutation(xyz.shape[0])]


def _thinned_half(seed=22):
    """x < 1/2: exactly 14 points in every cell of width 1/32; x >= 1/2: one point in three of ten such cells.  Level 1's finest
    cells are these (spacing = diagonal / 24).  Per OCCUPIED cell the level holds 11 points -- it keeps the finest cells --,
    per cell of the grid 7.2: evenly spread, the same points would call for cells one level coarser."""
    rng = np.random.default_rng(seed)
    g = 32
    ijk = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), axis=-1).reshape(-1, 3)
    dense = np.repeat(ijk[ijk[:, 0] < g // 2], 14, axis=0)
    thin = ijk[ijk[:, 0] >= g // 2]
    thin = thin[rng.random(thin.shape[0]) < 0.3]
    cells = np.vstack([dense, thin]).astype(np.float64)
    xyz = (cells + rng.random(cells.shape)) / g
    return xyz[rng.permutation(xyz.shape[0])]


@functools.lru_cache(maxsize=None)
def cloud(name):
    """name -> (xyz, spacing_at_root, max_points_per_node)"""
    if name in ("uniform", "special", "stacks-lattice"):
        xyz, spacing = D.cloud(name)
        return xyz, spacing, D.MAX_POINTS
    if name == "sparse-next":
        return _two_per_cell_lattice(), O.spacing_from_diagonal(*UNIT, 48), 50
    if name == "thinned-half":
        return _thinned_half(), O.spacing_from_diagonal(*UNIT, 24), 20
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle(name):
    if name in ("uniform", "special", "stacks-lattice"):
        return D.oracle(name)
    xyz, spacing, max_points = cloud(name)
    o = O.tile(xyz, *UNIT, O.MIN_DISTANCE, max_points, spacing)
    assert o["status"] == 0
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


def _open_at(name, level):
    """positions of the points still open when `level` starts (taken there or deeper), in the oracle's order"""
    xyz, _, _ = cloud(name)
    o = oracle(name)
    return xyz[o["perm"][o["level"] >= level]]


# ----------------------------------------------------------------------------------------------------------- CPU: the premises
def test_special_cloud_has_a_take_all_node_and_a_missing_node_at_level_0():
    xyz, _, max_points = cloud("special")
    o = oracle("special")
    assert xyz.shape[0] / 8.0 > max_points      # evenly spread, every node of level 0 would be sampled: the tables are built
    octant = (o["keys"] >> np.uint64(60)).astype(np.int64)
    open0 = o["level"] >= 0                     # the points that reach level 0
    per_node = np.bincount(octant[open0], minlength=8)
    assert per_node[0] == 0                     # octant 0: both points went to the root, the node does not exist
    assert 0 < per_node[7] <= max_points        # octant 7: a node that keeps all it holds (take-all) ...
    assert np.all(o["level"][(octant == 7) & open0] == 0)
    assert np.all(per_node[1:7] > max_points)   # ... beside six sampled ones: level 0 is not all_sampled, its table not the identity
    assert np.unique((o["keys"][o["level"] >= 1] >> np.uint64(57))).size < 64   # and level 1 has fewer than 64 nodes


def test_sparse_next_cloud_is_sparse_at_level_1_and_dense_by_the_even_estimate():
    xyz, _, max_points = cloud("sparse-next")
    o = oracle("sparse-next")
    assert o["stats"]["max_level"] >= 1
    for level, width in ((-1, 1 / 16), (0, 1 / 32)):       # root and level 0: dense (many points per finest cell), every node sampled
        p = _open_at("sparse-next", level)
        assert p.shape[0] / np.unique(_cells(p, width)).size >= 8.0
        nodes = np.unique(_cells(p, 0.5 ** (level + 1)), return_counts=True)[1]
        assert nodes.size == 8 ** (level + 1) and nodes.min() > max_points
    p = _open_at("sparse-next", 1)
    nodes = np.unique(_cells(p, 1 / 4), return_counts=True)[1]
    assert nodes.size == 64 and nodes.min() > max_points    # every node of level 1 is sampled ...
    occupied = np.unique(_cells(xyz, 1 / 64)).size          # (the survey counts the cells of taken points too)
    assert occupied == 262144 and p.shape[0] / occupied < 2.0  # ... and the level is sparse
    lam = _open_at("sparse-next", 0).shape[0] / 262144.0    # the guess is made while level 0 runs, from the points open then
    assert lam / -np.expm1(-lam) >= 2.0
    assert 0.125 * xyz.shape[0] < np.count_nonzero(o["level"] <= 0) < 0.5 * xyz.shape[0]   # level 0 leaves its survivors in place at 1/2


def test_thinned_half_keeps_fine_cells_at_level_1_where_the_even_estimate_coarsens():
    xyz, _, max_points = cloud("thinned-half")
    assert 10 ** 5 <= xyz.shape[0] <= 10 ** 6
    o = oracle("thinned-half")
    for level, width in ((-1, 1 / 8), (0, 1 / 16)):
        p = _open_at("thinned-half", level)
        nodes = np.unique(_cells(p, 0.5 ** (level + 1)), return_counts=True)[1]
        assert nodes.size == 8 ** (level + 1) and nodes.min() > max_points
        lam = p.shape[0] / float(8 ** (level + 1) * 512)
        assert lam / -np.expm1(-lam) >= 8.0                 # root and level 0: finest cells, by the survey and by the estimate
    p = _open_at("thinned-half", 1)
    nodes = np.unique(_cells(p, 1 / 4), return_counts=True)[1]
    assert nodes.size == 64 and nodes.min() > max_points    # every node of level 1 is sampled: all_sampled, identity node table
    occupied = np.unique(_cells(xyz, 1 / 32)).size
    assert p.shape[0] / occupied >= 8.0                     # the survey: finest cells (cl = 3)
    assert occupied / 32768.0 >= 0.5                        # ... numbered directly
    lam = _open_at("thinned-half", 0).shape[0] / 32768.0
    assert 2.0 <= lam / -np.expm1(-lam) < 8.0               # the estimate: dense, but one level coarser (cl = 2)
    assert np.count_nonzero(o["level"] <= 0) < 0.125 * xyz.shape[0]


# ----------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def _run(ctx, name, options, flags=0):
    """tile_device on a fresh copy of the cloud -> (keys, perm, level, stats, launch counts)"""
    import torch
    import schwarzwald_amd as swz
    xyz, spacing, max_points = cloud(name)
    n = xyz.shape[0]
    dev = torch.device("cuda:0")
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    d_xyz = torch.from_numpy(xyz).to(dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    level = torch.empty(n, dtype=torch.int8, device=dev)
    params = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=max_points, spacing_at_root=spacing, flags=flags)
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
    counts = {k: prof.get(k, {}).get("launches", 0) for k in COUNTS}
    return (keys.cpu().numpy().view(np.uint64), perm.cpu().numpy().view(np.uint32), level.cpu().numpy(), stats, counts)


def _compare(name, got, ref):
    """keys, perm, level and stats of a run against the SWZ_MD_PREBUILD=0 run and the oracle"""
    o = oracle(name)
    for what, a, b, c in (("keys", got[0], ref[0], o["keys"]), ("perm", got[1], ref[1], o["perm"]), ("level", got[2], ref[2], o["level"])):
        assert np.array_equal(b, c), "%s: %s with SWZ_MD_PREBUILD=0 differs from the oracle" % (name, what)
        assert np.array_equal(a, b), "%s: %s differs, first at %d" % (name, what, int(np.flatnonzero(a != b)[0]))
    for k in D.STATS:
        assert got[3][k] == ref[3][k], (name, k, got[3], ref[3])
    for k in ("num_nodes", "points_visited", "max_level"):
        assert got[3][k] == o["stats"][k], (name, k, got[3], o["stats"])
    r, g = ref[4], got[4]
    assert r["mq_tables_ahead"] == r["mq_prebuild_taken"] == r["mq_prebuild_dropped"] == r["mq_tables_late"] == 0, r
    assert g["mq_tables_ahead"] == 2 * (g["mq_prebuild_taken"] + g["mq_prebuild_dropped"]), g   # every product ends one way or the other
    assert g["mq_tables_late"] == 2 * g["mq_prebuild_taken"], g
    assert g["mq_tables_at_setup"] + g["mq_tables_late"] == r["mq_tables_at_setup"], (g, r)   # the same levels, built here or there
    return g


def _check(ctx, name, options=None, ref_ctx=None):
    """The default run against SWZ_MD_PREBUILD=0 (on ref_ctx, if given) and the oracle; returns the default run's launch counts."""
    ref = _run(ref_ctx or ctx, name, dict(options or {}, SWZ_MD_PREBUILD="0"))
    got = _run(ctx, name, dict(options or {}))
    print("%s %r: without %r, with %r" % (name, options, ref[4], got[4]))
    return _compare(name, got, ref)


@pytest.mark.gpu
def test_three_sampled_levels_take_the_tables_built_under_the_level_before(ctx):
    """Root, level 0 and level 1 of the uniform cloud: the tables of levels 0 and 1 are built once each, on the side stream,
    and set-up runs only the late kernels; the root builds its own; nothing is built for level 2, whose nodes keep their points."""
    g = _check(ctx, "uniform")
    assert g == {"mq_tables_ahead": 4, "mq_prebuild_taken": 2, "mq_prebuild_dropped": 0, "mq_tables_late": 4, "mq_tables_at_setup": 2}


@pytest.mark.gpu
def test_a_node_that_live_counts_make_take_all_drops_the_tables(ctx):
    """Octant 7 keeps all its points at level 0, octant 0 holds none: level 0 is not all_sampled, its node table is not the
    identity, and level 1 has fewer than 64 nodes."""
    g = _check(ctx, "special")
    assert g["mq_prebuild_taken"] == 0 and g["mq_prebuild_dropped"] >= 1, g


@pytest.mark.gpu
def test_a_sparse_next_level_goes_to_the_block_kernel_and_drops_the_tables(ctx):
    g = _check(ctx, "sparse-next", {"SWZ_MD_DEFER_MAX_GONE": "0.5"})
    # level 0 takes the root's; what level 0 builds for level 1 is dropped: the level is flushed and sampled by blocks
    assert g["mq_prebuild_taken"] == 1 and g["mq_prebuild_dropped"] >= 1, g


@pytest.mark.gpu
def test_other_cells_at_the_next_level_drop_the_tables(ctx):
    g = _check(ctx, "thinned-half")
    # level 1 is a key-sweep level of the chain with finer cells than were guessed: it builds all its tables itself
    assert g["mq_prebuild_taken"] == 1 and g["mq_prebuild_dropped"] >= 1 and g["mq_tables_at_setup"] >= 4, g


@pytest.mark.gpu
def test_no_second_set_of_buffers_where_the_cell_limit_forbids_it():
    """The uniform cloud's grids hold 64, 512 and 4096 cells.  SWZ_MD_DIRECT_MAX_CELLS=520 admits the root's and level 0's, but
    not the two side by side (576), nor level 0's beside level 1's: nothing is built ahead and the workspace of a fresh context
    is byte for byte as large as with SWZ_MD_PREBUILD=0.  (Level 1's own grid exceeds the limit: the chain ends in front of it.)"""
    import schwarzwald_amd as swz
    with swz.Context(0) as c0, swz.Context(0) as c1:
        g = _check(c1, "uniform", {"SWZ_MD_DIRECT_MAX_CELLS": "520"}, ref_ctx=c0)
        held = (c0.workspace_bytes(), c1.workspace_bytes())
    assert g["mq_tables_ahead"] == 0 and g["mq_prebuild_taken"] == 0 and g["mq_tables_at_setup"] >= 4, g
    assert held[0] == held[1], held


@pytest.mark.gpu
def test_the_cell_limit_admits_the_pair_of_grids_that_fits():
    """SWZ_MD_DIRECT_MAX_CELLS=4096 admits every grid, and the root's and level 0's side by side (576) but not level 0's and
    level 1's (4608): level 0 takes tables built ahead, level 1 builds its own, and the second set holds 512 cells, not 4096."""
    import schwarzwald_amd as swz
    with swz.Context(0) as c0, swz.Context(0) as c1:
        g = _check(c1, "uniform", {"SWZ_MD_DIRECT_MAX_CELLS": "4096"}, ref_ctx=c0)
        held = (c0.workspace_bytes(), c1.workspace_bytes())
    assert g == {"mq_tables_ahead": 2, "mq_prebuild_taken": 1, "mq_prebuild_dropped": 0, "mq_tables_late": 2, "mq_tables_at_setup": 4}
    assert held[1] - held[0] <= 512 * PER_CELL * 17 // 16 + 5 * 512, held   # (with the workspace's head-room of 1/16 and its rounding)


@pytest.mark.gpu
def test_stacks_and_lattice_ties_on_tables_built_ahead(ctx):
    """Stacks of identical points (runs of one key that span tiles of the build) and lattice points on cell faces: the smallest
    shapes at which a wrong run of cell bounds or a stale slot shows."""
    g = _check(ctx, "stacks-lattice")
    assert g["mq_prebuild_taken"] >= 1, g


@pytest.mark.gpu
def test_repeats_on_one_context_and_poisoned_memory_give_identical_bytes(ctx):
    import schwarzwald_amd as swz
    ref = _run(ctx, "stacks-lattice", {"SWZ_MD_PREBUILD": "0"})
    runs = [_run(ctx, "stacks-lattice", {}) for _ in range(3)]
    with swz.Context(0) as fresh:
        fresh.set_option("SWZ_POISON", "205")   # a table read before it is written would read 0xCD
        runs.append(_run(fresh, "stacks-lattice", {}))
    for r in runs:
        g = _compare("stacks-lattice", r, ref)   # against SWZ_MD_PREBUILD=0 and the oracle
        assert g == runs[0][4] and g["mq_prebuild_taken"] >= 1
        for x, y in zip(runs[0][:3], r[:3]):
            assert x.tobytes() == y.tobytes()


@pytest.mark.gpu
def test_property_mode_and_a_two_batch_tiler_never_ask_for_tables_ahead(ctx):
    """Property mode: the same bytes as with SWZ_MD_PREBUILD=0, the oracle's keys and permutation, and the mode's own oracle --
    spacing and maximality on every sampled node (test_min_distance_property.py).  Two batches: the node table of
    SWZ_MD_PREBUILD=0 and the CPU oracle's files."""
    import schwarzwald_amd as swz
    from test_min_distance_property import _check_property
    xyz, spacing, max_points = cloud("uniform")
    o = oracle("uniform")
    ref = _run(ctx, "uniform", {"SWZ_MD_PREBUILD": "0"}, flags=swz.FLAG_MIN_DISTANCE_PROPERTY)
    got = _run(ctx, "uniform", {}, flags=swz.FLAG_MIN_DISTANCE_PROPERTY)
    for k in COUNTS[:4]:
        assert got[4][k] == 0 and ref[4][k] == 0, (got[4], ref[4])
    for a, b in zip(got[:3], ref[:3]):
        assert a.tobytes() == b.tobytes()
    assert {k: got[3][k] for k in D.STATS} == {k: ref[3][k] for k in D.STATS}
    assert np.array_equal(got[0], o["keys"]) and np.array_equal(got[1], o["perm"])
    pairs, rest = _check_property(got[0], got[2], np.clip(xyz, 0.0, 1.0)[got[1]], spacing, max_points, got[3]["max_level"])
    assert pairs > 0 and rest > 0

    params = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=max_points, spacing_at_root=spacing)
    half = xyz.shape[0] // 2
    tables = {}
    for pre in ("0", None):
        ctx.set_option("SWZ_MD_PREBUILD", pre)
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            with swz.Tiler(ctx, *UNIT, params) as t:
                t.add_batch(xyz[:half])
                t.add_batch(xyz[half:])
                t.finalize()
                tables[pre] = t.node_table()
            prof = ctx.profile_get()
        finally:
            ctx.profile_enable(False)
            ctx.set_option("SWZ_MD_PREBUILD", None)
        assert prof.get("sample_min_distance", {}).get("launches", 0) > 0
        for k in COUNTS[:4]:
            assert prof.get(k, {}).get("launches", 0) == 0, (pre, k, prof.get(k))
    for k in ("level", "key", "offset", "count"):
        assert tables[None][k].tobytes() == tables["0"][k].tobytes(), k
    ot = O.Tiler(*UNIT, O.MIN_DISTANCE, max_points, spacing)
    assert ot.add_batch(xyz[:half]) == 0 and ot.add_batch(xyz[half:]) == 0 and ot.finalize() == 0
    ex = ot.export()
    ot.close()
    mine = sorted(zip(tables[None]["level"].tolist(), tables[None]["key"].tolist(), tables[None]["count"].tolist()))
    theirs = sorted(zip(np.asarray(ex["level"]).tolist(), np.asarray(ex["key"]).tolist(), np.asarray(ex["count"]).tolist()))
    assert mine == theirs
