"""The two ways the key sweep numbers its cells (schwarzwald_amd/csrc/swz_mqbuild.hip, MqArgs::direct) against the CPU oracle.

Compacted: the occupied cells get consecutive ids from a count and a scan over the keys.  Direct: a cell's id is its place in
the grid of its node, every per-cell array covers the whole grid and an empty cell is an entry that says so.  The accepted set
must be the oracle's, point for point, on both -- forced through SWZ_MD_DIRECT = 0 / 1 -- for what direct numbering can get
wrong: empty cells inside a node and at its faces, take-all nodes beside sampled ones, a cell that ends where its node ends,
the last cell of the last node, cell starts at and around the 512-point tiles of the build passes, one point, one cell, an
occupancy at the threshold, a grid that does not fit, memory nobody wrote, and a context that is used for another cloud.
Every cloud has at most 2 M points."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
# every level on the sweep; a forced direct numbering still gives way to the compacted one above this many grid entries (the
# deep levels of a clustered cloud have grids of hundreds of millions of mostly empty cells: ~0.6 KB each)
BASE = {"SWZ_MD_SPARSE_LIMIT": "0", "SWZ_MD_DIRECT_MAX_CELLS": str(1 << 24)}
NUMBERINGS = [{"SWZ_MD_DIRECT": "0"}, {"SWZ_MD_DIRECT": "1"}]
_ids = lambda m: "direct" if m.get("SWZ_MD_DIRECT") == "1" else "compacted"


@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def _tile(ctx, xyz, bmin, bmax, d, mppn, options):
    import schwarzwald_amd as swz
    spacing = O.spacing_from_diagonal(bmin, bmax, d)
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        return ctx.tile(xyz, bmin, bmax, swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=mppn, spacing_at_root=spacing))
    finally:
        for k in options:
            ctx.set_option(k, None)


def _check(ctx, xyz, bmin, bmax, d, mppn, options, oracle=None):
    o = oracle if oracle is not None else O.tile(xyz, bmin, bmax, O.MIN_DISTANCE, mppn, O.spacing_from_diagonal(bmin, bmax, d))
    assert o["status"] == 0
    g = _tile(ctx, xyz, bmin, bmax, d, mppn, options)
    assert np.array_equal(g.keys, o["keys"]) and np.array_equal(g.perm, o["perm"])
    bad = np.flatnonzero(g.level != o["level"])
    assert bad.size == 0, "%s: %d points differ, first at sorted position %d: level %d, oracle %d" % (
        options, bad.size, bad[0], g.level[bad[0]], o["level"][bad[0]])
    return o


def _holes(rng, n):
    """A uniform cloud with holes at the scale of the cells of every level the sweep may choose (1/8 ... 1/128 of the root,
    which are cells of the levels below as well): a third of the cells of each scale is empty, whole cells at the faces of
    the octants among them."""
    xyz = rng.random((n, 3))
    keep = np.ones(n, bool)
    for k in (3, 4, 5, 6, 7):
        c = np.floor(xyz * (1 << k)).astype(np.int64)
        keep &= ((c[:, 0] + 2 * c[:, 1] + 3 * c[:, 2] + k) % 7) > 1
    lo = np.floor(xyz * 64).astype(np.int64)
    keep &= ~((lo[:, 0] == 31) | (lo[:, 1] == 32) | (lo[:, 2] == 0) | (lo[:, 2] == 63))  # slabs at faces of the root's octants
    return xyz[keep]


@pytest.mark.parametrize("numbering", NUMBERINGS, ids=_ids)
def test_empty_cells_inside_nodes_and_at_their_faces(ctx, numbering):
    rng = np.random.default_rng(7001)
    xyz = _holes(rng, 1500000)
    for d, mppn in ((250, 2000), (60, 800)):
        _check(ctx, xyz, *UNIT, d, mppn, {**BASE, **numbering})


@pytest.mark.parametrize("numbering", NUMBERINGS, ids=_ids)
def test_take_all_nodes_beside_sampled_ones(ctx, numbering):
    """A few hundred points per octant in seven octants (take-all nodes from level 0 on) and a dense eighth: on every level
    below the root the sampled nodes are a subset and their index is not the node's."""
    rng = np.random.default_rng(7002)
    sparse = rng.random((2500, 3))
    sparse = sparse[~np.all(sparse >= 0.5, axis=1)]
    dense = 0.5 + 0.5 * rng.random((600000, 3))
    mid = np.column_stack([0.5 * rng.random(40000), 0.5 + 0.5 * rng.random(40000), 0.25 * rng.random(40000)])  # a second sampled octant, not adjacent in order
    xyz = np.vstack([sparse, dense, mid])
    for d, mppn in ((250, 1000), (100, 500)):
        _check(ctx, xyz, *UNIT, d, mppn, {**BASE, **numbering})


@pytest.mark.parametrize("numbering", NUMBERINGS, ids=_ids)
def test_cell_that_ends_with_its_node_and_last_cell_of_the_last_node(ctx, numbering):
    """The last cells of several nodes are occupied and the first cells of the nodes after them are not (a cell's end is then
    its node's end, not the next cell start), the very last cell of the grid (the corner at the maximum) is occupied, and the
    sampled node in front of a take-all one ends with an occupied cell."""
    rng = np.random.default_rng(7003)
    body = rng.random((500000, 3))
    c = np.floor(body * 4).astype(np.int64)  # nodes of level 1: empty their low corners, crowd their high ones
    frac = body * 4 - c
    body = body[~np.all(frac < 0.3, axis=1)]
    corners = (np.floor(rng.random((60000, 3)) * 4) + 1.0 - 0.02 * rng.random((60000, 3))) / 4.0
    top = 1.0 - 1e-3 * rng.random((3000, 3))
    xyz = np.clip(np.vstack([body, corners, top]), 0.0, 1.0)
    for d, mppn in ((250, 1500), (80, 600)):
        _check(ctx, xyz, *UNIT, d, mppn, {**BASE, **numbering})


@pytest.mark.parametrize("first", [511, 512, 513, 1023, 1024, 1025])
@pytest.mark.parametrize("numbering", NUMBERINGS, ids=_ids)
def test_cell_start_at_a_tile_edge_of_the_build_pass(ctx, numbering, first):
    """Both build passes walk the sorted keys in tiles of 512.  The first cell of the root (and of the levels below, as long
    as the points survive) holds exactly `first` points, so the second cell starts one before, at, and one after a tile edge."""
    rng = np.random.default_rng(7004 + first)
    blob = rng.random((first, 3)) / 1024.0  # inside one cell of every candidate size
    rest = rng.random((400000, 3))
    rest = rest[~np.all(rest < 0.125, axis=1)]
    xyz = np.vstack([blob, rest])
    _check(ctx, xyz, *UNIT, 250, 2000, {**BASE, **numbering})


@pytest.mark.parametrize("numbering", NUMBERINGS, ids=_ids)
def test_one_point_and_one_cell(ctx, numbering):
    rng = np.random.default_rng(7005)
    one = np.array([[0.3, 0.6, 0.9]])
    _check(ctx, one, *UNIT, 250, 1, {**BASE, **numbering})
    cell = 0.7 + rng.random((20000, 3)) / 2048.0  # all points in one cell of the root, and of several levels below
    for mppn in (100, 50000):
        _check(ctx, cell, *UNIT, 250, mppn, {**BASE, **numbering})


@pytest.mark.parametrize("kept", [15, 16, 17])
def test_occupancy_around_the_threshold(ctx, kept):
    """Slabs: of every 32 cells of the finest root grid along x, `kept` hold points, so 15/32, 16/32 and 17/32 of the cells of
    that grid and of every finer one are occupied: below, at and above the default threshold of one half.  The library
    estimates the occupancy itself; around it the threshold is moved as well, so that both numberings are met whatever cell
    size the levels choose."""
    rng = np.random.default_rng(7006 + kept)
    xyz = rng.random((1600000, 3))
    xyz = xyz[(np.floor(xyz[:, 0] * 128).astype(np.int64) % 32) < kept]
    o = None
    for thr in (None, "0.4", "0.46", "0.47", "0.5", "0.53", "0.54", "0.6", "0.99", "1.01"):
        opts = dict(BASE)
        if thr is not None:
            opts["SWZ_MD_DIRECT_MIN_OCCUPANCY"] = thr
        o = _check(ctx, xyz, *UNIT, 250, 2000, opts, oracle=o)


def test_grid_that_does_not_fit_takes_the_compacted_numbering(ctx):
    rng = np.random.default_rng(7007)
    xyz = _holes(rng, 600000)
    o = None
    for cap in ("0", "1", "4096", "300000", str(1 << 21), str(1 << 30)):
        o = _check(ctx, xyz, *UNIT, 250, 2000, {"SWZ_MD_SPARSE_LIMIT": "0", "SWZ_MD_DIRECT": "1", "SWZ_MD_DIRECT_MAX_CELLS": cap}, oracle=o)


@pytest.mark.parametrize("numbering", NUMBERINGS, ids=_ids)
def test_poisoned_workspace_shows_entries_nobody_wrote(numbering):
    """A context of its own whose new workspace memory is filled with 0xCD: an entry of a per-cell array that the build
    leaves out and somebody reads is no longer a zero by luck."""
    import schwarzwald_amd as swz
    rng = np.random.default_rng(7008)
    clouds = [_holes(rng, 700000), np.vstack([rng.random((3000, 3)), 0.5 + 0.5 * rng.random((300000, 3))])]
    with swz.Context(0) as c:
        c.set_option("SWZ_POISON", "205")
        try:
            for xyz in clouds:
                for modes in ({}, {"SWZ_MD_LAZY": "0"}, {"SWZ_MD_BIG": "1", "SWZ_MD_GROUPS": "1", "SWZ_MD_DENSE_MIN": "64"}):
                    _check(c, xyz, *UNIT, 250, 1500, {**BASE, **numbering, **modes})
        finally:
            c.set_option("SWZ_POISON", None)


@pytest.mark.parametrize("numbering", NUMBERINGS + [{}], ids=lambda m: _ids(m) if m else "chosen")
def test_two_clouds_on_one_context(numbering):
    """Nothing of a call survives into the next: a full cloud, then one whose cells are mostly somewhere else (and fewer), then
    the first again, on one context; per-cell arrays are reused, and which cells are empty is decided anew."""
    import schwarzwald_amd as swz
    rng = np.random.default_rng(7009)
    full = rng.random((900000, 3))
    other = _holes(rng, 500000) * np.array([1.0, 0.5, 1.0]) + np.array([0.0, 0.5, 0.0])
    with swz.Context(0) as c:
        oracles = [None, None]
        for which in (0, 1, 0, 1):
            xyz = (full, other)[which]
            oracles[which] = _check(c, xyz, *UNIT, 250, 2000, {**BASE, **numbering}, oracle=oracles[which])
