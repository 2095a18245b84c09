"""The block kernel's search loop and halo look-up (swz_mdblock.hip) on inputs that lean on exactly what they do: a lane is
busy while it has a candidate or a cell left (no flag), a lane without a candidate still computes a distance, the entry
of "no cell left" is a real entry, a halo point's run is found by probing a clamped table.  Every case against the oracle,
point for point, in both point formats."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
FORMATS = {"narrow": {}, "wide": {"SWZ_SP_BLOCK_WIDE": "1"}}
# every level the keys can decide goes to the block path; blocks as small as they come
EVERY_LEVEL = {"SWZ_MD_SPARSE_LIMIT": "1000", "SWZ_SP_BLOCK_MIN": "1"}


@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def _check(ctx, xyz, d, mppn, options, bounds=UNIT):
    import schwarzwald_amd as swz
    spacing = O.spacing_from_diagonal(*bounds, d)
    o = O.tile(xyz, *bounds, O.MIN_DISTANCE, mppn, spacing)
    assert o["status"] == 0
    try:
        for k, v in options.items():
            ctx.set_option(k, v)
        g = ctx.tile(xyz, *bounds, swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=mppn, spacing_at_root=spacing))
    finally:
        for k in options:
            ctx.set_option(k, None)
    assert np.array_equal(g.keys, o["keys"]) and np.array_equal(g.perm, o["perm"])
    assert np.array_equal(g.level, o["level"])


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_blocks_with_fewer_own_points_than_a_wavefront_has_lanes(ctx, fmt):
    """A thin cloud on fine cells: blocks of a few dozen points, so that most lanes of a round hold no point, the halo is
    staged right behind fewer than 64 own points and a wavefront's share of a block is often empty."""
    xyz = np.random.default_rng(101).random((60000, 3))
    for d, mppn in ((250, 300), (120, 150)):
        _check(ctx, xyz, d, mppn, {**EVERY_LEVEL, **FORMATS[fmt]})


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_one_crowded_cell_among_empty_ones(ctx, fmt):
    """Tight clumps far apart: one lane of a round has hundreds of candidates in one cell while the others have none --
    the loop runs on that lane alone -- and its neighbours outnumber what a list holds (it searches again)."""
    rng = np.random.default_rng(102)
    centres = rng.random((40, 3)) * 0.9 + 0.05
    clumps = (centres[:, None, :] + 0.0015 * rng.standard_normal((40, 600, 3))).reshape(-1, 3)
    xyz = np.clip(np.vstack([clumps, rng.random((20000, 3))]), 0.0, 1.0)
    _check(ctx, xyz, 250, 500, {**EVERY_LEVEL, **FORMATS[fmt]})
    _check(ctx, xyz, 250, 500, {"SWZ_MD_SPARSE_LIMIT": "1000", **FORMATS[fmt]})


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_lattice_ties_at_exactly_the_spacing(ctx, fmt):
    """A lattice whose pitch is the spacing of a level: every pair of neighbours sits at the bound itself (not closer: both
    stay) and inside the quantisation band, so every such pair is compared on the original positions; a second lattice
    shifted by a hair below the pitch puts pairs just inside."""
    d = 100
    spacing = O.spacing_from_diagonal(*UNIT, d)
    pitch = spacing / 4.0  # the spacing two levels down
    n = int(0.98 / pitch)
    ax = np.arange(n, dtype=np.float64) * pitch + 0.01
    lattice = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    shifted = lattice[::3] + np.array([pitch * (1.0 - 2.0 ** -20), 0.0, 0.0])
    xyz = np.clip(np.vstack([lattice, shifted]), 0.0, 1.0)
    xyz = xyz[np.random.default_rng(103).permutation(len(xyz))]
    _check(ctx, xyz, d, 400, {**EVERY_LEVEL, **FORMATS[fmt]})
    _check(ctx, xyz, d, 400, {"SWZ_MD_SPARSE_LIMIT": "1000", "SWZ_SP_FILTER_EPS": "1e30", **FORMATS[fmt]})


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_a_slab_of_points_so_that_most_halo_runs_are_empty(ctx, fmt):
    """Points on a thin slab and a line: most of the 216 granule runs around a block are empty, the table of run offsets is
    full of repeats, and the look-up of a halo point's run has to step over them."""
    rng = np.random.default_rng(104)
    slab = rng.random((150000, 3))
    slab[:, 2] = 0.5 + 0.002 * rng.standard_normal(len(slab))
    line = np.outer(rng.random(30000), [1.0, 1.0, 1.0]) + 0.0005 * rng.standard_normal((30000, 3))
    xyz = np.clip(np.vstack([slab, line]), 0.0, 1.0)
    _check(ctx, xyz, 250, 1000, {**EVERY_LEVEL, **FORMATS[fmt]})
    _check(ctx, xyz, 250, 1000, {"SWZ_MD_SPARSE_LIMIT": "1000", **FORMATS[fmt]})
