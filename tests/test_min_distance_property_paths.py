"""Property-mode MIN_DISTANCE (SWZ_FLAG_MIN_DISTANCE_PROPERTY) on ties, stacks and every kill path.

The families of tests/test_min_distance_adversarial.py (lattices with pairs exactly at a level's spacing, the same at pitch
0.001, LAS records in cubic and in their own bounds, stacks of duplicates) and three new ones run through every path of
swz_mdrounds.hip and swz_mdprop.hip, chosen by option and PROVEN by the SWZ_DEBUG trace: the block, records and mask-loop
kill passes, the rounds with and without the list of alive points and the per-cell steps over it, every compare on the exact
path, the coloured phases, and the exact paths a level goes to when the rounds decline.  What must hold: the exact mode's
keys and order, properties (a) spacing and (b) maximality on every sampled node with the reference's compare
((dx*dx + dy*dy) + dz*dz < float-squared spacing, widened to double: a pair AT the spacing is allowed and must not kill),
bit-identical sets from all accelerators of the rounds, and determinism.  Every comparison is exact.

New families (CPU premises below):
  shared-block  a clump of 71 000 points, a third of them stacks, around the common corner of eight root cells: one block of
                the block kill pass (2, 4 or 8 cells per edge) shared by three workgroups with a partial last chunk; cells of
                more than PM_BIG points for the big-cell pass of the phases; a ring of points in the cells around it.
  band          a lattice at the root spacing with partners displaced by less than one key cell: thousands of pairs inside
                the key metric's band on either side of the spacing and exactly at it.
  packed        a face-centred cubic packing at (1 + 1e-9) spacings: see below.

Bounds that are not a cube have no key metric: no level of theirs can run in rounds, whatever the options.  That is las-aabb
and, by a hair, las-cubic: its bounds are the minimum plus the largest extent, and at UTM offsets those sums do not subtract
back to the same extent on every axis (key_metric asks for ex == ey == ez).  The rounds legs assert exactly that there -- no
rounds line, the phases line on every sampled level -- and everything else as on the other families; family "las-cube" puts
the same records into bounds with whole-numbered corners 256 apart, which are a cube to the last bit, and runs in rounds.

PM_FRESH / PM_WIN (swz_mdprop.hip: 64 taken points of a cell, 128 of its neighbourhood, held in LDS; more spill).  Both can
occur at these sizes.  phases_cell_levels goes one level coarser than the finest cells (side r0 in [1, 2) spacings) when the
finest cells hold < 24 points on average and the points-weighted mean population one level up is <= 1024 (its other
condition, 0.75 * 8 * r0^3 <= 48, always holds for r0 <= 2); md_clamp_cell_levels does not bind below 2^31 cells.  The
cells are then up to 4 spacings wide.  A neighbourhood of 26 such cells passes 128 taken points easily: the lattice at
pitch = spacing has 64 per cell (family "lattice", level 4 in the phases leg: 26 * 64).  One cell passes 64 only with a
packing denser than a cubic lattice -- a cube of 4 x 4 x 4 spacings holds 64 lattice points, but about 90 of a face-centred
cubic packing.  Family "packed" is that, on 4-spacing cells, and test_packed_cells_spill_the_taken_points asserts the
properties there and, from the result, that a cell took more than PM_FRESH points.
"""
import functools
import re

import numpy as np
import pytest

import oracle_lib as O
import test_min_distance_adversarial as A
from test_min_distance_adversarial import UNIT, _level_spacing, _property_levels, _sq_dist, _with
from test_min_distance_property import _check_property

PR_CHUNK = 32768   # swz_mdrounds.hip: points of a block per workgroup of the block kill pass
PM_BIG = 4096      # swz_mdprop.hip: cells with more points get the big-cell pass
PM_FRESH = 64      # ... taken points of one cell held in LDS
PM_WIN = 128       # ... taken points of the 26 cells around it held in LDS at a time

# ------------------------------------------------------------------------------------------------------------ new families
SB_D, SB_MPPN = 250, 20000
SB_CELL = 64              # the clump sits around the corner (65, 65, 65) / 128 of the root cells 64 and 65 per axis
SB_STACKS, SB_STACK = 8, 3000
SB_LOOSE = 47000


def _geo_cell_width(extent, spacing_at_root):
    """make_plan's cell_levels_geo: halve the extent while the half is still a spacing (and 2^-20 of it) wide."""
    levels = 0
    while levels < 20 and extent / 2 >= float(spacing_at_root) * (1.0 + 2.0 ** -20):
        extent /= 2
        levels += 1
    return extent, levels


def _shared_block(seed):
    """-> (xyz, is_clump): the clump (loose points and stacks in a cube of half-side 0.57 root cells around the corner), a ring
    on the surface of the cube of half-side 1.05 cells around it, a uniform background over the 32^3 root cells around."""
    rng = np.random.default_rng(seed)
    w = 1.0 / 128.0
    centre = np.full(3, (SB_CELL + 1) * w)
    loose = centre + (rng.random((SB_LOOSE, 3)) - 0.5) * (2 * 0.57 * w)
    # one stack in each of the eight cells
    corners = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], dtype=np.float64)
    stacks = np.repeat(centre + corners * (0.2 + 0.3 * rng.random((SB_STACKS, 3))) * w, SB_STACK, axis=0)
    ring = (rng.random((3000, 3)) - 0.5) * 2.0
    ring[np.arange(3000), rng.integers(0, 3, 3000)] = rng.choice([-1.0, 1.0], 3000)
    ring = centre + ring * 1.05 * w
    back = (SB_CELL + 1 - 16) * w + rng.random((200000, 3)) * 32 * w
    xyz = np.vstack([loose, stacks, ring, back])
    is_clump = np.arange(xyz.shape[0]) < SB_LOOSE + SB_STACKS * SB_STACK
    perm = rng.permutation(xyz.shape[0])
    return xyz[perm], is_clump[perm]


BAND = ([0.0, 0.0, 0.0], [64.0, 64.0, 64.0])   # one key cell = 2^-15; spacing 1 at the root = 32 768 key cells
BAND_SPACING, BAND_MPPN = 1.0, 500


def _band(seed):
    """A 40^3 lattice of pitch 1 = the root spacing; every second lattice point has a partner displaced along one axis by
    0.1 .. 0.9 key cells either way: with the lattice neighbours along that axis it forms one pair just inside the spacing
    and one just outside, both within a key cell of it.  The lattice neighbours themselves are exactly at the spacing."""
    rng = np.random.default_rng(seed)
    g = np.arange(12, 52, dtype=np.float64)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    src = lat[(lat.sum(axis=1) % 2) == 0]
    eps = rng.choice([-1.0, 1.0], src.shape[0]) * (0.1 + 0.8 * rng.random(src.shape[0])) * 2.0 ** -15
    partners = src.copy()
    partners[np.arange(src.shape[0]), rng.integers(0, 3, src.shape[0])] += eps
    scatter = rng.random((5000, 3)) * 64.0
    xyz = np.vstack([lat, partners, scatter])
    return xyz[rng.permutation(xyz.shape[0])]


PACKED = ([0.0, 0.0, 0.0], [32.0, 32.0, 32.0])
PACKED_SPACING, PACKED_MPPN = 1.0, 20000


def _packed(seed):
    """Face-centred cubic packing with nearest neighbours (1 + 1e-9) spacings apart -- no pair is closer than the spacing,
    every position is taken -- and 12 000 duplicates for the points left out."""
    rng = np.random.default_rng(seed)
    a = (1.0 + 1e-9) / np.sqrt(2.0)
    g = np.arange(0, 46)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    fcc = ijk[(ijk.sum(axis=1) % 2) == 0].astype(np.float64) * a
    xyz = np.vstack([fcc, fcc[rng.integers(0, fcc.shape[0], 12000)]])
    return xyz[rng.permutation(xyz.shape[0])], fcc.shape[0]


@functools.lru_cache(maxsize=None)
def family(name):
    """name -> (xyz, bounds, [(spacing_at_root, max_points_per_node), ...]): the adversarial module's families and the new ones"""
    if name == "shared-block":
        return _shared_block(6)[0], UNIT, [(O.spacing_from_diagonal(*UNIT, SB_D), SB_MPPN)]
    if name == "band":
        return _band(7), BAND, [(BAND_SPACING, BAND_MPPN)]
    if name == "packed":
        return _packed(8)[0], PACKED, [(PACKED_SPACING, PACKED_MPPN)]
    if name == "las-cube":
        # The LAS records in bounds whose extents are EQUAL doubles: "las-cubic" adds the largest extent to the minimum at UTM
        # offsets, and the sums do not subtract back to one extent on every axis -- key_metric's test (ex == ey == ez) fails,
        # that family is decided on positions like las-aabb.  Whole-numbered corners 256 apart subtract exactly.
        xyz = A._las_cloud(3)
        lo = np.floor(xyz.min(axis=0))
        bounds = (lo.tolist(), (lo + 256.0).tolist())
        return xyz, bounds, [(O.spacing_from_diagonal(*bounds, 250), 2000), (O.spacing_from_diagonal(*bounds, 90), 500)]
    return A.family(name)


@functools.lru_cache(maxsize=None)
def _oracle(name, case):
    if name not in ("shared-block", "band", "packed", "las-cube"):
        return A._oracle(name, case)
    xyz, bounds, cases = family(name)
    sp, mppn = cases[case]
    o = O.tile(xyz, *bounds, O.MIN_DISTANCE, mppn, sp)
    assert o["status"] == 0
    return o


FAMILIES = ["lattice", "lattice-0.001", "las-cubic", "las-aabb", "las-cube", "stacks", "shared-block", "band"]
# the level whose spacing is the lattice pitch (test_lattice_has_exact_ties; band: the root), per case
TIE_LEVEL = {"lattice": (4, 3), "lattice-0.001": (4,), "band": (-1,)}


def _is_cubic(bounds):
    e = np.asarray(bounds[1]) - np.asarray(bounds[0])
    return e[0] == e[1] == e[2]


def _key_coords(keys):
    """key bit 3j + 2 is bit j of x, 3j + 1 of y, 3j of z (MortonIndex.h:62-79)"""
    out = np.zeros((keys.shape[0], 3), dtype=np.int64)
    for j in range(21):
        for axis, bit in ((0, 2), (1, 1), (2, 0)):
            out[:, axis] |= ((keys >> np.uint64(3 * j + bit)) & np.uint64(1)).astype(np.int64) << j
    return out


def _key_metric(bounds, spacing_at_root, L, extra_band=0.0):
    """key_metric (swz_mdkeys.hip): the spacing in key cells and the float thresholds of the band around its square."""
    cell = (bounds[1][0] - bounds[0][0]) / 2097152.0
    T = np.sqrt(_level_spacing(spacing_at_root, L)[1]) / cell
    band = 1.75 + T * 2.0 ** -20 + extra_band
    lo, hi = T - band, T + band
    f_lo = np.float32(0.0)
    if lo > 0.0:
        f_lo = np.float32(lo * lo)
        while float(f_lo) > lo * lo:
            f_lo = np.nextafter(f_lo, np.float32(0.0))
        f_lo = np.nextafter(f_lo, np.float32(0.0))
    f_hi = np.float32(hi * hi)
    while float(f_hi) < hi * hi:
        f_hi = np.nextafter(f_hi, np.float32(np.inf))
    f_hi = np.nextafter(f_hi, np.float32(np.inf))
    return T, float(f_lo), float(f_hi)


# --------------------------------------------------------------------------------------------------------- CPU: premises
def test_shared_block_premise():
    xyz, is_clump = _shared_block(6)
    sp, mppn = family("shared-block")[2][0]
    n = xyz.shape[0]
    assert n <= 300000 and int(is_clump.sum()) >= 70000
    width, cl = _geo_cell_width(1.0, sp)
    assert width == 1.0 / 128.0 and cl == 7
    s, sq = _level_spacing(sp, -1)
    keys, pos = O.index_points(xyz, *UNIT)
    centre = np.full(3, (SB_CELL + 1) * width)
    # the clump: within less than one root cell of the common corner of an aligned 2 x 2 x 2 group of root cells
    assert np.sqrt(_sq_dist(pos[is_clump], centre)).max() < width and SB_CELL % 8 == 0
    # a third of it in stacks, none larger than a node may hold
    _, counts = np.unique(pos[is_clump], axis=0, return_counts=True)
    stacked = int(counts[counts > 1].sum())
    assert 0.3 < stacked / is_clump.sum() < 0.4 and counts.max() <= mppn and counts.max() >= 1000
    # 1: whatever block edge the kill pass chooses, the clump's block is shared by three workgroups or more and the last
    # one gets a partial chunk
    block_counts = {}
    for bl in (1, 2, 3):
        block = keys >> np.uint64(63 - 3 * (cl - bl))
        ids = np.unique(block[is_clump])
        assert ids.size == 1, bl
        count = int((block == ids[0]).sum())
        block_counts[1 << bl] = count
        assert count > 2 * PR_CHUNK and count % PR_CHUNK != 0, (bl, count)
    # 2: root cells of more than PM_BIG points
    cell = keys >> np.uint64(63 - 3 * cl)
    cells, per_cell = np.unique(cell, return_counts=True)
    assert per_cell.max() > PM_BIG
    # 3: points of the cells around the clump's cells within the spacing of clump points (the reference's compare)
    from scipy.spatial import cKDTree
    clump_cells = np.unique(cell[is_clump])
    assert clump_cells.size == 8
    outside = np.flatnonzero(~np.isin(cell, clump_cells))
    m = cKDTree(pos[outside]).sparse_distance_matrix(cKDTree(pos[is_clump]), s * (1.0 + 1e-9), output_type="ndarray")
    clump_pos = pos[is_clump]
    near = np.unique(m["i"][_sq_dist(pos[outside][m["i"]], clump_pos[m["j"]]) < sq])
    grid = np.floor(pos / width).astype(np.int64)
    near_cells = np.unique(grid[outside[near]], axis=0)
    assert np.abs(near_cells - SB_CELL - 0.5).max() <= 1.5   # (all of them adjacent to the group)
    # ... and every one of the 26 cells around each of the clump's cells holds points
    occupied = {tuple(c) for c in np.unique(grid, axis=0)}
    for c in np.unique(grid[is_clump], axis=0):
        assert all((c[0] + i, c[1] + j, c[2] + k) in occupied for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1))
    # 4: not a sparse level (min_distance_level: points per occupied cell below 2 go to the exact block path)
    population = n / cells.size
    print("shared-block: %d points, clump %d (%d in stacks, largest %d); points of the clump's block by block edge %r; largest root "
          "cell %d points; %d cells around the clump with points within its spacing (%d such points); %.2f points per occupied "
          "root cell" % (n, int(is_clump.sum()), stacked, int(counts.max()), block_counts, int(per_cell.max()), near_cells.shape[0],
                         near.size, population))
    assert near_cells.shape[0] >= 8
    assert population >= 2.0


def test_band_premise():
    xyz, bounds, cases = family("band")
    sp, mppn = cases[0]
    assert 90000 <= xyz.shape[0] <= 110000 and _is_cubic(bounds)
    o = _oracle("band", 0)
    assert o["stats"]["max_level"] <= 1   # (the root and at most one more level are sampled)
    T, f_lo, f_hi = _key_metric(bounds, sp, -1)
    assert T == 32768.0
    a, b, d2, sq = A._node_pairs_at(o, sp, -1, radius_scale=1.0 + 1e-3)
    q = _key_coords(o["keys"])
    dq = (q[a] - q[b]).astype(np.float64)
    d2_key = (dq * dq).sum(axis=1)
    in_band = (d2_key >= f_lo) & (d2_key < f_hi)
    # (well inside: within one key cell of the spacing, whatever the rounding of the float evaluation -- the band is 1.75 wide)
    sure = np.abs(np.sqrt(d2_key) - T) <= 1.0
    assert in_band[sure].all()
    below, at, above = int((sure & (d2 < sq)).sum()), int((sure & (d2 == sq)).sum()), int((sure & (d2 > sq)).sum())
    print("band: %d points, spacing %.0f key cells, band [%.0f, %.0f): %d same-node pairs in the band, %d closer than the spacing, "
          "%d exactly at it, %d beyond" % (xyz.shape[0], T, f_lo, f_hi, int(in_band.sum()), below, at, above))
    assert below >= 1000 and at + above >= 1000 and at >= 100 and above >= 1000


def test_packed_premise():
    """No two distinct positions are closer than the spacing (all of them are taken at the root), the phases' cell rule
    chooses cells of 4 spacings there, and such a cell holds more than PM_FRESH positions, its neighbourhood more than PM_WIN."""
    from scipy.spatial import cKDTree
    xyz, distinct = _packed(8)
    sp, mppn = family("packed")[2][0]
    assert xyz.shape[0] <= 300000 and xyz.shape[0] > mppn
    s, sq = _level_spacing(sp, -1)
    pos = np.unique(xyz, axis=0)
    assert pos.shape[0] == distinct
    pairs = cKDTree(pos).query_pairs(s * (1.0 + 1e-6), output_type="ndarray")
    assert pairs.shape[0] > 100000 and not (_sq_dist(pos[pairs[:, 0]], pos[pairs[:, 1]]) < sq).any()
    # phases_cell_levels (swz_md.hip): the finest cells are 2 spacings wide and hold < 24 points each, the points-weighted mean
    # population one level up is <= 1024: one level coarser, 4 spacings
    width, cl = _geo_cell_width(32.0, sp)
    assert (width, cl) == (2.0, 4)
    fine = np.unique(np.floor(xyz / width), axis=0, return_counts=True)[1]
    r0 = width / s
    assert xyz.shape[0] / fine.size < 24.0 and 0.75 * 8.0 * r0 ** 3 <= 48.0
    coarse_all = np.unique(np.floor(xyz / (2 * width)), axis=0, return_counts=True)[1]
    assert (coarse_all.astype(np.float64) ** 2).sum() / xyz.shape[0] <= 1024.0
    assert xyz.shape[0] / fine.size >= 2.0   # (and the level is not sparse)
    cells, per_cell = np.unique(np.floor(pos / (2 * width)).astype(np.int64), axis=0, return_counts=True)
    print("packed: %d points, %d positions; cells of 4 spacings hold up to %d positions (PM_FRESH %d), %d cells more than that"
          % (xyz.shape[0], distinct, int(per_cell.max()), PM_FRESH, int((per_cell > PM_FRESH).sum())))
    assert per_cell.max() > PM_FRESH and (per_cell > PM_FRESH).sum() >= 100
    assert per_cell.min() * 7 > PM_WIN   # (a corner cell has seven cells around it)


# ------------------------------------------------------------------------------------------------------------ GPU: the trace
ROUNDS_LINE = re.compile(r"MIN_DISTANCE property level (-?\d+) in rounds: (\d+) pts in (\d+) nodes, .*? (\d+) rounds, (\d+) exact compares, "
                         r".*?; kill pass (block B=\d|records|mask loop), (\d+) extra chunks, list from round (\d+), (\d+) rounds by cell lists;")
PHASES_LINE = re.compile(r"MIN_DISTANCE property level (-?\d+): (\d+) pts in (\d+) nodes, cell levels (\d+) of (\d+), (\d+) cells .*?, "
                         r"(\d+) big-cell units,")
EXACT_LINES = (re.compile(r"MIN_DISTANCE level (-?\d+) block path[^:]*:.* abort 0 "), re.compile(r"MIN_DISTANCE level (-?\d+) on keys: sweep "),
               re.compile(r"MIN_DISTANCE level (-?\d+) sparse path: "))


def _parse(err):
    """-> {level: record of the algorithm that decided it}; a level a path declined or abandoned shows the later one"""
    out = {}
    for line in err.splitlines():
        m = ROUNDS_LINE.search(line)
        if m:
            out[int(m.group(1))] = dict(path="rounds", kill=m.group(6), exact=int(m.group(5)), chunks=int(m.group(7)),
                                        list_round=int(m.group(8)), cell_list_rounds=int(m.group(9)), rounds=int(m.group(4)))
            continue
        m = PHASES_LINE.search(line)
        if m:
            out[int(m.group(1))] = dict(path="phases", cell_levels=int(m.group(4)), geo=int(m.group(5)), units=int(m.group(7)))
            continue
        for rx in EXACT_LINES:
            m = rx.search(line)
            if m:
                out[int(m.group(1))] = dict(path="exact")
    return out


def _sampled_levels(r, mppn, last):
    """the levels -1 .. last on which a node holds more than mppn points"""
    out = []
    for L in range(-1, last + 1):
        active = r.level >= L
        shift = 63 - 3 * (L + 1)
        node = (r.keys[active] >> np.uint64(shift)) if shift < 63 else np.zeros(int(active.sum()), dtype=np.uint64)
        if active.any() and np.unique(node, return_counts=True)[1].max() > mppn:
            out.append(L)
    return out


@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


OPTIONS = ("SWZ_DEBUG", "SWZ_MD_SPARSE_LIMIT", "SWZ_MD_ROUNDS", "SWZ_MD_ROUNDS_BLOCK", "SWZ_MD_ROUNDS_WLIST_MIN_POP", "SWZ_MD_ROUNDS_LIST",
           "SWZ_MD_ROUNDS_CELL_LISTS", "SWZ_MD_KEYS_BAND", "SWZ_MD_KEYS")


@pytest.fixture(autouse=True)
def _options_cleared(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        for k in OPTIONS:
            c.set_option(k, None)


ROUNDS = {"SWZ_MD_SPARSE_LIMIT": "0"}
PLAIN = "rounds on every level"
LEGS = {
    "default": {},
    PLAIN: ROUNDS,
    "rounds, block kill off": dict(ROUNDS, SWZ_MD_ROUNDS_BLOCK="0"),
    "rounds, records forced": dict(ROUNDS, SWZ_MD_ROUNDS_BLOCK="0", SWZ_MD_ROUNDS_WLIST_MIN_POP="0"),
    "rounds, mask loop forced": dict(ROUNDS, SWZ_MD_ROUNDS_BLOCK="0", SWZ_MD_ROUNDS_WLIST_MIN_POP="1e9"),
    "rounds, no alive list": dict(ROUNDS, SWZ_MD_ROUNDS_LIST="0"),
    "rounds, no per-cell list steps": dict(ROUNDS, SWZ_MD_ROUNDS_CELL_LISTS="0"),
    # (the largest spacing of any family is 262 144 key cells: f_lo = 0, every pair in reach takes the exact compare)
    "rounds, every compare exact": dict(ROUNDS, SWZ_MD_KEYS_BAND="1e7"),
    "coloured phases on every level": {"SWZ_MD_KEYS": "0", "SWZ_MD_SPARSE_LIMIT": "0"},
    "rounds declined": {"SWZ_MD_ROUNDS": "0"},
}
TWICE = ("default", PLAIN, "coloured phases on every level")


def _run(ctx, capfd, name, case, options):
    """-> (result, {level: what decided it}) of one property-mode tile call under SWZ_DEBUG"""
    import schwarzwald_amd as swz
    xyz, bounds, cases = family(name)
    sp, mppn = cases[case]
    p = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=mppn, spacing_at_root=sp, flags=swz.FLAG_MIN_DISTANCE_PROPERTY)
    capfd.readouterr()
    r = _with(ctx, dict(options, SWZ_DEBUG="1"), lambda: ctx.tile(xyz, *bounds, p))
    return r, _parse(capfd.readouterr().err)


_plain = {}


def _plain_rounds(ctx, capfd, name, case):
    """the plain "rounds on every level" leg, once per family and case: what every other rounds leg must reproduce"""
    if (name, case) not in _plain:
        _plain[(name, case)] = _run(ctx, capfd, name, case, LEGS[PLAIN])
    return _plain[(name, case)]


def _properties(name, case, r, what):
    sp, mppn = family(name)[2][case]
    a, b = _check_property(r.keys, r.level, r.xyz_clamped[r.perm], sp, mppn, _property_levels(name, r))
    assert a > 0 and b > 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("name", FAMILIES)
def test_property_paths(ctx, capfd, name, leg):
    xyz, bounds, cases = family(name)
    cubic = _is_cubic(bounds)
    for case, (sp, mppn) in enumerate(cases):
        what = "%s, spacing %r, max_points %d, %s" % (name, sp, mppn, leg)
        o = _oracle(name, case)
        r, trace = _plain_rounds(ctx, capfd, name, case) if leg == PLAIN else _run(ctx, capfd, name, case, LEGS[leg])
        with capfd.disabled():
            print("\n" + what, "->", {L: (t["path"],) + ((t["kill"], t["chunks"], t["list_round"], t["cell_list_rounds"], t["exact"])
                                                        if t["path"] == "rounds" else ()) for L, t in sorted(trace.items())})
        # 1. keys and order are the exact mode's
        assert np.array_equal(r.keys, o["keys"]) and np.array_equal(r.perm, o["perm"]), what
        last = _property_levels(name, r)
        sampled = _sampled_levels(r, mppn, last)
        assert sampled and sampled[0] == -1, what
        assert all(L in trace for L in sampled), (what, sampled, sorted(trace))   # (no level is decided silently)
        tie = TIE_LEVEL[name][case] if name in TIE_LEVEL else None
        if tie is not None:
            assert tie in sampled, what
        in_rounds = {L: t for L, t in trace.items() if t["path"] == "rounds"}
        # 4. determinism
        if leg in TWICE:
            again, _ = _run(ctx, capfd, name, case, LEGS[leg])
            assert np.array_equal(again.level, r.level), what + ": two runs differ"

        if leg.startswith("rounds") and leg != "rounds declined":
            plain, plain_trace = _plain_rounds(ctx, capfd, name, case)
            # 3. accelerators of one algorithm: the same set, byte for byte
            assert r.level.tobytes() == plain.level.tobytes(), what + ": " + A._first_difference(r.level, plain.level)
            if leg == PLAIN:
                _properties(name, case, r, what)   # 2. (once for all the legs that agree with it)
            if not cubic:
                # no key metric without cubic bounds: never the rounds, the phases on every sampled level instead
                assert not in_rounds and all(trace[L]["path"] == "phases" for L in sampled), (what, trace)
                continue
            # 5. the path was taken
            assert in_rounds, (what, trace)
            assert set(in_rounds) == {L for L, t in plain_trace.items() if t["path"] == "rounds"}, what
            kills = {t["kill"] for t in in_rounds.values()}
            if leg == "rounds, records forced":
                # (a grid whose records -- 448 bytes per cell -- do not fit the memory falls back to the mask loop: the stacks' deep levels)
                assert "records" in kills and kills <= {"records", "mask loop"}, (what, kills)
            elif leg == "rounds, mask loop forced":
                assert kills == {"mask loop"}, (what, kills)
            elif leg == "rounds, block kill off":
                assert kills <= {"records", "mask loop"}, (what, kills)
            else:
                assert all(k in ("block B=2", "block B=4", "block B=8") for k in kills), (what, kills)
                if name == "shared-block":
                    assert in_rounds[-1]["chunks"] >= 2, (what, in_rounds[-1])
            if tie is not None:
                assert tie in in_rounds, (what, sorted(in_rounds))
            if leg == "rounds, no alive list":
                assert all(t["list_round"] == 0 and t["cell_list_rounds"] == 0 for t in in_rounds.values()), (what, in_rounds)
            elif leg == "rounds, no per-cell list steps":
                assert all(t["cell_list_rounds"] == 0 for t in in_rounds.values()), (what, in_rounds)
            elif leg == PLAIN:
                assert any(t["list_round"] > 0 for t in in_rounds.values()), (what, in_rounds)
                assert any(t["cell_list_rounds"] > 0 for t in in_rounds.values()), (what, in_rounds)
            if leg == "rounds, every compare exact":
                for L, t in in_rounds.items():
                    assert t["exact"] > 0 and t["exact"] >= plain_trace[L]["exact"], (what, L, t, plain_trace[L])
        elif leg == "coloured phases on every level":
            _properties(name, case, r, what)
            assert not in_rounds, (what, trace)
            assert all(trace[L]["path"] == "phases" for L in sampled), (what, sampled, trace)
            if name == "shared-block":
                assert trace[-1]["units"] > 0, (what, trace[-1])
                with capfd.disabled():
                    print("shared-block, phases: %d big-cell units at the root" % trace[-1]["units"])
        elif leg == "rounds declined":
            # 6. what neither the rounds nor the phases decided, an exact path did; all levels: the oracle's set
            assert not in_rounds, (what, trace)
            if cubic:
                assert all(trace[L]["path"] in ("exact", "phases") for L in sampled), (what, trace)
            if all(trace[L]["path"] == "exact" for L in sampled):
                assert np.array_equal(r.level, o["level"]), what + ": " + A._first_difference(r.level, o["level"])
            _properties(name, case, r, what)
        else:
            _properties(name, case, r, what)


@pytest.mark.gpu
def test_packed_cells_spill_the_taken_points(ctx, capfd):
    """Family "packed" in the coloured phases: cells of 4 spacings (the trace says so) that take more than PM_FRESH points
    each, with more than PM_WIN taken points around them; every position is taken, every duplicate handed down."""
    xyz, bounds, cases = family("packed")
    sp, mppn = cases[0]
    o = _oracle("packed", 0)
    r, trace = _run(ctx, capfd, "packed", 0, LEGS["coloured phases on every level"])
    assert np.array_equal(r.keys, o["keys"]) and np.array_equal(r.perm, o["perm"])
    assert trace[-1]["path"] == "phases" and (trace[-1]["cell_levels"], trace[-1]["geo"]) == (3, 4), trace
    a, b = _check_property(r.keys, r.level, r.xyz_clamped[r.perm], sp, mppn, r.stats["max_level"])
    assert a > 0 and b > 0
    pos = r.xyz_clamped[r.perm]
    taken = r.level == -1
    assert int(taken.sum()) == _packed(8)[1] == np.unique(pos[taken], axis=0).shape[0]
    per_cell = np.unique(np.floor(pos[taken] / 4.0).astype(np.int64), axis=0, return_counts=True)[1]
    print("packed, phases: up to %d taken points in a cell of 4 spacings, %d cells beyond PM_FRESH" % (int(per_cell.max()), int((per_cell > PM_FRESH).sum())))
    assert per_cell.max() > PM_FRESH and per_cell.min() * 7 > PM_WIN
    # the exact mode takes the same points here (every position once): the oracle's set
    assert np.array_equal(r.level == -1, o["level"] == -1)


# ------------------------------------------------------------------------------- GPU: the multi-batch tiler and FAST on hard data
HARD = [("lattice", 0), ("las-cubic", 0), ("stacks", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", HARD)
def test_property_mode_multibatch_on_hard_data(ctx, name, case):
    """Three batches through the tiler (nodes with cached points sample with AlwaysAdhereToMinSpacing): every point stored
    once; inside every node that has a child no two points closer than the node's spacing -- pairs AT the spacing are
    allowed, and the lattice has them."""
    import schwarzwald_amd as swz
    import torch
    from scipy.spatial import cKDTree
    xyz, bounds, cases = family(name)
    sp, mppn = cases[case]
    n = xyz.shape[0]
    pos = O.index_points(xyz, *bounds)[1]
    p = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=mppn, spacing_at_root=sp, flags=swz.FLAG_MIN_DISTANCE_PROPERTY)
    with swz.Tiler(ctx, *bounds, p) as t:
        for part in np.array_split(xyz, 3):
            d = torch.from_numpy(np.ascontiguousarray(part)).cuda()
            torch.cuda.synchronize()
            t.add_batch_device(d.data_ptr(), part.shape[0])
        t.finalize()
        info = t.info()
        table = t.node_table()
        ids = torch.empty(int(info["num_stored"]), dtype=torch.int32, device="cuda")
        t.export_device(0, ids.data_ptr(), 0)
        ids = ids.cpu().numpy().view(np.uint32)
    assert info["num_stored"] == n and np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32))
    keyset = {(int(l), int(k)) for l, k in zip(table["level"], table["key"])}
    checked = ties = 0
    for j in range(len(table["level"])):
        L, key = int(table["level"][j]), int(table["key"][j])
        if L >= 20 or not any((L + 1, key | (o << (3 * (19 - L)))) in keyset for o in range(8)):
            continue
        mine = ids[int(table["offset"][j]):int(table["offset"][j] + table["count"][j])]
        pts = pos[mine]
        s, sq = _level_spacing(sp, L)
        pairs = cKDTree(pts).query_pairs(s * (1.0 + 1e-9), output_type="ndarray")
        if pairs.size:
            d2 = _sq_dist(pts[pairs[:, 0]], pts[pairs[:, 1]])
            bad = np.flatnonzero(d2 < sq)
            assert bad.size == 0, "node (%d, %#x): points %d and %d at d^2 = %r < %r" % (
                L, key, int(mine[pairs[bad[0], 0]]), int(mine[pairs[bad[0], 1]]), float(d2[bad[0]]), sq)
            ties += int((d2 == sq).sum())
        checked += 1
    print("%s in three batches: %d nodes with children checked, %d pairs exactly at their node's spacing" % (name, checked, ties))
    assert checked > 0
    if name == "lattice":
        assert ties > 0


def _check_fast(name, r, sp, mppn, start):
    """(a) and (b) on what FAST samples: the start nodes (node level start - 1) and everything below them like any tiling, and
    the reconstruction above them -- the node of level lv - 1 samples what its children stored (the start nodes' own points,
    further up the points with bit lv + 1 of dup), whatever their number (AlwaysAdhereToMinSpacing), and marks what it takes
    with bit lv (Sampling.h:477-542 as restated in md_fast_ref.tile).  On these clouds the start nodes are small enough to
    take everything: the sampling happens in the reconstruction."""
    pos = r.xyz_clamped[r.perm]
    a, b = _check_property(r.keys, r.level, pos, sp, mppn, _property_levels(name, r), min_level=start - 1)
    ra = rb = 0
    for lv in range(start - 1, -1, -1):
        offered = (r.level == start - 1) if lv == start - 1 else ((r.dup >> np.uint32(lv + 1)) & np.uint32(1)).astype(bool)
        taken = ((r.dup >> np.uint32(lv)) & np.uint32(1)).astype(bool)
        assert offered.any() and not (taken & ~offered).any(), lv
        # as a tiling of its own: what the node was offered is active at its level, what it took has that level
        as_level = np.where(offered, np.where(taken, lv - 1, lv), -100).astype(np.int16)
        x, y = _check_property(r.keys, as_level, pos, sp, 0, lv - 1, min_level=lv - 1)
        ra, rb = ra + x, rb + y
    assert ra > 0 and rb > 0 and a + ra > 0 and b + rb > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", HARD)
def test_property_mode_fast_on_hard_data(ctx, capfd, name, case):
    """FAST with two start nodes' worth of concurrency: the flag survives the reconstruction (with no level called sparse, the trace
    shows the rounds or the coloured phases), nothing is sampled above the start level, and the properties hold from
    the start level down."""
    import schwarzwald_amd as swz
    xyz, bounds, cases = family(name)
    sp, mppn = cases[case]
    p = swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=mppn, spacing_at_root=sp, strategy=swz.FAST, fast_concurrency=2,
                       flags=swz.FLAG_MIN_DISTANCE_PROPERTY)
    r = ctx.tile(xyz, *bounds, p)
    start = r.stats["fast_start_levels"]
    assert start >= 1 and int(r.level.min()) >= start - 1
    _check_fast(name, r, sp, mppn, start)
    capfd.readouterr()
    forced = _with(ctx, {"SWZ_MD_SPARSE_LIMIT": "0", "SWZ_DEBUG": "1"}, lambda: ctx.tile(xyz, *bounds, p))
    trace = _parse(capfd.readouterr().err)
    assert any(t["path"] in ("rounds", "phases") for t in trace.values()), trace   # (the two property-mode algorithms)
    assert forced.stats["fast_start_levels"] == start and int(forced.level.min()) >= start - 1
    _check_fast(name, forced, sp, mppn, start)
