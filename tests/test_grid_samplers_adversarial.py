"""GRID_CENTER and JITTERED on the data that real point clouds are made of and random doubles never produce: lattices that are
symmetric about the cell centres (every point of a cell at the same distance: the FIRST of the minima must win), millimetre
records at UTM offsets (ties in real numbers that the rounding of the coordinates decides), offsets from the target that are
exact in doubles and permuted between two points (only the last bit of the sum decides: what an FMA changes), runs of one grid
cell placed against the edges of the kernels' tiles (1024 points in grid_argmin_keys_kernel, 512 in grid_argmin_kernel), points
on cell faces, on the targets and on the bounds, and JITTERED where its cell count flips from one power of two to the next.
Every decision path -- keys, keys with every run through the exact pass, positions, the box tables, FAST reconstruction, the
multi-batch tiler, the per-node sample_points entry -- must give the oracle's result point for point.

The CPU tests at the top check that each generator really produces its hard case, and hold the oracle (which no reference
vector pins for these two samplers) against an independent NumPy characterisation on the same data."""
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = [O.GRID_CENTER, O.JITTERED]
NAMES = {O.GRID_CENTER: "GRID_CENTER", O.JITTERED: "JITTERED"}
UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
KEY_TILE, POS_TILE = 1024, 512   # points per block of grid_argmin_keys_kernel / grid_argmin_kernel (checked below)


# ------------------------------------------------------------------------------------------- the NumPy characterisation
# (copies of the helpers of tests/test_oracle_properties.py, split into "targets" and "first of the minima" so that the
# generators below can ask where a cell's target is)
def _compact3(v):
    out = np.zeros_like(v)
    for b in range(21):
        out |= ((v >> np.uint64(3 * b)) & np.uint64(1)) << np.uint64(b)
    return out


@functools.lru_cache(maxsize=None)
def _jitter_tables():
    text = open(os.path.join(ROOT, "oracle", "jitter_tables.inc")).read()
    out = {}
    for w in (16, 32, 64):
        body = text.split("SWZ_JITTER_TABLE(%d)" % w)[1].split("};")[0]
        nums = [int(x) for x in re.findall(r"\b\d+\b", body)]
        out[w] = np.array(nums[-16 * w:], dtype=np.int64).reshape(16, w)
    return out


def _jitter_offsets(gx, gy, gz, cells, node_level):
    """JitteredSampling's permutation entry per axis (0 .. cells - 1) of the grid cell (gx, gy, gz), Sampling.h:669-739."""
    tab = _jitter_tables()[16 if cells <= 16 else (32 if cells <= 32 else 64)]
    plen = min(cells, 64)
    start = (3 * (node_level + 1)) % 16
    return (tab[start][(gy + gz) % plen] - 1, tab[(start + 1) % 16][(gx + gz) % plen] - 1,
            tab[(start + 2) % 16][(gx + gy) % plen] - 1)


def _prev_pow2(x):
    x = int(x)
    for s in (1, 2, 4, 8, 16):
        x |= x >> s
    return x - (x >> 1)


def _chain_bounds(keys, bmin, bmax, depth):
    """get_octant_bounds iterated by get_bounds_from_morton_index (OctreeAlgorithms.cpp:3-18, .h:104-116), per point."""
    n = len(keys)
    lo = np.tile(np.asarray(bmin, dtype=np.float64), (n, 1))
    hi = np.tile(np.asarray(bmax, dtype=np.float64), (n, 1))
    for level in range(depth):
        octant = (keys >> np.uint64(3 * (20 - level))) & np.uint64(7)
        half = (hi - lo) / 2.0
        for axis, bit in ((0, 4), (1, 2), (2, 1)):
            up = (octant & np.uint64(bit)) != 0
            lo[:, axis] = np.where(up, lo[:, axis] + half[:, axis], lo[:, axis])
        hi = lo + half
    return lo, hi


def _targets_unit(keys, sampler, node_level, spacing_at_root):
    """(cell id, target) per point of a node of the UNIT cube: every box edge is a dyadic rational there, so the closed forms
    below are exact whatever the order of evaluation.  None when JITTERED has fewer than 16 cells."""
    s_node = float(np.float32(spacing_at_root)) / 2.0 ** (node_level + 1)
    node_ext = 0.5 ** (node_level + 1)
    if sampler == O.GRID_CENTER:
        grid_level = max(-1, int(np.floor(np.log2(np.float32(1.0 / s_node)))) - 1)
    else:
        cells = _prev_pow2(np.uint32(node_ext / s_node))
        if cells < 16:
            return None
        grid_level = node_level + int(np.log2(cells))
    cell = keys >> np.uint64(3 * (20 - grid_level)) if grid_level >= 0 else np.zeros_like(keys)
    gx, gy, gz = _compact3(cell >> np.uint64(2)), _compact3(cell >> np.uint64(1)), _compact3(cell)
    size = 0.5 ** (grid_level + 1)
    if sampler == O.GRID_CENTER:
        t = np.stack([(gx + 0.5) * size, (gy + 0.5) * size, (gz + 0.5) * size], axis=1)
    else:
        m = np.uint64(cells - 1)
        px, py, pz = _jitter_offsets((gx & m).astype(np.int64), (gy & m).astype(np.int64), (gz & m).astype(np.int64), cells, node_level)
        perm_size = size / cells
        t = np.stack([gx * size + px * perm_size, gy * size + py * perm_size, gz * size + pz * perm_size], axis=1)
    return cell, t


def _targets_in_bounds(keys, sampler, node_level, spacing_at_root, bmin, bmax):
    """The same in any bounds, in the reference's order of operations (Sampling.h:314-416 GRID_CENTER, :598-759 JITTERED):
    the boxes come out of the halving chain, never out of a closed form.  All keys share the node's prefix."""
    s_node = float(np.float32(spacing_at_root)) / 2.0 ** (node_level + 1)
    ext_x_root = float(bmax[0]) - float(bmin[0])
    if sampler == O.GRID_CENTER:
        grid_level = max(-1, int(np.floor(np.log2(np.float32(ext_x_root / s_node)))) - 1)
        lo, hi = _chain_bounds(keys, bmin, bmax, grid_level + 1)
        t = lo + (hi - lo) / 2.0
    else:
        nlo, nhi = _chain_bounds(keys[:1], bmin, bmax, node_level + 1)
        ext_x = float(nhi[0, 0] - nlo[0, 0])
        cells = _prev_pow2(np.uint32(ext_x / s_node))
        if cells < 16:
            return None
        levels = int(np.log2(cells))
        grid_level = node_level + levels
        rel = (keys >> np.uint64(3 * (20 - grid_level))) & np.uint64((1 << (3 * levels)) - 1)
        gx, gy, gz = (_compact3(rel >> np.uint64(2)).astype(np.int64), _compact3(rel >> np.uint64(1)).astype(np.int64),
                      _compact3(rel).astype(np.int64))
        px, py, pz = _jitter_offsets(gx, gy, gz, cells, node_level)
        cell_size = ext_x / cells
        perm_size = cell_size / cells
        g = np.stack([gx, gy, gz], axis=1).astype(np.float64)
        p = np.stack([px, py, pz], axis=1).astype(np.float64)
        t = nlo[0] + (g * cell_size + p * perm_size)
    cell = keys >> np.uint64(3 * (20 - grid_level)) if grid_level >= 0 else np.zeros_like(keys)
    return cell, t


def _jitter_cell_count(keys, node_level, spacing_at_root, bounds):
    """JITTERED's cells a side in the node of keys[0]: prev_pow2((uint32)(extent.x / spacing)), Sampling.h:621-640."""
    nlo, nhi = _chain_bounds(keys[:1], bounds[0], bounds[1], node_level + 1)
    s_node = float(np.float32(spacing_at_root)) / 2.0 ** (node_level + 1)
    return _prev_pow2(np.uint32(float(nhi[0, 0] - nlo[0, 0]) / s_node))


def _sq_dist(a, b):
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _runs(cell):
    starts = np.flatnonzero(np.r_[True, cell[1:] != cell[:-1]])
    return starts, np.r_[starts[1:], len(cell)]


def _first_minima(cell, d2):
    """(taken flags, number of points attaining the minimum per run): the FIRST minimum of every run of equal cell id
    (std::min_element, Sampling.h:392-403 / :741-750)."""
    starts, ends = _runs(cell)
    run = np.cumsum(np.r_[True, cell[1:] != cell[:-1]]) - 1
    at_min = d2 == np.minimum.reduceat(d2, starts)[run]
    idx = np.flatnonzero(at_min)
    first = idx[np.r_[True, run[idx][1:] != run[idx][:-1]]]
    taken = np.zeros(len(cell), dtype=bool)
    taken[first] = True
    return taken, np.add.reduceat(at_min.astype(np.int64), starts)


def _expected_grid_sample(keys, pos, sampler, node_level, spacing_at_root):
    cell, t = _targets_unit(keys, sampler, node_level, spacing_at_root)
    return _first_minima(cell, _sq_dist(pos, t))[0]


def _expected_grid_sample_in_bounds(keys, pos, sampler, node_level, spacing_at_root, bmin, bmax):
    cell, t = _targets_in_bounds(keys, sampler, node_level, spacing_at_root, bmin, bmax)
    return _first_minima(cell, _sq_dist(pos, t))[0]


def _sorted(xyz, bounds):
    keys, clamped = O.index_points(xyz, *bounds)
    order = O.sort_by_key(keys)
    return keys[order], order, clamped


def _node_slice(ks, level, at):
    """(indices, node key) of the node at `level` that holds the sorted point `at` (the root: everything)."""
    if level < 0:
        return np.arange(len(ks)), 0
    sh = np.uint64(3 * (20 - level))
    return np.flatnonzero((ks >> sh) == (ks[at] >> sh)), int(ks[at] >> sh) << int(sh)


def _oracle_flags(sampler, ks, order, clamped, node_key, level, bounds, spacing):
    """(status or count, taken flags in Morton order) of the oracle's sample_points, AlwaysAdhereToMinSpacing."""
    cnt, _, i2 = O.sample_points(sampler, 10, ks, order, clamped, node_key, level, *bounds, spacing, O.ALWAYS_ADHERE)
    if cnt < 0:
        return cnt, None
    flags = np.zeros(len(order), dtype=np.uint8)
    where = np.empty(int(order.max()) + 1, dtype=np.int64)
    where[order] = np.arange(len(order))
    flags[where[i2[:cnt]]] = 1
    # the partition is stable: taken points first, the rest behind, both in Morton order
    assert np.array_equal(i2[:cnt], order[flags == 1]) and np.array_equal(i2[cnt:], order[flags == 0])
    return cnt, flags


# ----------------------------------------------------------------------------------------------------------- data families
# 1. symmetric lattice ------------------------------------------------------------------------------------------------
LATTICE = ([0.0, 0.0, 0.0], [64.0, 64.0, 64.0])


@functools.lru_cache(maxsize=None)
def _symmetric_lattice():
    """The 64^3 points at integer + 0.5 in [0, 64]^3, shuffled: in grid cells 2 or 4 units wide every cell holds a set of
    points that is symmetric about its centre."""
    rng = np.random.default_rng(101)
    g = np.arange(64, dtype=np.float64) + 0.5
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return xyz[rng.permutation(xyz.shape[0])]


# 2. millimetre records at UTM offsets --------------------------------------------------------------------------------
LAS_OFFSET = np.array([500000.0, 5400000.0, 200.0])
LAS_SIDE = 262.144   # 2^18 mm: 256 cells of 1.024 m, their centres on half millimetres
LAS_BOUNDS = (LAS_OFFSET.tolist(), (LAS_OFFSET + LAS_SIDE).tolist())
# offset + 262.144 rounds differently on each axis: the three extents of LAS_BOUNDS differ in their last bits (GRID_CENTER weighs
# the axes, JITTERED decides on positions).  With the side rounded to 2^-29 (6e-10 shorter) the sums are exact and the bounds
# are a cube to the bit: both samplers on keys, and the pairs below tie to 1e-9 of a key cell instead of exactly.
LAS_SIDE_EXACT = float(np.round(LAS_SIDE * 2.0 ** 29) / 2.0 ** 29)
LAS_CUBE = (LAS_OFFSET.tolist(), (LAS_OFFSET + LAS_SIDE_EXACT).tolist())
LAS_CELL_MM = 1024
# float(1.024) is a little more than 1.024: extent / spacing falls short of 256 and JITTERED, which truncates it, would take
# 128 cells a side (GRID_CENTER rounds log2f and takes 256); one float less gives both the 1.024 m grid
MM_SPACING = {O.GRID_CENTER: 1.024, O.JITTERED: float(np.nextafter(np.float32(1.024), np.float32(0.0)))}


@functools.lru_cache(maxsize=None)
def _mm_tie_records():
    """Integer millimetre records: per occupied 1.024 m cell one point at centre + (a, b, c) mm, one at centre +
    (+-a', +-b', +-c') with (a', b', c') a permutation of (a, b, c) -- the same distance in real numbers -- and one farther
    away.  (The centre sits on a half millimetre: the records are kept doubled, in half millimetres, for the exact sums.)"""
    rng = np.random.default_rng(11)
    cells = np.unique(rng.integers(0, 256, size=(32000, 3)), axis=0)
    k = len(cells)
    a = rng.integers(1, 400, size=(k, 3))
    perm = np.array([rng.permutation(3) for _ in range(k)])
    sign = rng.choice([-1, 1], size=(k, 3))
    c = cells * LAS_CELL_MM + LAS_CELL_MM // 2
    p1 = c + a
    p2 = c + sign * np.take_along_axis(a, perm, 1)
    far = c + rng.integers(401, 511, size=(k, 3)) * rng.choice([-1, 1], size=(k, 3))
    rec = np.vstack([p1, p2, far])
    return rec[rng.permutation(len(rec))]


def _las_decode(rec):
    return rec.astype(np.float64) * 0.001 + LAS_OFFSET   # integer * scale + offset, as LAS decoding computes it


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


def _aabb(xyz):
    return xyz.min(axis=0).tolist(), xyz.max(axis=0).tolist()


# 2b. ties that only the rounding of the sum decides --------------------------------------------------------------------
# (In family 2 the coordinates themselves carry the rounding of the UTM offset: the "tied" distances differ by 1e-10 or so,
# a million times what the last bit of the sum is worth.  Here the offsets from the target are exact in doubles.)
ULP_SPACING = 1.0 / 32.0


@functools.lru_cache(maxsize=None)
def _ulp_tie_cloud(sampler):
    """Unit cube, 32 cells a side: per occupied cell one point at target + (+-a, +-b, +-c), one at target + a permutation of
    it with other signs, one farther away.  a, b, c are multiples of 2^-45 with 37 significant bits: the differences to the
    target (a multiple of 2^-10) are exact, their squares are not, and (a*a + b*b) + c*c against (b*b + c*c) + a*a differ in the
    last bit or not at all -- what an FMA, a different order of the sum or a float would decide differently."""
    rng = np.random.default_rng(202 + sampler)
    g = np.unique(rng.integers(0, 32, size=(24000 if sampler == O.GRID_CENTER else 60000, 3)), axis=0)
    if sampler == O.GRID_CENTER:
        off = np.full(g.shape, 16, dtype=np.int64)
    else:
        off = np.stack(_jitter_offsets(g[:, 0], g[:, 1], g[:, 2], 32, -1), axis=1)
        keep = np.all((off >= 5) & (off <= 27), axis=1)          # (room for the offsets on both sides of the target)
        g, off = g[keep], off[keep]
    k = len(g)
    target = (g * 32 + off) / 1024.0
    a = rng.integers(2 ** 33, 2 ** 37, size=(k, 3)) * 2.0 ** -45      # 0.008 to 0.125 cells
    perm = np.array([rng.permutation(3) for _ in range(k)])
    p1 = target + rng.choice([-1.0, 1.0], size=(k, 3)) * a
    p2 = target + rng.choice([-1.0, 1.0], size=(k, 3)) * np.take_along_axis(a, perm, 1)
    far = rng.random((k, 3))
    near = np.linalg.norm(far - off / 32.0, axis=1) < 0.25
    far[near] = np.where(off[near] < 16, 0.97, 0.03)
    xyz = np.vstack([p1, p2, (g + far) / 32.0])
    return xyz[rng.permutation(len(xyz))]


# 3. runs placed against tile edges -----------------------------------------------------------------------------------
# Unit cube, spacing 1/32: the root's grid has 32 cells a side for both samplers.  At the root every point is active and
# the array the kernels see is the cloud in Morton order, so a run starts at the sum of the populations of the cells before
# it.  (length, slot of the closest point or None, "same" for one position repeated) in Morton order of the cells:
EDGE_SPACING = 1.0 / 32.0
EDGE_RUNS = [
    (1024, None),      # starts at 0, ends on the edge of tile 0: exactly one tile
    (2048, None),      # 1024: exactly two tiles
    (1, None),         # 3072: starts on an edge
    (1022, None),      # 3073: start = 1 mod 1024 (and mod 512); ends at 4095
    (4097, 0),         # 4095: starts on the LAST slot of a tile, covers four whole tiles, ends on an edge; winner = first slot
    (4607, 4606),      # 8192: starts on an edge; winner = last slot; ends at 12799 = 511 mod 512
    (4200, 100),       # 12799: starts on the last slot of a 512-tile; winner in the first tile it touches
    (4300, 2000),      # 16999: winner in a middle tile
    (4400, 4390),      # 21299: winner in the last tile, not in the last slot
    (5021, "same"),    # 25699: one position 5021 times, ends on 30720 = 30 * 1024
    (1, None),         # 30720
    (510, None),       # 30721: start = 1; ends at 31231 = 511 mod 512
    (2, None),         # 31231: starts on the last slot of a 512-tile, ends inside the next
]
EDGE_FILL = 30000      # then small runs, and a last run that brings the total to 1 mod 1024


@functools.lru_cache(maxsize=None)
def _tile_edge_cloud(sampler):
    """-> (xyz shuffled, the run lengths in Morton order).  The closest point of a run with a slot is the only point within
    0.3 cells of the run's target (a point within 0.002 cells of it), with exactly `slot` of the others before it in Morton
    order."""
    rng = np.random.default_rng(303 + sampler)
    cellno = np.arange(32 ** 3, dtype=np.uint64)
    g = np.stack([_compact3(cellno >> np.uint64(2)), _compact3(cellno >> np.uint64(1)), _compact3(cellno)], axis=1).astype(np.int64)
    if sampler == O.GRID_CENTER:
        target = g + 0.5                                                    # (in cells)
    else:
        target = g + np.stack(_jitter_offsets(g[:, 0], g[:, 1], g[:, 2], 32, -1), axis=1) / 32.0
    lengths = list(EDGE_RUNS)
    fill = 0
    while fill < EDGE_FILL:
        lengths.append((int(rng.integers(1, 41)), None))
        fill += lengths[-1][0]
    total = sum(l for l, _ in lengths)
    lengths.append((600 + (1 - (total + 600)) % KEY_TILE, None))
    parts, counts, c = [], [], 0
    for length, slot in lengths:
        while True:
            lo, t = g[c].astype(np.float64), target[c]
            c += 1
            if slot is None:
                pts = lo + rng.random((length, 3))
            elif slot == "same":
                pts = np.repeat(lo + rng.random((1, 3)), length, axis=0)
            else:
                # (just below the target when few points go before it -- most of the cell then follows it in Morton order --,
                # just above otherwise)
                w = t + (-0.001 if slot < length // 2 else 0.001) * (1.0 + rng.random(3))
                if np.any(np.floor(w) != lo):
                    continue                                               # (the target sits on a face of its cell: the next cell)
                cand = lo + rng.random((8 * length, 3))
                cand = cand[np.linalg.norm(cand - t, axis=1) > 0.3]
                keys, _ = O.index_points(np.vstack([w[None], cand]) / 32.0, *UNIT)
                before, after = cand[keys[1:] < keys[0]], cand[keys[1:] > keys[0]]
                if len(before) < slot or len(after) < length - 1 - slot:
                    continue                                               # (the target sits in a corner: the next cell)
                pts = np.vstack([before[:slot], w[None], after[:length - 1 - slot]])
            break
        parts.append(pts / 32.0)
        counts.append(length)
    xyz = np.vstack(parts)
    return xyz[rng.permutation(len(xyz))], counts


# 4. faces, targets, bounds -------------------------------------------------------------------------------------------
FACE_SPACING = 1.0 / 32.0
EMPTY_SLAB = 13        # z cell kept free of everything but the pairs that share one key cell


@functools.lru_cache(maxsize=None)
def _faces_and_targets():
    """Unit cube, 32 cells a side at the root for both samplers: points on cell faces, on the upper faces of the bounds, on the
    targets of both samplers (some twice), pairs alone in a grid cell inside ONE key cell, and outliers beyond the bounds."""
    rng = np.random.default_rng(404)
    back = rng.random((40000, 3))
    faces = rng.random((6000, 3))
    snap = rng.random((6000, 3)) < 0.5
    snap[~snap.any(axis=1), 0] = True
    faces = np.where(snap, np.floor(faces * 32.0) / 32.0, faces)
    upper = rng.random((2000, 3))
    on = rng.random((2000, 3)) < 0.4
    on[~on.any(axis=1), 2] = True
    upper = np.where(on, 1.0, upper)
    gc = rng.integers(0, 32, size=(3000, 3))
    centres = (gc + 0.5) / 32.0
    gj = rng.integers(0, 32, size=(3000, 3))
    jit = (gj + np.stack(_jitter_offsets(gj[:, 0], gj[:, 1], gj[:, 2], 32, -1), axis=1) / 32.0) / 32.0
    outl = rng.random((1000, 3))
    beyond = rng.random((1000, 3)) < 0.4
    beyond[~beyond.any(axis=1), 1] = True
    outl = np.where(beyond, np.where(rng.random((1000, 3)) < 0.5, -0.5 * rng.random((1000, 3)), 1.0 + 0.5 * rng.random((1000, 3))), outl)
    rest = np.vstack([back, faces, upper, centres, centres[:500], jit, jit[:500], outl])
    zc = np.floor(np.clip(rest[:, 2], 0.0, 1.0) * 32.0)
    rest = rest[zc != EMPTY_SLAB]
    # pairs: two positions of one key cell (2^-21 wide), nothing else in their grid cell
    pc = rng.permutation(1024)[:500]
    cell = np.stack([pc // 32, pc % 32, np.full(500, EMPTY_SLAB)], axis=1)
    kc = cell * 65536 + rng.integers(0, 65536, size=(500, 3))
    pairs = np.vstack([(kc + 0.25 + 0.5 * rng.random((500, 3))) / 2097152.0, (kc + 0.25 + 0.5 * rng.random((500, 3))) / 2097152.0])
    xyz = np.vstack([rest, pairs])
    return xyz[rng.permutation(len(xyz))]


# 5. JITTERED where its cell count flips ------------------------------------------------------------------------------
BOX_LO, BOX_SIDE = [-7.123456789, 100.000001, 3.3333333], 17.71717171
BOX = (BOX_LO, [b + BOX_SIDE for b in BOX_LO])   # (a chain that rounds: test_gpu_parity.py::test_grid_samplers_box_table_depths)
EDGE_CELLS = [16, 32, 64, 128]


def _edge_spacings(bounds, cells):
    """The float spacing nearest to extent.x / cells and its two neighbours, finest first."""
    s = np.float32((bounds[1][0] - bounds[0][0]) / cells)
    return [float(np.nextafter(s, np.float32(0.0))), float(s), float(np.nextafter(s, np.float32(np.inf)))]


@functools.lru_cache(maxsize=None)
def _flip_cloud(which):
    bounds = UNIT if which == "unit" else BOX
    rng = np.random.default_rng(505)
    lo, hi = np.array(bounds[0]), np.array(bounds[1])
    u = np.vstack([rng.random((50000, 3)), 0.37 + 0.01 * rng.standard_normal((10000, 3))]).clip(0.0, 1.0)
    u[::13] = u[rng.integers(0, 500, len(u[::13]))]        # exact duplicates
    return lo + u * (hi - lo), bounds


# the families that go through the whole matrix: name -> (xyz, bounds, {sampler: [(spacing_at_root, max_points_per_node)]})
@functools.lru_cache(maxsize=None)
def family(name, sampler):
    if name == "lattice":
        # (4.0: the root's cells 4 wide, level 0's 2 wide, level 1's hold one point each; 2.0: 2 wide at the root)
        return _symmetric_lattice(), LATTICE, [(4.0, 500), (2.0, 40000)]
    if name in ("mm-ties", "mm-ties-cube"):
        return _las_decode(_mm_tie_records()), LAS_BOUNDS if name == "mm-ties" else LAS_CUBE, [(MM_SPACING[sampler], 300)]
    if name == "ulp-ties":
        return _ulp_tie_cloud(sampler), UNIT, [(ULP_SPACING, 300)]
    if name in ("las-cubic", "las-aabb"):
        xyz = _las_decode(_las_records(3))
        bounds = LAS_BOUNDS if name == "las-cubic" else _aabb(xyz)
        return xyz, bounds, [(O.spacing_from_diagonal(*bounds, 250), 2000)]
    if name == "tile-edges":
        return _tile_edge_cloud(sampler)[0], UNIT, [(EDGE_SPACING, 20000)]
    if name == "faces":
        return _faces_and_targets(), UNIT, [(FACE_SPACING, 1000)]
    if name == "flip":
        xyz, bounds = _flip_cloud("box")
        return xyz, bounds, [(_edge_spacings(bounds, 16)[0], 400), (_edge_spacings(bounds, 64)[2], 1500)]
    raise KeyError(name)


FAMILIES = ["lattice", "mm-ties", "mm-ties-cube", "ulp-ties", "las-cubic", "las-aabb", "tile-edges", "faces", "flip"]


@functools.lru_cache(maxsize=None)
def _oracle(name, sampler, case, strategy=O.ACCURATE, concurrency=8):
    xyz, bounds, cases = family(name, sampler)
    sp, mppn = cases[case]
    return O.tile(xyz, *bounds, sampler, mppn, sp, strategy=strategy, fast_concurrency=concurrency)


# --------------------------------------------------------------------------------------------------------- CPU: premises
def _check_against_numpy(xyz, bounds, sampler, level, spacing, at=None, unit=False):
    """Oracle against the characterisation for one node; returns (count taken, minima per run)."""
    ks, order, clamped = _sorted(xyz, bounds)
    sel, node_key = _node_slice(ks, level, len(ks) // 3 if at is None else at)
    cnt, flags = _oracle_flags(sampler, ks[sel], order[sel], clamped, node_key, level, bounds, spacing)
    pos = clamped[order[sel]]
    cell, t = (_targets_unit(ks[sel], sampler, level, spacing) if unit
               else _targets_in_bounds(ks[sel], sampler, level, spacing, *bounds))
    want, ties = _first_minima(cell, _sq_dist(pos, t))
    assert cnt == int(want.sum())
    bad = np.flatnonzero(flags != want)
    assert bad.size == 0, "%s level %d spacing %r: %d points differ from the characterisation, first at %d" % (
        NAMES[sampler], level, spacing, bad.size, bad[0])
    return cnt, ties


def test_symmetric_lattice_ties_in_every_cell():
    """Family 1: every GRID_CENTER cell of the root has a tied minimum (8 points at 0.75 from the centre of a cell 2 wide, the
    8 innermost of 64 in a cell 4 wide), the oracle takes one point per cell and it is the first of the tied ones; JITTERED
    (targets on multiples of 1/16 or 1/4) ties in at least 1000 cells."""
    xyz = _symmetric_lattice()
    for spacing, cells in ((2.0, 32768), (4.0, 4096)):
        cnt, ties = _check_against_numpy(xyz, LATTICE, O.GRID_CENTER, -1, spacing)
        assert cnt == cells and len(ties) == cells
        assert int((ties >= 2).sum()) == cells and int(ties.min()) == 8
    tied = {}
    for spacing in (2.0, 4.0):
        cnt, ties = _check_against_numpy(xyz, LATTICE, O.JITTERED, -1, spacing)
        tied[spacing] = int((ties >= 2).sum())
    print("JITTERED cells with a shared minimum, by spacing:", tied)
    assert min(tied.values()) >= 1000
    # an inner node: level 0 under a root spacing of 4.0 has cells 2 wide again (16 a side: PERMUTATIONS_16)
    for sampler in SAMPLERS:
        cnt, ties = _check_against_numpy(xyz, LATTICE, sampler, 0, 4.0)
        assert cnt == 4096 and int((ties >= 2).sum()) >= (4096 if sampler == O.GRID_CENTER else 100)


def test_mm_records_tie_in_real_numbers_and_rounding_decides():
    """Family 2: in exact integer arithmetic the two nearest points of (almost) every cell tie; as doubles at (5e5, 5.4e6, 200)
    most of these pairs differ and some stay equal -- both kinds by the thousand."""
    rec = _mm_tie_records()
    xyz = _las_decode(rec)
    cell = rec // LAS_CELL_MM
    cid = (cell[:, 0] * 1000 + cell[:, 1]) * 1000 + cell[:, 2]
    d_exact = ((2 * rec - (2 * cell * LAS_CELL_MM + LAS_CELL_MM)) ** 2).sum(axis=1)       # (in half millimetres, squared)
    o = np.lexsort((d_exact, cid))
    first = np.flatnonzero(np.r_[True, cid[o][1:] != cid[o][:-1]])
    tie = (cid[o][first + 1] == cid[o][first]) & (d_exact[o][first + 1] == d_exact[o][first])
    ks, order, clamped = _sorted(xyz, LAS_BOUNDS)
    assert np.array_equal(clamped, xyz)
    _, t = _targets_in_bounds(ks, O.GRID_CENTER, -1, 1.024, *LAS_BOUNDS)
    d2 = np.empty(len(xyz))
    d2[order] = _sq_dist(xyz[order], t)
    a, b = o[first[tie]], o[first[tie] + 1]
    differ, equal = int((d2[a] != d2[b]).sum()), int((d2[a] == d2[b]).sum())
    print("%d cells, %d tied in integers: %d differ as doubles, %d equal" % (len(first), int(tie.sum()), differ, equal))
    assert int(tie.sum()) >= 10000 and differ >= 1000 and equal >= 1000
    assert len({h - l for l, h in zip(*LAS_BOUNDS)}) == 3 and len({h - l for l, h in zip(*LAS_CUBE)}) == 1
    for bounds in (LAS_BOUNDS, LAS_CUBE):
        for sampler in SAMPLERS:
            cnt, _ = _check_against_numpy(xyz, bounds, sampler, -1, MM_SPACING[sampler])
            assert cnt == len(first)                  # the grid is the 1.024 m one: a point per occupied cell
        _check_against_numpy(xyz, bounds, O.GRID_CENTER, 1, 4.096)          # (an inner node whose cells are the same)


def _ulps_apart(x, y):
    return np.abs(x.view(np.int64) - y.view(np.int64))


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_permuted_offsets_tie_to_the_last_bit(sampler):
    """Family 2b: the two nearest points of every cell are at the same distance in real numbers and at most a few units in
    the last place apart as doubles; thousands of cells of either kind -- equal, and unequal by rounding alone."""
    xyz = _ulp_tie_cloud(sampler)
    ks, order, clamped = _sorted(xyz, UNIT)
    assert np.array_equal(clamped, xyz)
    cnt, ties = _check_against_numpy(xyz, UNIT, sampler, -1, ULP_SPACING, unit=True)
    cell, t = _targets_unit(ks, sampler, -1, ULP_SPACING)
    pos = xyz[order]
    d2 = _sq_dist(pos, t)
    starts, ends = _runs(cell)
    assert np.all(ends - starts == 3) and cnt == len(starts)
    nearest = np.argsort(d2.reshape(-1, 3), axis=1)[:, :2] + starts[:, None]
    for j in (0, 1):                                                   # the differences to the target are exact
        q, tq = pos[nearest[:, j]], t[nearest[:, j]]
        assert np.array_equal((q - tq) + tq, q) and np.all(np.abs(q - tq) * 2.0 ** 45 == np.rint(np.abs(q - tq) * 2.0 ** 45))
    assert np.array_equal(np.sort(np.abs(pos[nearest[:, 0]] - t[nearest[:, 0]]), axis=1),
                          np.sort(np.abs(pos[nearest[:, 1]] - t[nearest[:, 1]]), axis=1))   # ... and permutations of one another
    two = np.sort(d2.reshape(-1, 3), axis=1)[:, :2]
    apart = _ulps_apart(two[:, 0].copy(), two[:, 1].copy())
    equal, differ = int((apart == 0).sum()), int((apart > 0).sum())
    print("%s: %d cells, the two nearest equal in %d, apart by rounding in %d (at most %d ulp)" % (
        NAMES[sampler], len(starts), equal, differ, int(apart.max())))
    assert int(apart.max()) <= 4 and equal >= 1000 and differ >= 1000
    assert int((ties == 2).sum()) == equal


def test_las_surface_is_quantised_at_utm_offsets():
    rec = _las_records(3)
    xyz = _las_decode(rec)
    assert np.array_equal(np.rint((xyz - LAS_OFFSET) / 0.001).astype(np.int64), rec)
    inside = np.all((xyz >= LAS_OFFSET) & (xyz <= LAS_OFFSET + LAS_SIDE), axis=1)
    assert 0 < int((~inside).sum()) < 100                          # (a few returns of the tree blobs lie below the bounds)
    lo, hi = _aabb(xyz)
    assert len({round(h - l, 3) for l, h in zip(lo, hi)}) == 3     # the AABB is no cube: JITTERED decides on positions there
    assert np.unique(rec, axis=0).shape[0] < rec.shape[0]
    for bounds in (LAS_BOUNDS, (lo, hi)):
        sp = O.spacing_from_diagonal(*bounds, 250)
        for sampler in SAMPLERS:
            _check_against_numpy(xyz, bounds, sampler, -1, sp)


def test_tile_sizes_are_what_the_edge_family_aims_at():
    text = open(os.path.join(ROOT, "schwarzwald_amd", "csrc", "swz_grid.hip")).read()
    v = {}
    for short in ("GA_THREADS", "GA_IPT", "GAK_IPT"):
        name = "SWZ_" + short   # (compile-time constants, not options: test_abi_and_host.py looks for quoted option names)
        m = re.search(r"#ifndef %s\s*\n#define %s (\d+)" % (name, name), text)
        assert m, "swz_grid.hip no longer defines %s: tests/test_grid_samplers_adversarial.py must learn the tile sizes anew" % name
        v[short] = int(m.group(1))
    keys, positions = v["GA_THREADS"] * v["GAK_IPT"], v["GA_THREADS"] * v["GA_IPT"]
    assert (keys, positions) == (KEY_TILE, POS_TILE), (
        "the grid samplers' tiles are %d (keys) and %d (positions) points now, the runs of family 3 (EDGE_RUNS) are placed "
        "against tiles of %d and %d: move them" % (keys, positions, KEY_TILE, POS_TILE))


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_tile_edge_runs_are_where_they_should_be(sampler):
    """Family 3: the run starts recomputed from the oracle's sorted keys have every alignment the kernels branch on, and the
    oracle's winners sit in the slots they were built for."""
    xyz, counts = _tile_edge_cloud(sampler)
    ks, order, clamped = _sorted(xyz, UNIT)
    cnt, ties = _check_against_numpy(xyz, UNIT, sampler, -1, EDGE_SPACING, unit=True)
    _, flags = _oracle_flags(sampler, ks, order, clamped, 0, -1, UNIT, EDGE_SPACING)
    cell, _ = _targets_unit(ks, sampler, -1, EDGE_SPACING)
    assert int(cell.max()) < 32 ** 3 and len(np.unique(cell)) == len(counts)
    starts, ends = _runs(cell)
    assert np.array_equal(ends - starts, counts)
    length = ends - starts
    win = np.flatnonzero(flags)
    assert len(win) == len(starts) == cnt
    m = len(ks)
    for tile, residues in ((KEY_TILE, (0, 1, KEY_TILE - 1)), (POS_TILE, (0, 1, POS_TILE - 1))):
        for r in residues:
            assert np.any((starts % tile == r) & (length >= 2)), "no run starts at %d mod %d" % (r, tile)
    assert np.any((ends[:-1] % KEY_TILE == 0))                                        # ends on an edge, the next starts on it
    assert np.any((starts % KEY_TILE == 0) & (length == KEY_TILE)) and np.any((starts % KEY_TILE == 0) & (length == 2 * KEY_TILE))
    whole = ends // KEY_TILE - -(-starts // KEY_TILE)                                 # whole tiles inside the run
    big = (length >= 4000) & (whole >= 3) & (ties == 1)
    first_tile, last_tile = starts // KEY_TILE, (ends - 1) // KEY_TILE
    wt = win // KEY_TILE
    assert np.any(big & (wt == first_tile) & (win > starts))
    assert np.any(big & (wt > first_tile) & (wt < last_tile))
    assert np.any(big & (wt == last_tile) & (win < ends - 1))
    assert np.any(big & (win == starts)) and np.any(big & (win == ends - 1))
    assert np.any(big & (starts % KEY_TILE == KEY_TILE - 1) & (win == starts))        # (a winner alone on a tile's last slot)
    same = np.flatnonzero((length >= 5000) & (ties == length))
    assert same.size == 1 and win[same[0]] == starts[same[0]]
    a, b = starts[same[0]], ends[same[0]]
    assert np.all(ks[a:b] == ks[a]) and np.all(order[a:b][1:] > order[a:b][:-1])       # equal keys: by input index
    assert m % KEY_TILE == 1 and length[-1] >= 3                                       # the last run ends on m = 1 mod 1024 ...
    assert (m - 1) % KEY_TILE == 0 and (m - 1) % POS_TILE == 0                         # ... and, one point shorter, on an edge


def test_faces_targets_and_bounds_are_there():
    """Family 4: every kind survives the encoding."""
    xyz = _faces_and_targets()
    ks, order, clamped = _sorted(xyz, UNIT)
    pos = clamped[order]
    assert int((xyz != clamped).any(axis=1).sum()) >= 900                             # outliers, clamped in place
    assert np.all(clamped >= 0.0) and np.all(clamped <= 1.0)
    kc = np.stack([_compact3(ks >> np.uint64(2)), _compact3(ks >> np.uint64(1)), _compact3(ks)], axis=1).astype(np.int64)
    on_face = (pos * 32.0 == np.floor(pos * 32.0)) & (pos < 1.0)
    assert int(on_face.any(axis=1).sum()) >= 5000
    assert np.all((kc >> 16)[on_face] == (pos * 32.0)[on_face])                       # a face belongs to the upper cell
    on_upper = pos == 1.0
    assert int(on_upper.any(axis=1).sum()) >= 2000 and np.all(kc[on_upper] == 2 ** 21 - 1)
    for sampler in SAMPLERS:
        cnt, ties = _check_against_numpy(xyz, UNIT, sampler, -1, FACE_SPACING, unit=True)
        cell, t = _targets_unit(ks, sampler, -1, FACE_SPACING)
        at_target = _sq_dist(pos, t) == 0.0
        assert int(at_target.sum()) >= 3000 and int((ties >= 2).sum()) >= 300         # (some targets hold two points)
        starts, ends = _runs(cell)
        two = starts[(ends - starts) == 2]
        one_key = two[(ks[two] == ks[two + 1]) & (pos[two] != pos[two + 1]).any(axis=1)]
        assert one_key.size >= 450
        _check_against_numpy(xyz, UNIT, sampler, 0, 2.0 * FACE_SPACING, at=len(ks) - 1, unit=True)


@pytest.mark.parametrize("which", ["unit", "box"])
def test_jittered_cell_count_flips_where_the_characterisation_says(which):
    """Family 5: extent.x / spacing at 16, 32, 64 and 128 and one float either side, at the root and in an inner node: the
    oracle's error for fewer than 16 cells and every taken point are the characterisation's."""
    xyz, bounds = _flip_cloud(which)
    ks, order, clamped = _sorted(xyz, bounds)
    for level in (-1, 1):
        sel, node_key = _node_slice(ks, level, len(ks) // 2)
        for cells in EDGE_CELLS:
            counts = []
            for sp in _edge_spacings(bounds, cells):
                cnt, flags = _oracle_flags(O.JITTERED, ks[sel], order[sel], clamped, node_key, level, bounds, sp)
                counts.append(_jitter_cell_count(ks[sel], level, sp, bounds))
                tgt = (_targets_unit(ks[sel], O.JITTERED, level, sp) if which == "unit"
                       else _targets_in_bounds(ks[sel], O.JITTERED, level, sp, *bounds))
                if counts[-1] < 16:
                    assert tgt is None and cnt == O.ERR_JITTER_GRID_TOO_SMALL, (level, cells, sp)
                    continue
                want, _ = _first_minima(tgt[0], _sq_dist(clamped[order[sel]], tgt[1]))
                assert cnt == int(want.sum()) and np.array_equal(flags == 1, want), (level, cells, sp)
                if which == "unit" and level == -1:
                    assert np.array_equal(want, _expected_grid_sample_in_bounds(ks, clamped[order], O.JITTERED, -1, sp, *bounds))
            # one float below extent / cells the grid has `cells` cells a side, one float above it half as many (in the unit
            # cube the middle one is extent / cells exactly)
            assert counts[0] == cells and counts[2] == cells // 2 and counts[1] in (cells, cells // 2), (level, cells, counts)
            assert which != "unit" or counts[1] == cells


# ----------------------------------------------------------------------------------------------------------- GPU: the matrix
@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


OPTION_NAMES = ("SWZ_GRID_KEYS", "SWZ_GRID_KEYS_SLACK", "SWZ_GRID_TABLE_DEPTH", "SWZ_JITTER_TABLE")


@pytest.fixture(autouse=True)
def _options_cleared(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        for k in OPTION_NAMES:
            c.set_option(k, None)


SINGLE = {
    "default": {},
    "every run through the exact pass": {"SWZ_GRID_KEYS_SLACK": "1e9"},
    "positions": {"SWZ_GRID_KEYS": "0"},
    "no box table": {"SWZ_GRID_TABLE_DEPTH": "0", "SWZ_JITTER_TABLE": "0"},
    "deepest box table": {"SWZ_GRID_TABLE_DEPTH": "6", "SWZ_JITTER_TABLE": "0"},
    "positions, no box table": {"SWZ_GRID_KEYS": "0", "SWZ_GRID_TABLE_DEPTH": "0", "SWZ_JITTER_TABLE": "0"},
}
LEGS = list(SINGLE) + ["FAST 2", "FAST 8", "multi-batch ACCURATE", "multi-batch FAST", "sample_points"]


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


# (copies of the helpers of tests/test_multibatch.py: the same batches through the oracle's tiler and the library's)
def _oracle_files(bounds, xyz, k, sampler, max_points, spacing, strategy, concurrency):
    t = O.Tiler(bounds[0], bounds[1], sampler, max_points, spacing, strategy=strategy, fast_concurrency=concurrency)
    for part in np.array_split(xyz, k):
        st = t.add_batch(part)
        assert st == 0, st
    assert t.finalize() == 0
    ex = t.export()
    c = t.counts()
    t.close()
    return ex, c


def _gpu_files(ctx, bounds, xyz, k, sampler, max_points, spacing, strategy, concurrency):
    import schwarzwald_amd as swz
    import torch
    params = swz.TileParams(sampler=sampler, max_points_per_node=max_points, spacing_at_root=spacing, strategy=strategy,
                            fast_concurrency=concurrency)
    with swz.Tiler(ctx, bounds[0], bounds[1], params) as t:
        for p in np.array_split(xyz, k):
            d = torch.from_numpy(np.ascontiguousarray(p)).cuda()
            torch.cuda.synchronize()
            t.add_batch_device(d.data_ptr(), p.shape[0])
        t.finalize()
        info = t.info()
        table = t.node_table()
        ns = int(info["num_stored"])
        d_keys = torch.empty(max(ns, 1), dtype=torch.int64, device="cuda")
        d_ids = torch.empty(max(ns, 1), dtype=torch.int32, device="cuda")
        d_lvl = torch.empty(max(ns, 1), dtype=torch.int8, device="cuda")
        t.export_device(d_keys.data_ptr(), d_ids.data_ptr(), d_lvl.data_ptr())
        ids = d_ids.cpu().numpy().view(np.uint32)[:ns]
        lvl = d_lvl.cpu().numpy()[:ns]
    return dict(table=table, ids=ids, level=lvl, info=info)


def _compare_files(g, ex, c, what):
    tb = g["table"]
    assert len(tb["level"]) == len(ex["level"]) == c["num_nodes"], what
    assert np.array_equal(tb["level"], ex["level"]) and np.array_equal(tb["key"], ex["key"]), what
    assert np.array_equal(tb["offset"], ex["offset"]) and np.array_equal(tb["count"], ex["count"]), what
    assert np.array_equal(g["ids"], ex["ids"]), what + ": " + _first_difference(g["ids"], ex["ids"])
    assert np.array_equal(g["level"], np.repeat(ex["level"], ex["count"].astype(np.int64))), what


def _sample_points_both(ctx, sampler, ks, order, clamped, node_key, level, bounds, spacing, what):
    import schwarzwald_amd as swz
    cnt, flags = _oracle_flags(sampler, ks, order, clamped, node_key, level, bounds, spacing)
    if cnt < 0:
        assert cnt == O.ERR_JITTER_GRID_TOO_SMALL, what
        with pytest.raises(swz.SwzError) as e:
            ctx.sample_points(sampler, 10, ks, order, clamped, node_key, level, *bounds, spacing, swz.ALWAYS_ADHERE_TO_MIN_SPACING)
        assert e.value.code == 3, what
        return cnt
    got = ctx.sample_points(sampler, 10, ks, order, clamped, node_key, level, *bounds, spacing, swz.ALWAYS_ADHERE_TO_MIN_SPACING)
    assert np.array_equal(got, flags), what + ": " + _first_difference(got, flags)
    return cnt


@pytest.mark.gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("sampler", SAMPLERS, ids=[NAMES[s] for s in SAMPLERS])
@pytest.mark.parametrize("name", FAMILIES)
def test_adversarial_family_matches_oracle(ctx, name, sampler, leg):
    import schwarzwald_amd as swz
    xyz, bounds, cases = family(name, sampler)
    for case, (sp, mppn) in enumerate(cases):
        what = "%s, %s, spacing %r, max_points %d, %s" % (name, NAMES[sampler], sp, mppn, leg)
        if leg in SINGLE:
            o = _oracle(name, sampler, case)
            assert o["status"] == 0 and o["stats"]["max_level"] >= 0, what
            p = swz.TileParams(sampler=sampler, max_points_per_node=mppn, spacing_at_root=sp)
            g = _with(ctx, SINGLE[leg], lambda: ctx.tile(xyz, *bounds, p))
            assert np.array_equal(g.keys, o["keys"]) and np.array_equal(g.perm, o["perm"]), what
            assert np.array_equal(g.level, o["level"]), what + ": " + _first_difference(g.level, o["level"])
            assert g.stats["num_nodes"] == o["stats"]["num_nodes"], what
        elif leg.startswith("FAST"):
            conc = int(leg.split()[1])
            o = _oracle(name, sampler, case, O.FAST, conc)
            assert o["status"] == 0, what
            p = swz.TileParams(sampler=sampler, max_points_per_node=mppn, spacing_at_root=sp, strategy=swz.FAST,
                               fast_concurrency=conc)
            g = ctx.tile(xyz, *bounds, p)
            assert np.array_equal(g.perm, o["perm"]), what
            assert np.array_equal(g.level, o["level"]), what + ": " + _first_difference(g.level, o["level"])
            assert np.array_equal(g.dup, o["dup"]), what
        elif leg.startswith("multi-batch"):
            strategy = O.FAST if leg.endswith("FAST") else O.ACCURATE
            ex, c = _oracle_files(bounds, xyz, 3, sampler, mppn, sp, strategy, 2)
            g = _gpu_files(ctx, bounds, xyz, 3, sampler, mppn, sp, strategy, 2)
            inversions = int(g["info"]["rekey_inversions"]), int(c["unsorted_cached_nodes"])
            print("%s: rekey inversions %d, oracle's unsorted cached nodes %d" % ((what,) + inversions))
            if inversions == (0, 0):
                _compare_files(g, ex, c, what)
            else:
                # quantised positions on key-cell boundaries: a node that re-reads its points against its own bounds may
                # order them differently from the root's keys, where the library sorts and the reference merges unsorted
                # (the documented divergence, see test_multibatch.py::test_gpu_rekey_inversion_is_counted_and_confined and
                # the same branch of test_min_distance_adversarial.py): both must see it, and every point is still stored
                # (ACCURATE: exactly once; FAST, whose copies depend on the decisions: at least once)
                assert min(inversions) > 0, what
                if strategy == O.ACCURATE:
                    assert g["ids"].size == c["num_stored"] == xyz.shape[0], what
                ids = np.sort(g["ids"]) if strategy == O.ACCURATE else np.unique(g["ids"])
                assert np.array_equal(ids, np.arange(xyz.shape[0], dtype=np.uint32)), what
        else:
            ks, order, clamped = _sorted(xyz, bounds)
            for level in (-1, 0):
                # (the spacing a level-0 node of the tiler would see: sample_points halves it per level itself)
                sel, node_key = _node_slice(ks, level, len(ks) - 1)
                cnt = _sample_points_both(ctx, sampler, ks[sel], order[sel], clamped, node_key, level, bounds, sp,
                                          what + ", node level %d" % level)
                assert cnt > 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("leg", list(SINGLE))
@pytest.mark.parametrize("sampler", SAMPLERS, ids=[NAMES[s] for s in SAMPLERS])
def test_tile_edge_runs_through_sample_points(ctx, sampler, leg):
    """Family 3 through the per-node entry, where the number of points is the caller's: the whole cloud (the last run ends on
    m = 1 mod 1024: its last point alone in a tile), one point less (the last run ends with the last tile), and cut inside and
    at the ends of the long runs."""
    xyz, counts = _tile_edge_cloud(sampler)
    ks, order, clamped = _sorted(xyz, UNIT)
    n = len(ks)
    ends = np.cumsum(counts)
    cuts = [n, n - 1, int(ends[4]), int(ends[4]) + 1, int(ends[5]) - 1, int(ends[7]) - 1000, int(ends[9]), int(ends[9]) - 1023]
    for m in cuts:
        what = "tile-edges, %s, %s, the first %d points" % (NAMES[sampler], leg, m)
        _with(ctx, SINGLE[leg], lambda: _sample_points_both(ctx, sampler, ks[:m], order[:m], clamped, 0, -1, UNIT, EDGE_SPACING, what))


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["default", "every run through the exact pass", "positions", "no box table"])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=[NAMES[s] for s in SAMPLERS])
def test_symmetric_lattice_inner_nodes_through_sample_points(ctx, sampler, leg):
    """Family 1 as a root and as inner nodes whose cells are 2 wide: level 0 under a root spacing of 4.0 (JITTERED: 16 cells,
    PERMUTATIONS_16), level 1 under 8.0 (GRID_CENTER; JITTERED has 8 cells there: the error)."""
    xyz = _symmetric_lattice()
    ks, order, clamped = _sorted(xyz, LATTICE)
    for level, sp in ((-1, 2.0), (-1, 4.0), (0, 4.0), (1, 8.0)):
        sel, node_key = _node_slice(ks, level, 5 * len(ks) // 7)
        what = "lattice, %s, %s, node level %d, spacing %r" % (NAMES[sampler], leg, level, sp)
        cnt = _with(ctx, SINGLE[leg], lambda: _sample_points_both(ctx, sampler, ks[sel], order[sel], clamped, node_key, level,
                                                                  LATTICE, sp, what))
        assert cnt == (O.ERR_JITTER_GRID_TOO_SMALL if (sampler, level) == (O.JITTERED, 1) else len(sel) // (64 if sp == 4.0 and level < 0 else 8)), what


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["default", "every run through the exact pass", "positions", "no box table", "deepest box table"])
@pytest.mark.parametrize("which", ["unit", "box"])
def test_jittered_cell_count_flips_like_the_oracle(ctx, which, leg):
    """Family 5 on the GPU: the cell count, the table, the error for fewer than 16 cells and every taken point."""
    xyz, bounds = _flip_cloud(which)
    ks, order, clamped = _sorted(xyz, bounds)
    errors = 0
    for level in (-1, 1):
        sel, node_key = _node_slice(ks, level, len(ks) // 2)
        for cells in EDGE_CELLS:
            for sp in _edge_spacings(bounds, cells):
                what = "flip %s, %s, node level %d, extent / %d, spacing %r" % (which, leg, level, cells, sp)
                cnt = _with(ctx, SINGLE[leg], lambda: _sample_points_both(ctx, O.JITTERED, ks[sel], order[sel], clamped, node_key,
                                                                          level, bounds, sp, what))
                errors += cnt < 0
    assert errors >= 2
