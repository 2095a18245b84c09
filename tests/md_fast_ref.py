"""Expected values for MIN_DISTANCE_FAST (AdaptivePoissonDiskSampling, Sampling.h:477-542, with the densities of
TilerProcess.cpp:500-508).  The oracle does not know this sampler; this is a Python restatement of its rules on the oracle's
primitives (sparse_grid_greedy, index_points, sort_by_key, partition_child_octants, required_morton_index_depth, node bounds
from orc_get_bounds_from_morton_index).  TEST INFRASTRUCTURE ONLY: it never touches the library under test.

sample_points      rules 1-3 of one node
tile               a single batch, ACCURATE (oracle.cpp do_tiling_for_node) or FAST (start nodes + reconstruction, dup_mask)
MultiBatch         the multi-batch ACCURATE tiler (oracle.cpp MBTiler): files re-read, re-keyed, merged, behaviour by cached count
reconstruct_files  FAST finalize of a multi-batch tiler: the levels above the start nodes from the files below them
"""
import numpy as np

import oracle_lib as O

MIN_DISTANCE_FAST = 4
LEVELS = 21


def stride(node_level):
    """nth_point = (uint32_t)std::round(1 / density(node_level))"""
    density = np.float32(0.25) if node_level < 0 else (np.float32(0.5) if node_level < 1 else np.float32(1.0))
    return int(np.round(np.float32(1.0) / density))


def candidate_level(root_extent_x, spacing_at_root, node_level):
    """max(-1, (int)floor(log2f(root_extent.x / spacing_at_this_node)) - 1); the ratio is a double narrowed to float"""
    spacing_at_this_node = float(np.float32(spacing_at_root)) / 2.0 ** (node_level + 1)
    return max(-1, int(np.floor(np.log2(np.float32(root_extent_x / spacing_at_this_node)))) - 1)


def required_depth(node_level, bmin, bmax, spacing_at_root):
    """Sampling.cpp:45-47: the node level, like MIN_DISTANCE (asked of the oracle for that sampler)."""
    return int(O.lib().orc_required_morton_index_depth(O.MIN_DISTANCE, node_level, O._vec3(bmin), O._vec3(bmax),
                                                       O.C.c_float(spacing_at_root)))


def node_bounds(node_key, node_level, bmin, bmax):
    if node_level < 0:
        return list(bmin), list(bmax)
    return O.bounds_from_morton_index(int(node_key), bmin, bmax, node_level + 1)


def sample_points(max_points, keys, idx, xyz, node_key, node_level, bmin, bmax, spacing_at_root,
                  behaviour=O.TAKE_ALL_WHEN_BELOW_MAX):
    """taken flag per element of the node's Morton-sorted range (keys, idx); xyz: the positions idx refers to."""
    n = len(keys)
    taken = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return taken
    if behaviour == O.TAKE_ALL_WHEN_BELOW_MAX and n <= max_points:
        taken[:] = 1
        return taken
    if candidate_level(bmax[0] - bmin[0], spacing_at_root, node_level) == -1:
        taken[0] = 1
        return taken
    cand = np.arange(0, n, stride(node_level))
    nmin, nmax = node_bounds(node_key, node_level, bmin, bmax)
    spacing_at_this_node = float(np.float32(spacing_at_root)) / 2.0 ** (node_level + 1)
    acc = O.sparse_grid_greedy(xyz, np.asarray(idx, dtype=np.uint32)[cand], nmin, nmax, float(np.float32(spacing_at_this_node)))
    taken[cand] = acc
    return taken


def _children(skeys, child_level):
    """(octant, begin, end) of the non-empty child ranges of a sorted key range"""
    off = O.partition_child_octants(skeys, child_level)
    return [(o, off[o], off[o + 1]) for o in range(8) if off[o + 1] > off[o]]


def _shift(level):
    return 3 * (LEVELS - 1 - level)


def tile(xyz, bmin, bmax, max_points, spacing_at_root, max_depth=100, strategy=O.ACCURATE, fast_start_level=None):
    """dict(keys, perm, level, dup, num_nodes, points_visited) like oracle_lib.tile.  FAST needs the start level (the
    oracle's MIN_DISTANCE FAST run of the same input reports it; it does not depend on the sampler)."""
    keys, xc = O.index_points(xyz, bmin, bmax)
    perm = O.sort_by_key(keys)
    skeys = keys[perm]
    n = len(skeys)
    level = np.full(n, -128, dtype=np.int8)
    dup = np.zeros(n, dtype=np.uint32)
    max_level = min(LEVELS - 1, max_depth)
    count = dict(nodes=0, visited=0)

    def do_node(pos, node_key, node_level):
        count["visited"] += len(pos)
        req = required_depth(node_level, bmin, bmax, spacing_at_root)
        assert req == node_level
        count["nodes"] += 1
        if req >= max_level:  # terminal
            level[pos] = node_level
            return
        t = sample_points(max_points, skeys[pos], perm[pos], xc, node_key, node_level, bmin, bmax, spacing_at_root).astype(bool)
        level[pos[t]] = node_level
        rest = pos[~t]
        for o, b, e in _children(skeys[rest], node_level + 1):
            do_node(rest[b:e], int(node_key) | (o << _shift(node_level + 1)), node_level + 1)

    if n == 0:
        return dict(keys=skeys, perm=perm, level=level, dup=dup, num_nodes=0, points_visited=0)
    everything = np.arange(n)
    if strategy == O.ACCURATE:
        do_node(everything, 0, -1)
    else:
        S = int(fast_start_level)
        sh = np.uint64(3 * (LEVELS - S))
        prefix = skeys >> sh
        heads = np.flatnonzero(np.concatenate([[True], prefix[1:] != prefix[:-1]]))
        ends = np.concatenate([heads[1:], [n]])
        for b, e in zip(heads, ends):
            do_node(everything[b:e], int(prefix[b]) << int(sh), S - 1)
        # finalize: every ancestor of a start node samples what its children persisted, AlwaysAdhereToMinSpacing
        stored = [dict() for _ in range(S + 1)]
        for p in np.flatnonzero(level == S - 1):
            stored[S].setdefault(int(prefix[p]), []).append(p)
        for lv in range(S - 1, -1, -1):
            for index in sorted({k >> 3 for k in stored[lv + 1]}):
                data = np.array([p for o in range(8) for p in stored[lv + 1].get((index << 3) | o, [])], dtype=np.int64)
                node_key = 0 if lv == 0 else index << (3 * (LEVELS - lv))
                t = sample_points(max_points, skeys[data], perm[data], xc, node_key, lv - 1, bmin, bmax, spacing_at_root,
                                  O.ALWAYS_ADHERE).astype(bool)
                stored[lv][index] = list(data[t])
                dup[data[t]] |= np.uint32(1 << lv)
                count["nodes"] += 1
    return dict(keys=skeys, perm=perm, level=level, dup=dup, num_nodes=count["nodes"], points_visited=count["visited"])


def _rekey(ids, xyz, node_key, node_level, bmin, bmax):
    """read_pnts_from_disk: the node's own index, the levels below it from an index relative to the NODE's bounds"""
    nmin, nmax = node_bounds(node_key, node_level, bmin, bmax)
    rel, _ = O.index_points(xyz[ids], nmin, nmax)
    return np.uint64(node_key) | (rel >> np.uint64(3 * (node_level + 1)))


def _merge(new_keys, new_ids, old_keys, old_ids):
    """std::merge(new, cached): on equal keys the new points come first"""
    keys = np.concatenate([new_keys, old_keys])
    ids = np.concatenate([new_ids, old_ids])
    order = np.argsort(keys, kind="stable")
    return keys[order], ids[order]


def files_table(files):
    """dict(level, key, offset, count, ids) ordered by (level, key), like oracle_lib.Tiler.export"""
    names = sorted(k for k, v in files.items() if len(v))
    count = np.array([len(files[k]) for k in names], dtype=np.uint64)
    return dict(level=np.array([k[0] for k in names], dtype=np.int8), key=np.array([k[1] for k in names], dtype=np.uint64),
                offset=np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.uint64) if len(names) else count, count=count,
                ids=np.concatenate([files[k] for k in names]).astype(np.uint32) if names else np.zeros(0, np.uint32))


class MultiBatch:
    """ACCURATE over several batches (MBTiler): files[(level, key)] = global ids in file order.  With start_level = S > 0 the
    batches of a FAST tiler (MBTiler::add_batch): every batch is split at its start nodes (node level S - 1), each of which
    is tiled like a root; reconstruct_files(files, xyz, ..., S - 1) then is the finalize.

    A file whose re-keyed points are no longer ascending ends the comparison with the library (which sorts them, where the
    reference merges them as they are): by default that is an assertion; with count_unsorted=True such nodes are counted in
    unsorted_cached_nodes instead (like the oracle's counter), and files is not to be trusted when the count is not zero."""

    def __init__(self, bmin, bmax, max_points, spacing_at_root, max_depth=100, start_level=0, count_unsorted=False):
        self.bmin, self.bmax, self.max_points, self.spacing, self.max_depth = list(bmin), list(bmax), max_points, spacing_at_root, max_depth
        self.start_level, self.count_unsorted = int(start_level), count_unsorted
        self.xyz = np.zeros((0, 3))
        self.files = {}
        self.points_visited = 0
        self.unsorted_cached_nodes = 0

    def add_batch(self, batch):
        batch = np.ascontiguousarray(batch, dtype=np.float64).reshape(-1, 3)
        base = self.xyz.shape[0]
        keys, xc = O.index_points(batch, self.bmin, self.bmax)
        self.xyz = np.vstack([self.xyz, xc])
        if len(keys) == 0:
            return
        perm = O.sort_by_key(keys)
        skeys, ids = keys[perm], (perm + base).astype(np.uint32)
        if self.start_level <= 0:
            self._node(skeys, ids, 0, -1)
            return
        sh = np.uint64(3 * (LEVELS - self.start_level))
        prefix = skeys >> sh
        heads = np.flatnonzero(np.concatenate([[True], prefix[1:] != prefix[:-1]]))
        for b, e in zip(heads, np.concatenate([heads[1:], [len(skeys)]])):
            self._node(skeys[b:e], ids[b:e], int(prefix[b]) << int(sh), self.start_level - 1)

    def _node(self, keys, ids, node_key, node_level):
        cached = np.asarray(self.files.get((node_level, node_key), []), dtype=np.uint32)
        ckeys = _rekey(cached, self.xyz, node_key, node_level, self.bmin, self.bmax) if len(cached) else np.zeros(0, np.uint64)
        if len(ckeys) > 1 and not np.all(ckeys[1:] >= ckeys[:-1]):
            assert self.count_unsorted, "a file read back out of order: choose another input"
            self.unsorted_cached_nodes += 1
        self.points_visited += len(keys) + len(cached)
        max_level = min(LEVELS - 1, self.max_depth)
        if node_level >= max_level:  # terminal: new ++ cached
            self.files[(node_level, node_key)] = list(ids) + list(cached)
            return
        keys, ids = _merge(keys, ids, ckeys, cached)
        behaviour = O.ALWAYS_ADHERE if len(cached) else O.TAKE_ALL_WHEN_BELOW_MAX
        t = sample_points(self.max_points, keys, ids, self.xyz, node_key, node_level, self.bmin, self.bmax, self.spacing,
                          behaviour).astype(bool)
        if t.any():
            self.files[(node_level, node_key)] = list(ids[t])
        rk, ri = keys[~t], ids[~t]
        for o, b, e in _children(rk, node_level + 1):
            self._node(rk[b:e], ri[b:e], int(node_key) | (o << _shift(node_level + 1)), node_level + 1)


def reconstruct_files(files, xyz, bmin, bmax, max_points, spacing_at_root, lowest_given_level, unsorted=None):
    """FAST finalize on node files: files holds the levels >= lowest_given_level (node level; ids into xyz, clamped
    positions); the levels above are rebuilt, deepest first, from the children's files in octant order, keyed against the
    root bounds, with AlwaysAdhereToMinSpacing.  Returns files with the rebuilt levels added.  unsorted: a list that receives
    the parents whose children's files are out of order (instead of the assertion; the result is then not to be trusted)."""
    out = {k: list(v) for k, v in files.items() if k[0] >= lowest_given_level}
    for lv in range(lowest_given_level, -1, -1):  # children at node level lv (lv + 1 octants), parents at lv - 1
        child_shift = _shift(lv)
        parents = sorted({(k[1] >> child_shift) >> 3 for k in out if k[0] == lv})
        for index in parents:
            node_key = 0 if lv == 0 else index << (3 * (LEVELS - lv))
            ids = [i for o in range(8) for i in out.get((lv, node_key | (o << child_shift)), [])]
            ids = np.asarray(ids, dtype=np.uint32)
            keys, _ = O.index_points(xyz[ids], bmin, bmax)
            if not np.all(keys[1:] >= keys[:-1]):
                assert unsorted is not None, "children's files out of order inside a parent: choose another input"
                unsorted.append((lv - 1, node_key))
            t = sample_points(max_points, keys, ids, xyz, node_key, lv - 1, bmin, bmax, spacing_at_root, O.ALWAYS_ADHERE).astype(bool)
            out[(lv - 1, node_key)] = list(ids[t])
    return out
