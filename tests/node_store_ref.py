"""What tests/test_node_store_paths.py needs beside the oracle: points on the centres of the 2^21 key grid (every key is
then integer arithmetic), a traced Python restatement of the multi-batch ACCURATE tiler for every sampler the oracle knows
(md_fast_ref.MultiBatch with the oracle's own sample_points), and the quantities that decide which way the library's node
store goes: the brackets of the merge's workgroups and the segments a workgroup of the file gather spans.  TEST
INFRASTRUCTURE ONLY: it never touches the library under test."""
import numpy as np

import md_fast_ref as M
import oracle_lib as O

CELLS = 1 << 21


def _spread(v):
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros(v.shape, dtype=np.uint64)
    for b in range(21):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def keys_of_cells(cells):
    """Morton keys of key-grid cells (n, 3): x in bit 2, y in bit 1, z in bit 0 of every digit"""
    cells = np.asarray(cells, dtype=np.uint64).reshape(-1, 3)
    return (_spread(cells[:, 0]) << np.uint64(2)) | (_spread(cells[:, 1]) << np.uint64(1)) | _spread(cells[:, 2])


def points_of_cells(cells, bounds):
    """the centres of key-grid cells (n, 3) of a box whose extents are powers of two: exact in double"""
    lo, hi = np.asarray(bounds[0], dtype=np.float64), np.asarray(bounds[1], dtype=np.float64)
    return lo + (np.asarray(cells, dtype=np.float64).reshape(-1, 3) + 0.5) * ((hi - lo) / CELLS)


def lattice(per_axis, offset=0, lo=0, hi=CELLS):
    """per_axis^3 cells, evenly spaced over [lo, hi) on every axis, shifted by offset cells"""
    step = (hi - lo) // per_axis
    a = lo + offset + step * np.arange(per_axis, dtype=np.int64)
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
    return g


def random_cells(rng, n, lo=(0, 0, 0), hi=(CELLS, CELLS, CELLS)):
    """n DISTINCT cells inside [lo, hi)"""
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    c = lo + (rng.random((2 * n + 64, 3)) * (hi - lo)).astype(np.int64)
    _, first = np.unique(keys_of_cells(c), return_index=True)
    c = c[np.sort(first)]
    assert len(c) >= n
    return c[:n]


class StoreTrace(M.MultiBatch):
    """MultiBatch with the oracle's sampler, remembering per batch and level what each node merged:
    batches[b][level] = [(node_key, new_keys, cached_keys)] in node order; snapshots[b] = {(level, key): file length} after
    batch b; unsorted_cached_nodes counts the INTERNAL nodes that read a file back out of order, unsorted_terminal the terminal
    ones (their sum is the oracle's counter).  Re-rooting is not restated (case D asks the oracle alone)."""

    def __init__(self, bounds, sampler, max_points, spacing, max_depth=100):
        super().__init__(bounds[0], bounds[1], max_points, spacing, max_depth, count_unsorted=True)
        self.sampler = sampler
        self.batches, self.snapshots = [], []
        self.unsorted_terminal = 0

    def add_batch(self, batch):
        self.cur = {}
        self.batches.append(self.cur)
        super().add_batch(batch)
        self.snapshots.append({k: len(v) for k, v in self.files.items() if len(v)})

    def _node(self, keys, ids, node_key, node_level):
        cached = np.asarray(self.files.get((node_level, node_key), []), dtype=np.uint32)
        ckeys = M._rekey(cached, self.xyz, node_key, node_level, self.bmin, self.bmax) if len(cached) else np.zeros(0, np.uint64)
        self.cur.setdefault(node_level, []).append((int(node_key), np.array(keys, dtype=np.uint64), ckeys))
        self.points_visited += len(keys) + len(cached)
        req = int(O.lib().orc_required_morton_index_depth(self.sampler, node_level, O._vec3(self.bmin), O._vec3(self.bmax),
                                                          O.C.c_float(self.spacing)))
        max_level = min(M.LEVELS - 1, self.max_depth)
        terminal = (node_level >= max_level) if req > node_level else (req >= max_level)
        if len(ckeys) > 1 and not np.all(ckeys[1:] >= ckeys[:-1]):
            # (a terminal node's file is new ++ cached: out of order by design, and appended to again as it is -- the
            # oracle's counter sees those too; only an internal node's merge depends on the order)
            if terminal:
                self.unsorted_terminal += 1
            else:
                self.unsorted_cached_nodes += 1
        if terminal:
            self.files[(node_level, node_key)] = list(ids) + list(cached)
            return
        assert req < M.LEVELS, "a node that needs re-rooting: not restated here"
        keys, ids = M._merge(keys, ids, ckeys, cached)
        behaviour = O.ALWAYS_ADHERE if len(cached) else O.TAKE_ALL_WHEN_BELOW_MAX
        taken, pk, pi = O.sample_points(self.sampler, self.max_points, keys, ids, self.xyz, node_key, node_level, self.bmin,
                                        self.bmax, self.spacing, behaviour)
        assert taken > 0, taken
        self.files[(node_level, node_key)] = list(pi[:taken])
        rk, ri = pk[taken:], pi[taken:]
        for o, b, e in M._children(rk, node_level + 1):
            self._node(rk[b:e], ri[b:e], int(node_key) | (o << M._shift(node_level + 1)), node_level + 1)

    # ---- what the library's level-synchronous loop sees
    def level_runs(self, batch, level):
        """(new run, cached run, [node keys], [cached file lengths]) of a level of a batch: the nodes' runs one behind the other"""
        nodes = self.batches[batch].get(level, [])
        new = np.concatenate([n[1] for n in nodes]) if nodes else np.zeros(0, np.uint64)
        old = np.concatenate([n[2] for n in nodes]) if nodes else np.zeros(0, np.uint64)
        return new, old, [n[0] for n in nodes], [len(n[2]) for n in nodes]

    def files_before(self, batch, level):
        """{node key: file length} of a level before a batch"""
        if batch == 0:
            return {}
        return {k[1]: v for k, v in self.snapshots[batch - 1].items() if k[0] == level}


def node_shift(level):
    return 63 if level < 0 else 3 * (M.LEVELS - 1 - level)


def _widest(a, b, side, tile):
    if len(a) == 0:
        return 0
    i0 = np.arange(0, len(a), tile)
    last = np.minimum(i0 + tile - 1, len(a) - 1)
    return int((np.searchsorted(b, a[last], side) - np.searchsorted(b, a[i0], side)).max())


def merge_brackets(new, cached, shift, tile):
    """The widest bracket over the workgroups of the merge's two passes: (new run ranked in the cached one: elements
    strictly smaller; cached run ranked in the new one: smaller or equal), keys compared after >> shift"""
    a, b = new >> np.uint64(shift), cached >> np.uint64(shift)
    return _widest(a, b, "left", tile), _widest(b, a, "right", tile)


def gather_span(lengths, group=256):
    """The most segments (empty ones included) that `group` consecutive outputs of the file gather span"""
    lengths = np.asarray(lengths, dtype=np.int64)
    total = int(lengths.sum())
    if total == 0:
        return 0
    poff = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    e0 = np.arange(0, total, group)
    last = np.minimum(e0 + group - 1, total - 1)
    seg = lambda e: np.searchsorted(poff, e, "right") - 1
    return int((seg(last) - seg(e0) + 1).max())
