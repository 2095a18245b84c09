"""Node tables shared by the tests of the world-frame converter's kernels (test_srs_node_boxes_gpu.py,
test_pnts_origin_gpu.py): placed by the tile T of the kernel under test."""
import numpy as np


def tables(T):
    """name -> (rows of the buffer, list of (offset, count))"""
    out = {"one_node_%d" % n: (n, [(0, n)]) for n in (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)}
    mixed = [(5, 0), (7, T - 8), (T - 1, 2), (T + 1, 0), (T + 1, 40)]                  # a gap in front; boundaries at T - 1 and T + 1
    mixed += [(T + 60 + i, 1) for i in range(300)]                                     # more nodes than a tile has rows, after a gap
    mixed += [(T + 360, 0), (T + 360, 0), (T + 365, 2 * T), (3 * T + 365, 0)]           # empty nodes between others; a gap behind
    out["mixed"] = (3 * T + 500, mixed)
    out["gaps_only"] = (T + 9, [(3, 0), (T + 9, 0)])                                    # no node holds a point: all rows are mapped
    return out


def nodes(table):
    return dict(offset=np.array([o for o, _ in table], dtype=np.uint64), count=np.array([c for _, c in table], dtype=np.uint64))
