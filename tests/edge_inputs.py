"""Inputs for the edge tests of the Morton encode, the re-key, the device node lists and the payload gather
(test_encode_edges.py, test_rekey_edges.py, test_node_lists_device_edges.py, test_payload_gather_edges.py).
Plain numpy and, for node boxes and keys, the CPU oracle: no GPU, no library.  Every family is seeded; the premises the GPU tests rely on are checked on the CPU by the
tests without a gpu mark in the same modules."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TWO21 = 1 << 21


def _box(mn, ext):
    mn = [float(v) for v in mn]
    ext = [float(ext)] * 3 if np.isscalar(ext) else [float(v) for v in ext]
    return mn, [a + e for a, e in zip(mn, ext)]


UNIT = _box([0.0, 0.0, 0.0], 1.0)
ODD = _box([-512.25, 1000.5, -3.125], 777.7)                                  # the known answer of test_gpu_parity.py
UTM = _box([399812.37, 5651234.91, 211.03], [1234.567, 987.653, 89.31])       # georeferenced magnitudes, ~1 km at 5.6e6
BOXES = {"unit": UNIT, "odd": ODD, "utm": UTM}


def inside(rng, n, box):
    """n points strictly inside the box (the open unit interval scaled: never on a face)"""
    lo, hi = np.array(box[0]), np.array(box[1])
    return lo + (0.001 + 0.998 * rng.random((n, 3))) * (hi - lo)


def step(x, ulps):
    """x moved by `ulps` representable doubles (negative: towards -inf)"""
    x = np.array(x, dtype=np.float64)
    for _ in range(abs(int(ulps))):
        x = np.nextafter(x, np.inf if ulps > 0 else -np.inf)
    return x


# ------------------------------------------------------------------------------------------------------------- encode
FACE_CELLS = [0, 1, 2, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, TWO21 - 2, TWO21 - 1]
FACE_ULPS = (-2, -1, 0, 1, 2)


def cell_face_points(box, axis, seed):
    """Points on and beside cell faces of one axis: x = min + k * extent / 2^21 in double for the cells of FACE_CELLS and 2000
    random cells, moved by the steps of FACE_ULPS; the other two axes random inside.  Returns (xyz, k per point, ulps per point)."""
    rng = np.random.default_rng(seed)
    k = np.concatenate([np.array(FACE_CELLS, dtype=np.int64), rng.integers(0, TWO21, size=2000)])
    mn, ext = box[0][axis], box[1][axis] - box[0][axis]
    face = mn + k.astype(np.float64) * ext / float(TWO21)
    cols, ks, us = [], [], []
    for u in FACE_ULPS:
        cols.append(step(face, u))
        ks.append(k)
        us.append(np.full(k.shape, u))
    x = np.concatenate(cols)
    xyz = inside(rng, x.shape[0], box)
    xyz[:, axis] = x
    return xyz, np.concatenate(ks), np.concatenate(us)


def compact_by_3(v):
    """every third bit of v (bit 0, 3, 6, ...) packed: the inverse of the encode's bit spreading"""
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros(v.shape, dtype=np.uint64)
    for j in range(21):
        out |= ((v >> np.uint64(3 * j)) & np.uint64(1)) << np.uint64(j)
    return out


def key_cell(keys, axis):
    """the cell index of one axis inside a 21-level key: x is bit 3j+2, y 3j+1, z 3j"""
    return compact_by_3(np.asarray(keys, dtype=np.uint64) >> np.uint64(2 - axis)).astype(np.int64)


SPECIAL_POSITIONS = (0, 255, 256, 511, -1)
SPECIAL_SIZES = (1, 85, 86, 255, 256, 257, 513, 100003)


def special_points(box, seed):
    """One row per special: the value on one axis, the others inside -- the faces, one step outside them, infinities, NaN,
    +-1e308, -0.0 and the smallest denormal (inside when min = 0.0), and a point ON the upper face of one axis whose next
    axis is -0.0 (inside in a box with min = 0.0: nothing may be written back, the sign stays)."""
    rng = np.random.default_rng(seed)
    rows, names = [], []
    for axis in range(3):
        mn, mx = box[0][axis], box[1][axis]
        values = {"min": mn, "max": mx, "above max": np.nextafter(mx, np.inf), "below min": np.nextafter(mn, -np.inf),
                  "+inf": np.inf, "-inf": -np.inf, "nan": np.nan, "+1e308": 1e308, "-1e308": -1e308, "-0.0": -0.0,
                  "denormal": 5e-324}
        for name, v in values.items():
            p = inside(rng, 1, box)[0]
            p[axis] = v
            rows.append(p)
            names.append("%s on axis %d" % (name, axis))
        p = inside(rng, 1, box)[0]
        p[axis] = mx
        p[(axis + 1) % 3] = -0.0
        rows.append(p)
        names.append("max on axis %d, -0.0 on the next" % axis)
    return np.array(rows), names


def special_clouds(box, n, seed):
    """Clouds of n inside points with the specials at SPECIAL_POSITIONS, five specials per cloud."""
    sp, _ = special_points(box, seed)
    pos = sorted({p % n for p in SPECIAL_POSITIONS if -n <= p < n})
    rng = np.random.default_rng(seed + n)
    clouds = []
    for first in range(0, len(sp), len(pos)):
        xyz = inside(rng, n, box)
        for j, s in zip(pos, sp[first:first + len(pos)]):
            xyz[j] = s
        clouds.append(xyz)
    return clouds


# name -> (bounds, what the encode entry does with them)
EXTREME_BOUNDS = {
    "extent 5e-324": (_box([0.0] * 3, 5e-324), "refused"),     # 2^21 / extent = inf: (min - min) * inf = NaN
    "extent 1e-310": (_box([0.0] * 3, 1e-310), "refused"),     # the same
    "extent 1e-300": (_box([0.0] * 3, 1e-300), "accepted"),    # scale 2.1e306: finite, every product below 2^21 + 1
    "extent 1e300": (_box([0.0] * 3, 1e300), "accepted"),      # scale 2.1e-294: finite and normal
    "-1e308 .. 1e308": (([-1e308] * 3, [1e308] * 3), "refused"),     # the extent overflows to inf: scale 0, inf * 0 = NaN
    "max = +inf": (([0.0] * 3, [np.inf] * 3), "refused"),
}


def extreme_points(box, seed):
    """min, max, the centre, a point outside on every axis, NaN, and random points inside -- for bounds with finite faces;
    an infinite face stands for itself."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(box[0]), np.array(box[1])
    with np.errstate(all="ignore"):
        mid = lo / 2 + hi / 2
        rnd = lo + rng.random((59, 3)) * (hi - lo)
        rnd = np.where(np.isfinite(rnd), rnd, mid)
    fixed = np.array([lo, hi, mid, [lo[0], hi[1], mid[2]], [hi[0], lo[1], lo[2]], [-1.0, 5.0, np.nan], [np.inf, -np.inf, 0.0]])
    return np.vstack([fixed, rnd])


# ------------------------------------------------------------------------------------------------------------- re-key
REKEY_DEPTHS = (1, 2, 5, 12)
REKEY_PATHS = 3
REKEY_FACE_POINTS = 6      # per node, axis, plane and step
REKEY_NODE_FILLER = 1500
REKEY_ROOT_FILLER = 30000


def rekey_nodes(seed):
    """(key, depth) of the nodes whose faces the family visits: depths 1, 2, 5 and 12 along a few seeded key paths"""
    rng = np.random.default_rng(seed)
    paths = rng.integers(0, 1 << 63, size=REKEY_PATHS, dtype=np.uint64)
    return [(int(k) >> (63 - 3 * d) << (63 - 3 * d), d) for k in paths for d in REKEY_DEPTHS]


def rekey_family(box, seed, node_filler=REKEY_NODE_FILLER):
    """Points on the six faces and the three mid-planes of every node of rekey_nodes(seed) and one step either side, random
    filler inside each of those nodes and all over the root, shuffled (so that every batch reaches every node).
    Returns (xyz, is_face_point, nodes); the node boxes are the oracle's get_bounds_from_morton_index."""
    import oracle_lib as O
    rng = np.random.default_rng(seed + 1)
    nodes = rekey_nodes(seed)
    parts = [inside(rng, REKEY_ROOT_FILLER, box)]
    face = [np.zeros(REKEY_ROOT_FILLER, dtype=bool)]
    for key, depth in nodes:
        nb = O.bounds_from_morton_index(key, box[0], box[1], depth)
        parts.append(inside(rng, node_filler, nb))
        face.append(np.zeros(node_filler, dtype=bool))
        for axis in range(3):
            mn, mx = nb[0][axis], nb[1][axis]
            planes = (mn, mn + (mx - mn) / 2, mx)      # the mid-plane the way box_descend halves: min + extent / 2
            for plane in planes:
                for u in (-1, 0, 1):
                    p = inside(rng, REKEY_FACE_POINTS, nb)
                    p[:, axis] = step(plane, u)
                    parts.append(p)
                    face.append(np.ones(REKEY_FACE_POINTS, dtype=bool))
    xyz, face = np.vstack(parts), np.concatenate(face)
    order = rng.permutation(xyz.shape[0])
    return xyz[order], face[order], nodes


def rekeyed(key, p, box, depth):
    """read_pnts_from_disk's key of the point p (root key `key`) in a file of its ancestor with `depth` octants: the node's
    digits, then the first 21 - depth digits of the index of p inside the node's box (no clamp), all by the oracle"""
    import oracle_lib as O
    if depth == 0:
        return O.morton_index(p, box[0], box[1])
    sh = 63 - 3 * depth
    nb = O.bounds_from_morton_index(int(key), box[0], box[1], depth)
    return (int(key) >> sh << sh) | (O.morton_index(p, nb[0], nb[1]) >> (3 * depth))


def rekey_consistent(xyz, box):
    """Per point: every ancestor box gives it the key the root box gives it.  Files of such points come back ascending (no
    inversion, the premise of an exact comparison); a point a step beside a face for which this fails is where the
    halving chain and the root scale round differently -- the documented divergence."""
    import oracle_lib as O
    keys, clamped = O.index_points(xyz, *box)
    return np.array([all(rekeyed(k, p, box, d) == int(k) for d in range(1, 21)) for k, p in zip(keys, clamped)], dtype=bool)


# ------------------------------------------------------------------------------------------------------------- node lists
def level_shift(level):
    return 63 if level < 0 else 3 * (20 - int(level))


def node_lists_reference(keys, level):
    """A stable group by level, then by key >> shift: (order, dict of level / key / offset / count)"""
    keys = np.asarray(keys, dtype=np.uint64)
    level = np.asarray(level, dtype=np.int8)
    order = np.argsort(level, kind="stable").astype(np.uint32)
    lv = level[order].astype(np.int64)
    sh = np.where(lv < 0, 63, 3 * (20 - lv)).astype(np.uint64)
    prefix = keys[order] >> sh
    head = np.ones(len(order), dtype=bool)
    head[1:] = (lv[1:] != lv[:-1]) | (prefix[1:] != prefix[:-1])
    off = np.flatnonzero(head).astype(np.uint64)
    cnt = np.diff(np.append(off, np.uint64(len(order)))).astype(np.uint64)
    nkey = np.where(lv[head] < 0, np.uint64(0), prefix[head] << sh[head]).astype(np.uint64)
    return order, dict(level=lv[head].astype(np.int8), key=nkey, offset=off, count=cnt)


def source_constants(path, names):
    """`constexpr int NAME = <integer or product of earlier names>;` of a source file of the library"""
    text = open(os.path.join(ROOT, path)).read()
    env = {}
    for m in re.finditer(r"constexpr\s+(?:int|uint32_t)\s+(\w+)\s*=\s*([\w\s*]+);", text):
        try:
            env[m.group(1)] = int(eval(m.group(2), {"__builtins__": {}}, dict(env)))
        except Exception:
            pass
    return {n: env[n] for n in names}


def node_list_cases():
    """name -> (sorted keys < 2^63, levels in [-1, 20])"""
    rng = np.random.default_rng(20)
    sort_c = source_constants("schwarzwald_amd/csrc/swz_sort.hip", ["SC_TILE", "RS_TILE"])
    m = re.search(r"static int scan_rec\(.*?if \(n <= (\d+)\)", open(os.path.join(ROOT, "schwarzwald_amd/csrc/swz_sort.hip")).read(), re.S)
    tiles = sorted({sort_c["SC_TILE"], sort_c["RS_TILE"], int(m.group(1))})   # scan tile, partition tile, single-block scan limit

    def sorted_keys(n):
        return np.sort(rng.integers(0, 1 << 63, size=n, dtype=np.uint64))

    cases = {}
    cases["one point"] = (np.array([0x123456789ABCDEF], dtype=np.uint64), np.array([7], dtype=np.int8))
    cases["all level -1"] = (sorted_keys(1000), np.full(1000, -1, dtype=np.int8))
    k = sorted_keys(1000)
    k[100:110] = k[100]                                   # equal keys: one node at level 20
    cases["all level 20"] = (k, np.full(1000, 20, dtype=np.int8))
    cases["equal keys at different levels"] = (np.full(9, 0x7123456789ABCDEF & ((1 << 63) - 1), dtype=np.uint64),
                                               np.array([3, 1, 3, -1, 20, 1, 0, 20, 3], dtype=np.int8))
    # level 5 (shift 45): neighbours that differ below the shift only (one node), in the lowest digit of the prefix (two)
    base = 0x2AAAAAAAAAAAAAAA >> 45 << 45
    k = np.array([base, base + 1, base + (1 << 45) - 1, base + (1 << 45), base + (1 << 45) + 5, base + (7 << 45)], dtype=np.uint64)
    cases["neighbours at the node's shift"] = (k, np.full(6, 5, dtype=np.int8))
    k = sorted_keys(3000)
    lv = rng.integers(-1, 21, size=3000).astype(np.int8)
    lv[:2] = (20, -1)
    cases["levels -1 and 20 together"] = (k, lv)
    cases["every level, two tiles of the partition"] = (sorted_keys(2 * sort_c["RS_TILE"] + 17),
                                                        (np.arange(2 * sort_c["RS_TILE"] + 17) % 22 - 1).astype(np.int8))
    k = np.unique(sorted_keys(5000))
    cases["every point its own node"] = (k, np.full(len(k), 20, dtype=np.int8))
    # heads exactly at multiples of 256 and at the tile sizes, n one below, at and one above a tile size
    for t in tiles:
        for n in (t - 1, t, t + 1, 3 * t + 1):
            heads = sorted({0} | {h for h in list(range(256, n, 256)) + [x * j for x in tiles for j in (1, 2, 3)] if h < n} | {n - 1})
            node = np.zeros(n, dtype=np.uint64)
            node[heads] = 1
            node = np.cumsum(node) - 1                                   # node index of every point
            low = rng.integers(0, 1 << 45, size=n, dtype=np.uint64)
            k = (node.astype(np.uint64) << np.uint64(45)) | low
            k = np.sort(k)                                               # (sorted inside a node; the prefix already ascends)
            cases["heads at seams, n = %d" % n] = (k, np.full(n, 5, dtype=np.int8))
    return cases


# ------------------------------------------------------------------------------------------------------------- payload gather
GATHER_SIZES = (1, 255, 256, 257, 65537)
GUARD_ROWS = 64
SENTINEL = 0xA5


def gather_indices(kind, n, rng):
    """n indices below n"""
    if kind == "identity":
        return np.arange(n, dtype=np.uint32)
    if kind == "reversed":
        return np.arange(n, dtype=np.uint32)[::-1].copy()
    if kind == "permutation":
        return rng.permutation(n).astype(np.uint32)
    assert kind == "repeats"
    return rng.integers(0, max(n // 3, 1), size=n).astype(np.uint32)


def gather_source(dtype, width, n, rng):
    """n rows of raw bytes with NaNs that carry payload bits, -0.0, denormals and 0xFF bytes among them"""
    dt = np.dtype(dtype)
    raw = rng.integers(0, 256, size=n * width * dt.itemsize, dtype=np.uint8)
    a = raw.view(dt).reshape(n, width).copy()
    flat = a.reshape(-1)
    special = {np.dtype(np.float64): np.array([0x7FF8000000000001, 0xFFF0DEADBEEF0001, 0x8000000000000000, 0x0000000000000001,
                                               0x800FFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64),
               np.dtype(np.float32): np.array([0x7FC00001, 0xFF80BEEF, 0x80000000, 0x00000001, 0x807FFFFF, 0xFFFFFFFF],
                                              dtype=np.uint32).view(np.float32)}.get(dt)
    if special is None:
        special = np.array([np.iinfo(dt).max, np.iinfo(dt).min, 0], dtype=dt) if dt.kind in "iu" else None
    at = rng.integers(0, flat.shape[0], size=min(flat.shape[0], 4 * len(special)))
    flat.view(np.uint8).reshape(-1, dt.itemsize)[at] = np.resize(special, at.shape[0]).view(np.uint8).reshape(-1, dt.itemsize)
    flat.view(np.uint8)[rng.integers(0, flat.nbytes, size=min(flat.nbytes, 8))] = 0xFF
    return a
