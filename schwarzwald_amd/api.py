"""ctypes binding of libswz_gpu.so (include/swz_gpu.h).

Host-buffer methods take numpy arrays; *_device methods take raw device pointers (ints, e.g.
torch.Tensor.data_ptr()).  Every failure raises SwzError with the library's message; a missing
library raises at load time -- nothing here computes on the CPU.
"""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

RANDOM_GRID, GRID_CENTER, MIN_DISTANCE, JITTERED = 0, 1, 2, 3
SAMPLERS = {"RANDOM_GRID": RANDOM_GRID, "GRID_CENTER": GRID_CENTER, "MIN_DISTANCE": MIN_DISTANCE,
            "JITTERED": JITTERED}
# MIN_DISTANCE_FAST (AdaptivePoissonDiskSampling): every n-th point of a node through MIN_DISTANCE's greedy test,
# n = min_distance_fast_stride(node level).  ALL_SAMPLERS holds the five --sampling names; SAMPLERS stays the four that every
# entry point, sharded or not, takes.
MIN_DISTANCE_FAST = 4
ALL_SAMPLERS = dict(SAMPLERS, MIN_DISTANCE_FAST=MIN_DISTANCE_FAST)
TAKE_ALL_WHEN_COUNT_BELOW_MAX_POINTS, ALWAYS_ADHERE_TO_MIN_SPACING = 0, 1
ACCURATE, FAST = 0, 1
ERR_BAD_ARG = 2
ERR_INTERNAL = 7
ERR_TILER_FAILED = 8
ERR_PEER_FAILED = 100  # raised by the multi-GPU driver on the ranks that did not fail themselves

_HERE = os.path.dirname(os.path.abspath(__file__))


class SwzError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("swz error %d: %s" % (code, message))
        self.code = code


class _TileParams(C.Structure):
    _fields_ = [("sampler", C.c_int32), ("max_points_per_node", C.c_uint64), ("spacing_at_root", C.c_float),
                ("max_depth", C.c_uint32), ("strategy", C.c_int32), ("fast_concurrency", C.c_uint32),
                ("flags", C.c_uint32)]


ABI_VERSION = 3  # SWZ_ABI_VERSION of include/swz_gpu.h
FLAG_MIN_DISTANCE_PROPERTY = 1


class _TileStats(C.Structure):
    _fields_ = [("num_nodes", C.c_uint64), ("points_visited", C.c_uint64), ("max_level", C.c_int32),
                ("fast_start_levels", C.c_int32), ("num_levels", C.c_uint32), ("min_distance_rounds", C.c_uint32)]


class _ShardInfo(C.Structure):
    _fields_ = [("global_points", C.c_uint64), ("d_ghost_xyz", C.c_void_p), ("num_ghosts", C.c_uint64)]


class _TilerInfo(C.Structure):
    _fields_ = [("num_points", C.c_uint64), ("num_stored", C.c_uint64), ("num_nodes", C.c_uint64),
                ("num_batches", C.c_uint64), ("rekey_inversions", C.c_uint64), ("fast_start_levels", C.c_int32),
                ("staged_bytes", C.c_uint64), ("staged_wait_ms", C.c_double)]


class _TilerShardInfo(C.Structure):
    _fields_ = [("global_new_points", C.c_uint64), ("global_root_stored", C.c_uint64), ("d_ghost_xyz", C.c_void_p),
                ("num_ghosts", C.c_uint64)]


class _KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double),
                ("algorithmic_bytes", C.c_uint64)]


@dataclass
class TileParams:
    sampler: int = MIN_DISTANCE
    max_points_per_node: int = 20000      # --max-points-per-node default, executable/main.cpp:230-232
    spacing_at_root: float = 0.0
    max_depth: int = 100                  # TilerProcess.cpp:624-629
    strategy: int = ACCURATE
    fast_concurrency: int = 8
    flags: int = 0                        # FLAG_MIN_DISTANCE_PROPERTY: see include/swz_gpu.h

    def _c(self):
        return _TileParams(self.sampler, self.max_points_per_node, self.spacing_at_root, self.max_depth,
                           self.strategy, self.fast_concurrency, self.flags)


@dataclass
class TileResult:
    keys: np.ndarray      # sorted Morton keys
    perm: np.ndarray      # original index of each sorted position
    level: np.ndarray     # node level that persists the point (-1 = root)
    dup: np.ndarray       # FAST duplicate mask (zeros for ACCURATE)
    stats: dict
    xyz_clamped: np.ndarray


def spacing_from_diagonal(bmin, bmax, diagonal_fraction):
    """TilerProcess.cpp:598-604: (float)(bounds.extent().length() / diagonal_fraction)."""
    e = np.asarray(bmax, dtype=np.float64) - np.asarray(bmin, dtype=np.float64)
    return float(np.float32(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) / diagonal_fraction))


# attribute columns of a point batch: name -> (index = bit of BinaryPersistence's bitmask, numpy dtype, row width)
ATTRIBUTES = {
    "rgb": (0, np.uint8, 3), "normal": (1, np.float32, 3), "intensity": (2, np.uint16, 1),
    "classification": (3, np.uint8, 1), "edge_of_flight_line": (4, np.uint8, 1), "gps_time": (5, np.float64, 1),
    "number_of_returns": (6, np.uint8, 1), "return_number": (7, np.uint8, 1), "point_source_id": (8, np.uint16, 1),
    "scan_direction_flag": (9, np.uint8, 1), "scan_angle_rank": (10, np.int8, 1), "user_data": (11, np.uint8, 1),
}


class _LasLayout(C.Structure):
    _fields_ = [("scale", C.c_double * 3), ("offset", C.c_double * 3), ("min", C.c_double * 3), ("max", C.c_double * 3),
                ("point_format", C.c_uint32), ("record_bytes", C.c_uint32)]


class _AttributeColumns(C.Structure):
    _fields_ = [("column", C.c_void_p * 12)]


def _host_columns(attrs, n=None):
    """dict name -> array  =>  (swz_attribute_columns, keep-alive list of contiguous arrays)"""
    cols, keep = _AttributeColumns(), {}
    for name, arr in (attrs or {}).items():
        idx, dt, width = ATTRIBUTES[name]
        a = np.ascontiguousarray(arr, dtype=dt).reshape(-1, width) if width > 1 else np.ascontiguousarray(arr, dtype=dt).reshape(-1)
        if n is not None and a.shape[0] != n:
            raise ValueError("attribute %s has %d rows, expected %d" % (name, a.shape[0], n))
        keep[name] = a
        cols.column[idx] = a.ctypes.data
    return cols, keep


def device_columns(ptrs):
    """dict name -> device pointer  =>  swz_attribute_columns"""
    cols = _AttributeColumns()
    for name, ptr in (ptrs or {}).items():
        cols.column[ATTRIBUTES[name][0]] = int(ptr)
    return cols


_NODE_DTYPES = dict(level=np.int8, key=np.uint64, offset=np.uint64, count=np.uint64)


def _node_columns(nodes, *names):
    """The named columns of a node table (dict of level / key / offset / count) as the contiguous arrays the library reads."""
    return [np.ascontiguousarray(nodes[k], dtype=_NODE_DTYPES[k]) for k in names]


def node_name(level, key):
    """"r" + octant digits of a node (TilingAlgorithms.cpp:139)."""
    buf = C.create_string_buffer(24)
    if load_library().swz_node_name(int(level), int(key), buf) != 0:
        raise ValueError("bad node level %d" % level)
    return buf.value.decode()


def node_name_entwine(level, key):
    """Entwine's "D-X-Y-Z" name of a node (OctreeNodeIndex.h:556-573)."""
    buf = C.create_string_buffer(72)
    if load_library().swz_node_name_entwine(int(level), int(key), buf) != 0:
        raise ValueError("bad node level %d" % level)
    return buf.value.decode()


def node_from_entwine_name(name):
    """(level, key) of an Entwine node name; ValueError for a malformed name or more than 21 levels."""
    lv, key = C.c_int8(), C.c_uint64()
    if load_library().swz_node_from_entwine_name(name.encode(), C.byref(lv), C.byref(key)) != 0:
        raise ValueError("not an Entwine node name: %r" % name)
    return int(lv.value), int(key.value)


def node_bounds(level, key, root_min, root_max):
    """Box of a node, descending octant by octant from the root box like get_octant_bounds."""
    mn, mx = (C.c_double * 3)(), (C.c_double * 3)()
    if load_library().swz_node_bounds(int(level), int(key), _vec3(root_min), _vec3(root_max), mn, mx) != 0:
        raise ValueError("bad node level %d" % level)
    return list(mn), list(mx)


def node_geometric_error(level, spacing_at_root):
    """Cesium tileset geometricError of a node: spacing_at_root / 2^depth."""
    return float(load_library().swz_node_geometric_error(int(level), C.c_float(spacing_at_root)))


def required_morton_index_depth(sampler, node_level, root_min, root_max, spacing_at_root):
    """required_morton_index_depth of the reference (Sampling.cpp:29-62) as the library evaluates it."""
    L = load_library()
    L.swz_required_morton_index_depth.restype = C.c_int32
    L.swz_required_morton_index_depth.argtypes = [C.c_int, C.c_int32, _dp, _dp, C.c_float]
    return int(L.swz_required_morton_index_depth(int(sampler), int(node_level), _vec3(root_min), _vec3(root_max),
                                                 C.c_float(spacing_at_root)))


def min_distance_fast_stride(node_level):
    """The n of MIN_DISTANCE_FAST at a node level (-1 = the root): 4, 2, then 1 (swz_min_distance_fast_stride)."""
    L = load_library()
    L.swz_min_distance_fast_stride.restype = C.c_int32
    L.swz_min_distance_fast_stride.argtypes = [C.c_int32]
    return int(L.swz_min_distance_fast_stride(int(node_level)))


class _TilesetNode(C.Structure):
    _fields_ = [("level", C.c_int8), ("has_content", C.c_uint8), ("is_tileset_root", C.c_uint8), ("tight", C.c_uint8),
                ("num_children", C.c_uint32), ("key", C.c_uint64), ("parent", C.c_int64), ("first_child", C.c_int64),
                ("geometric_error", C.c_double), ("bounds_min", C.c_double * 3), ("bounds_max", C.c_double * 3)]


def tileset_build(node_level, node_key, root_min, root_max, spacing_at_root, global_offset=None, node_boxes=None):
    """Tileset tree of a node table (Cesium3DTilesPersistence.cpp:80-156): list of dicts ordered by (level, key).
    node_boxes: (box_min, box_max), num_nodes x 3 each in table order (Tiler.node_boxes) -- swz_tileset_build_boxes: the
    bounds become the boxes of the points, united bottom-up, and the dicts carry `tight` (tileset_write then writes
    half-axes)."""
    L = load_library()
    lv = np.ascontiguousarray(node_level, dtype=np.int8)
    key = np.ascontiguousarray(node_key, dtype=np.uint64)
    off = _vec3(global_offset) if global_offset is not None else None
    num = C.c_uint64()
    head = (lv.shape[0], lv.ctypes.data_as(_i8p), key.ctypes.data_as(_u64p))
    tail = (_vec3(root_min), _vec3(root_max), C.c_float(spacing_at_root), off)
    if node_boxes is None:
        build, args = L.swz_tileset_build, head + tail
    else:
        lo = np.ascontiguousarray(node_boxes[0], dtype=np.float64).reshape(-1)
        hi = np.ascontiguousarray(node_boxes[1], dtype=np.float64).reshape(-1)
        if lo.shape[0] != 3 * lv.shape[0] or hi.shape[0] != 3 * lv.shape[0]:
            raise ValueError("node_boxes must hold 3 values per node")
        build, args = L.swz_tileset_build_boxes, head + (lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp)) + tail
    if build(*args, 0, None, C.byref(num)) != 0:
        raise ValueError("bad node table")
    buf = (_TilesetNode * max(int(num.value), 1))()
    if build(*args, int(num.value), buf, C.byref(num)) != 0:
        raise ValueError("bad node table")
    tiles = [dict(level=int(t.level), key=int(t.key), has_content=bool(t.has_content), is_tileset_root=bool(t.is_tileset_root),
                  num_children=int(t.num_children), parent=int(t.parent), first_child=int(t.first_child),
                  geometric_error=float(t.geometric_error), bounds_min=list(t.bounds_min), bounds_max=list(t.bounds_max))
             for t in buf[:int(num.value)]]
    if node_boxes is not None:
        for d, t in zip(tiles, buf):
            d["tight"] = bool(t.tight)
    return tiles


def bin_write_node(path, xyz, attrs=None, compressed=False):
    """BinaryPersistence::persist_points for one node (host only, no GPU needed)."""
    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    cols, keep = _host_columns(attrs, x.shape[0])
    st = load_library().swz_bin_write_node(None, os.fsencode(path), x.shape[0], x.ctypes.data_as(_dp), C.byref(cols),
                                           int(bool(compressed)))
    if st != 0:
        raise SwzError(st, "swz_bin_write_node(%s) failed" % path)


def bin_read_node(path, compressed=False):
    """BinaryPersistence::retrieve_points: returns (xyz, dict of attribute arrays)."""
    L = load_library()
    mask, count = C.c_uint32(), C.c_uint64()
    st = L.swz_bin_read_header(None, os.fsencode(path), int(bool(compressed)), C.byref(mask), C.byref(count))
    if st != 0:
        raise SwzError(st, "swz_bin_read_header(%s) failed" % path)
    n = int(count.value)
    xyz = np.empty((n, 3), dtype=np.float64)
    out = {}
    for name, (idx, dt, width) in ATTRIBUTES.items():
        if mask.value & (1 << idx):
            out[name] = np.empty((n, width) if width > 1 else n, dtype=dt)
    cols, keep = _host_columns(out, n)
    st = L.swz_bin_read_node(None, os.fsencode(path), int(bool(compressed)), xyz.ctypes.data_as(_dp), C.byref(cols))
    if st != 0:
        raise SwzError(st, "swz_bin_read_node(%s) failed" % path)
    return xyz, keep


# 3D Tiles node files (include/swz_gpu.h, swz_pnts_*): the arrays a .pnts file may hold besides POSITION, and how RGB is made
PNTS_RGB, PNTS_INTENSITY = 1 << 0, 1 << 2
RGB_FROM_COLOR, RGB_FROM_INTENSITY_LINEAR, RGB_FROM_INTENSITY_LOG = 0, 1, 2


def _pnts_mask(attrs):
    """("rgb", "intensity") or a mask  =>  mask"""
    if isinstance(attrs, (int, np.integer)):
        return int(attrs)
    mask = 0
    for name in attrs or ():
        if name not in ("rgb", "intensity"):
            raise ValueError("a .pnts file holds rgb and intensity besides the positions, not %r" % (name,))
        mask |= PNTS_RGB if name == "rgb" else PNTS_INTENSITY
    return mask


def pnts_layout(counts, attrs=(), rgb_from=RGB_FROM_COLOR):
    """swz_pnts_layout: where every node's .pnts body lies in one contiguous image.  Returns a dict of per-node arrays
    offset / size / rgb_offset / intensity_offset and the image's total size."""
    cnt = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    m = cnt.shape[0]
    out = {k: np.empty(m, dtype=np.uint64) for k in ("offset", "size", "rgb_offset", "intensity_offset")}
    total = C.c_uint64()
    st = load_library().swz_pnts_layout(m, cnt.ctypes.data_as(_u64p), _pnts_mask(attrs), int(rgb_from),
                                        out["offset"].ctypes.data_as(_u64p), out["size"].ctypes.data_as(_u64p),
                                        out["rgb_offset"].ctypes.data_as(_u64p), out["intensity_offset"].ctypes.data_as(_u64p),
                                        C.byref(total))
    if st != 0:
        raise SwzError(st, "swz_pnts_layout failed")
    out["total"] = int(total.value)
    return out


def pnts_rgb_from_intensity(rgb_from, intensity):
    """One value of the grey table of --calculate-rgb-from (PNTSWriter.cpp:507-527)."""
    return int(load_library().swz_pnts_rgb_from_intensity(int(rgb_from), int(intensity)))


def pnts_write_node(path, count, body, attrs=(), rtc_center=None):
    """One .pnts file from a packed body (a slice of the image pnts_pack_device wrote; host only)."""
    b = np.ascontiguousarray(body, dtype=np.uint8).reshape(-1)
    rtc = _vec3(rtc_center) if rtc_center is not None else None
    st = load_library().swz_pnts_write_node(None, os.fsencode(path), int(count), b.ctypes.data, b.shape[0], _pnts_mask(attrs), rtc)
    if st != 0:
        raise SwzError(st, "swz_pnts_write_node(%s) failed" % path)


def pnts_write_node_rows(path, xyz, attrs=None, write=None, rgb_from=RGB_FROM_COLOR, rtc_center=None):
    """The same file from unpacked rows: double positions plus the columns of attrs (dict name -> array), converted on the
    host.  write: the arrays to put into the file (default: what attrs holds of rgb / intensity)."""
    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    cols, keep = _host_columns(attrs, x.shape[0])
    if write is None:
        write = [k for k in ("rgb", "intensity") if k in (attrs or {})]
    rtc = _vec3(rtc_center) if rtc_center is not None else None
    st = load_library().swz_pnts_write_node_rows(None, os.fsencode(path), x.shape[0], x.ctypes.data_as(_dp), C.byref(cols),
                                                 _pnts_mask(write), int(rgb_from), rtc)
    if st != 0:
        raise SwzError(st, "swz_pnts_write_node_rows(%s) failed" % path)


def pnts_read_node(path):
    """retrieve_points of a .pnts file: (xyz as float64 of the stored floats, dict of rgb / intensity if present, RTC_CENTER)."""
    L = load_library()
    mask, count, rtc = C.c_uint32(), C.c_uint64(), (C.c_double * 3)()
    st = L.swz_pnts_read_header(None, os.fsencode(path), C.byref(count), C.byref(mask), rtc)
    if st != 0:
        raise SwzError(st, "swz_pnts_read_header(%s) failed" % path)
    n = int(count.value)
    xyz = np.empty((n, 3), dtype=np.float64)
    out = {}
    if mask.value & PNTS_RGB:
        out["rgb"] = np.empty((n, 3), dtype=np.uint8)
    if mask.value & PNTS_INTENSITY:
        out["intensity"] = np.empty(n, dtype=np.uint16)
    cols, keep = _host_columns(out, n)
    st = L.swz_pnts_read_node(None, os.fsencode(path), xyz.ctypes.data_as(_dp), C.byref(cols))
    if st != 0:
        raise SwzError(st, "swz_pnts_read_node(%s) failed" % path)
    return xyz, keep, list(rtc)


def pnts_parse_image(image):
    """swz_pnts_parse_image: where the arrays of a .pnts file image (bytes, or a uint8 array) are -- a dict of count, mask,
    attrs, rtc_center and position_offset / rgb_offset / intensity_offset, counted from the first byte of the image (0 for
    an array the file lacks).  Host only; a refusal raises SwzError."""
    b = np.frombuffer(bytes(image), dtype=np.uint8) if isinstance(image, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(image, dtype=np.uint8).reshape(-1)
    count, mask, rtc = C.c_uint64(), C.c_uint32(), (C.c_double * 3)()
    pos, rgb, inten = C.c_uint64(), C.c_uint64(), C.c_uint64()
    keep = b if b.shape[0] else np.zeros(1, dtype=np.uint8)
    st = load_library().swz_pnts_parse_image(None, C.c_void_p(keep.ctypes.data), int(b.shape[0]), C.byref(count), C.byref(mask), rtc,
                                             C.byref(pos), C.byref(rgb), C.byref(inten))
    if st != 0:
        raise SwzError(st, "swz_pnts_parse_image failed")
    m = int(mask.value)
    return dict(count=int(count.value), mask=m, attrs=[k for k, bit in (("rgb", PNTS_RGB), ("intensity", PNTS_INTENSITY)) if m & bit],
                rtc_center=list(rtc), position_offset=int(pos.value), rgb_offset=int(rgb.value), intensity_offset=int(inten.value))


def _tileset_buffer(tiles):
    buf = (_TilesetNode * max(len(tiles), 1))()
    for t, d in zip(buf, tiles):
        t.level, t.key, t.has_content, t.is_tileset_root = d["level"], d["key"], int(d["has_content"]), int(d["is_tileset_root"])
        t.num_children, t.parent, t.first_child, t.geometric_error = d["num_children"], d["parent"], d["first_child"], d["geometric_error"]
        t.bounds_min, t.bounds_max = _vec3(d["bounds_min"]), _vec3(d["bounds_max"])
        t.tight = int(bool(d.get("tight", False)))
    return buf


def tileset_write(tiles, directory):
    """swz_tileset_write: the tileset JSON files of tileset_build's output (the list of dicts it returns)."""
    st = load_library().swz_tileset_write(None, _tileset_buffer(tiles), len(tiles), os.fsencode(directory))
    if st != 0:
        raise SwzError(st, "swz_tileset_write(%s) failed" % directory)


def tileset_oriented_boxes(srs, tiles):
    """swz_tileset_oriented_boxes: (len(tiles), 12) float64 -- per entry of tileset_build's output the centre of its bounds
    and the three vectors to the centres of its upper x, y and z faces, all four points mapped to ECEF through srs (a
    definition string or an Srs; boundingBoxFromAABB, Tileset.cpp:52-92).  srs None maps nothing: centre and half extents."""
    srs = _as_srs(srs)
    obb = np.empty((len(tiles), 12), dtype=np.float64)
    st = load_library().swz_tileset_oriented_boxes(srs._ref() if srs is not None else None, _tileset_buffer(tiles), len(tiles),
                                                   obb.ctypes.data_as(_dp))
    if st != 0:
        raise SwzError(st, "swz_tileset_oriented_boxes failed")
    return obb


def tileset_write_oriented(tiles, obb, directory):
    """swz_tileset_write_oriented: tileset_write with boundingVolume.box of every entry taken from obb (len(tiles) x 12); an
    entry marked `tight` keeps its own axis-aligned half-axes."""
    o = np.ascontiguousarray(obb, dtype=np.float64).reshape(-1)
    if o.shape[0] != 12 * len(tiles):
        raise ValueError("obb must hold 12 values per entry")
    st = load_library().swz_tileset_write_oriented(None, _tileset_buffer(tiles), len(tiles), o.ctypes.data_as(_dp), os.fsencode(directory))
    if st != 0:
        raise SwzError(st, "swz_tileset_write_oriented(%s) failed" % directory)


# LAS node files and Entwine metadata (include/swz_gpu.h, swz_las_* / swz_ept_*)
LAS_NAMING_POTREE, LAS_NAMING_ENTWINE = 0, 1


class _EptJson(C.Structure):
    _fields_ = [("bounds_min", C.c_double * 3), ("bounds_max", C.c_double * 3), ("conforming_min", C.c_double * 3),
                ("conforming_max", C.c_double * 3), ("points", C.c_uint64), ("attribute_mask", C.c_uint32),
                ("reserved", C.c_uint32), ("span", C.c_double), ("srs_authority", C.c_char_p), ("srs_horizontal", C.c_char_p),
                ("srs_wkt", C.c_char_p), ("version", C.c_char_p)]


def _las_mask(attrs):
    """names of ATTRIBUTES or a mask  =>  mask over the attribute indices"""
    if isinstance(attrs, (int, np.integer)):
        return int(attrs)
    mask = 0
    for name in attrs or ():
        mask |= 1 << ATTRIBUTES[name][0]
    return mask


def las_scale_from_bounds(bmin, bmax):
    """compute_las_scale_from_bounds (LASPersistence.cpp:16-28): the scale of a node file from the node box."""
    return float(load_library().swz_las_scale_from_bounds(_vec3(bmin), _vec3(bmax)))


def las_stored_box(box_min, box_max, las_offset, scale):
    """swz_las_stored_box: the box of the stored records of a node whose points have the box [box_min, box_max]."""
    lo, hi = (C.c_double * 3)(), (C.c_double * 3)()
    if load_library().swz_las_stored_box(_vec3(box_min), _vec3(box_max), _vec3(las_offset), float(scale), lo, hi) != 0:
        raise ValueError("bad scale")
    return list(lo), list(hi)


def las_record_layout(attrs=()):
    """(point format 0-3, record bytes) of the records a mask writes."""
    fmt, rb = C.c_uint32(), C.c_uint32()
    st = load_library().swz_las_record_layout(_las_mask(attrs), C.byref(fmt), C.byref(rb))
    if st != 0:
        raise SwzError(st, "swz_las_record_layout failed")
    return int(fmt.value), int(rb.value)


def las_pack_tile():
    """The stored rows one workgroup of las_pack_device takes."""
    return int(load_library().swz_las_pack_tile())


def las_image_layout(counts, attrs=()):
    """swz_las_image_layout: where every node's point records lie in one contiguous image.  Returns a dict of the per-node
    arrays offset / size and the image's total size."""
    cnt = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    m = cnt.shape[0]
    out = {k: np.empty(m, dtype=np.uint64) for k in ("offset", "size")}
    total = C.c_uint64()
    st = load_library().swz_las_image_layout(m, cnt.ctypes.data_as(_u64p), _las_mask(attrs), out["offset"].ctypes.data_as(_u64p),
                                             out["size"].ctypes.data_as(_u64p), C.byref(total))
    if st != 0:
        raise SwzError(st, "swz_las_image_layout failed")
    out["total"] = int(total.value)
    return out


def las_write_node(path, count, body, attrs, box_min, box_max, scale):
    """One LAS 1.2 node file from packed records (a slice of the image las_pack_device wrote; host only)."""
    b = np.ascontiguousarray(body, dtype=np.uint8).reshape(-1)
    fmt, rb = las_record_layout(attrs)
    if b.shape[0] < int(count) * rb:
        raise ValueError("the body holds %d bytes, %d records of %d need more" % (b.shape[0], count, rb))
    st = load_library().swz_las_write_node(None, os.fsencode(path), int(count), b.ctypes.data, _las_mask(attrs), _vec3(box_min),
                                           _vec3(box_max), float(scale))
    if st != 0:
        raise SwzError(st, "swz_las_write_node(%s) failed" % path)


def las_write_node_rows(path, xyz, attrs, box_min, box_max, scale, write=None):
    """The same file from unpacked rows: double positions plus the columns of attrs (dict name -> array), converted on the
    host.  write: the columns to put into the records (default: all of attrs)."""
    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    cols, keep = _host_columns(attrs, x.shape[0])
    if write is None:
        write = list(attrs or {})
    st = load_library().swz_las_write_node_rows(None, os.fsencode(path), x.shape[0], x.ctypes.data_as(_dp), C.byref(cols),
                                                _las_mask(write), _vec3(box_min), _vec3(box_max), float(scale))
    if st != 0:
        raise SwzError(st, "swz_las_write_node_rows(%s) failed" % path)


def las_read_header(path):
    """Header of a LAS node file: dict of count, point_format, record_bytes, offset_to_point_data, scale, offset, min, max."""
    count, fmt, rb, at, lay = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32(), _LasLayout()
    st = load_library().swz_las_read_header(None, os.fsencode(path), C.byref(count), C.byref(fmt), C.byref(rb), C.byref(at),
                                            C.byref(lay))
    if st != 0:
        raise SwzError(st, "swz_las_read_header(%s) failed" % path)
    return dict(count=int(count.value), point_format=int(fmt.value), record_bytes=int(rb.value), offset_to_point_data=int(at.value),
                scale=list(lay.scale), offset=list(lay.offset), min=list(lay.min), max=list(lay.max))


def las_read_node(path):
    """retrieve_points of a LAS node file (formats 0-3): (xyz, dict of every attribute column a LAS record carries)."""
    head = las_read_header(path)
    n = head["count"]
    xyz = np.empty((n, 3), dtype=np.float64)
    out = {}
    for name, (idx, dt, width) in ATTRIBUTES.items():
        if name == "normal" or (name == "gps_time" and not head["point_format"] & 1) or (name == "rgb" and not head["point_format"] & 2):
            continue
        out[name] = np.empty((n, width) if width > 1 else n, dtype=dt)
    cols, keep = _host_columns(out, n)
    st = load_library().swz_las_read_node(None, os.fsencode(path), xyz.ctypes.data_as(_dp), C.byref(cols))
    if st != 0:
        raise SwzError(st, "swz_las_read_node(%s) failed" % path)
    return xyz, keep


def bin_persist_nodes(directory, nodes, xyz, attrs=None, compressed=False, ctx=None):
    """One BinaryPersistence file per node of a node table from the gathered (host) payload (host only, no GPU needed)."""
    x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    cols, keep = _host_columns(attrs, x.shape[0])
    nl, nk, no, nc = _node_columns(nodes, "level", "key", "offset", "count")
    L = load_library()
    st = L.swz_bin_persist_nodes(ctx, os.fsencode(directory), nl.shape[0], nl.ctypes.data_as(_i8p), nk.ctypes.data_as(_u64p),
                                 no.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p), x.ctypes.data_as(_dp), C.byref(cols),
                                 int(bool(compressed)))
    if st != 0:
        raise SwzError(st, (L.swz_last_error(ctx) or b"").decode() if ctx else "swz_bin_persist_nodes(%s) failed" % directory)


def node_boxes_tile():
    """Stored rows one workgroup of swz_node_boxes_device takes (tests place their edges by it)."""
    return int(load_library().swz_node_boxes_tile())


def bin_pack_tile():
    """The stored rows one workgroup of bin_pack_device takes."""
    return int(load_library().swz_bin_pack_tile())


def bin_layout(counts, attrs=()):
    """swz_bin_layout: where every node's BIN file lies in one contiguous image.  Returns a dict of the per-node arrays
    offset / size (of the body, a multiple of 8) / file_size and the image's total size."""
    cnt = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    m = cnt.shape[0]
    out = {k: np.empty(m, dtype=np.uint64) for k in ("offset", "size", "file_size")}
    total = C.c_uint64()
    st = load_library().swz_bin_layout(m, cnt.ctypes.data_as(_u64p), _las_mask(attrs), out["offset"].ctypes.data_as(_u64p),
                                       out["size"].ctypes.data_as(_u64p), out["file_size"].ctypes.data_as(_u64p), C.byref(total))
    if st != 0:
        raise SwzError(st, "swz_bin_layout failed")
    out["total"] = int(total.value)
    return out


def bin_persist_nodes_image(directory, nodes, image, attrs=(), compressed=False, ctx=None):
    """One BIN (.binz: zlib) file per node of a node table out of a host copy of the image bin_pack_device wrote."""
    img = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1)
    nl, nk, nc = _node_columns(nodes, "level", "key", "count")
    if not (nl.shape[0] == nk.shape[0] == nc.shape[0]):
        raise ValueError("the columns of the node table differ in length")
    L = load_library()
    st = L.swz_bin_persist_nodes_image(ctx, os.fsencode(directory), nl.shape[0], nl.ctypes.data_as(_i8p), nk.ctypes.data_as(_u64p),
                                       nc.ctypes.data_as(_u64p), img.ctypes.data, img.shape[0], _las_mask(attrs),
                                       int(bool(compressed)))
    if st != 0:
        raise SwzError(st, (L.swz_last_error(ctx) or b"").decode() if ctx else "swz_bin_persist_nodes_image(%s) failed" % directory)


# swz_tiler_write_output: the formats, its parameters and what it reports
OUTPUT_FORMATS = {"BIN": 0, "BINZ": 1, "3DTILES": 2, "LAS": 3, "ENTWINE_LAS": 4}
OUT_TIGHT_BOUNDS = 1


class _OutputParams(C.Structure):
    _fields_ = [("format", C.c_int), ("attribute_mask", C.c_uint32), ("rgb_mapping", C.c_int), ("flags", C.c_uint32),
                ("global_offset", C.c_double * 3), ("chunk_points", C.c_uint64), ("ept", C.POINTER(_EptJson))]


class _OutputStats(C.Structure):
    _fields_ = [("nodes", C.c_uint64), ("stored_points", C.c_uint64), ("bytes_written", C.c_uint64), ("chunks", C.c_uint64),
                ("pack_ms", C.c_double), ("copy_ms", C.c_double), ("write_ms", C.c_double), ("wall_ms", C.c_double)]


def output_flags_check(format, flags):
    """swz_output_flags_check: raises SwzError with the text write_output refuses these flags with for the format."""
    fmt = OUTPUT_FORMATS[format] if isinstance(format, str) else int(format)
    what = C.c_char_p()
    st = load_library().swz_output_flags_check(fmt, int(flags), C.byref(what))
    if st != 0:
        raise SwzError(st, (what.value or b"").decode())


def output_chunks(counts, chunk_points):
    """swz_output_chunks: the first node of every chunk write_output cuts a node table into, and one entry past the last."""
    cnt = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    num = C.c_uint64()
    L = load_library()
    if L.swz_output_chunks(cnt.shape[0], cnt.ctypes.data_as(_u64p), int(chunk_points), 0, None, C.byref(num)) != 0:
        raise ValueError("bad node table")
    first = np.zeros(int(num.value) + 1, dtype=np.uint64)
    if L.swz_output_chunks(cnt.shape[0], cnt.ctypes.data_as(_u64p), int(chunk_points), int(num.value), first.ctypes.data_as(_u64p),
                           C.byref(num)) != 0:
        raise ValueError("bad node table")
    return first


def merge_shard_node_tables(tables, max_nodes=None, count_only=False):
    """swz_merge_shard_node_tables (host, no GPU): `tables` holds one (level, key, count) triple of arrays per shard, as
    swz_tiler_node_table gives them for the shard's tiler.  Returns (level, key, count, shard) of the merged table, ordered by
    (level, node key): one root entry whose count is the sum of the parts with shard -1, the owner for every other node.
    count_only: every output is NULL and only the number of nodes comes back.  max_nodes: the capacity of the outputs
    (default: exactly what is needed).  ValueError for a capacity that is too small, RuntimeError for a node below the root
    that lies on two shards."""
    L = load_library()
    n = len(tables)
    lv = [np.ascontiguousarray(t[0], dtype=np.int8).reshape(-1) for t in tables]
    ky = [np.ascontiguousarray(t[1], dtype=np.uint64).reshape(-1) for t in tables]
    ct = [np.ascontiguousarray(t[2], dtype=np.uint64).reshape(-1) for t in tables]
    nn = (C.c_uint64 * max(n, 1))(*[a.shape[0] for a in lv])
    pl = (_i8p * max(n, 1))(*[a.ctypes.data_as(_i8p) for a in lv])
    pk = (_u64p * max(n, 1))(*[a.ctypes.data_as(_u64p) for a in ky])
    pc = (_u64p * max(n, 1))(*[a.ctypes.data_as(_u64p) for a in ct])
    num = C.c_uint64()

    def check(st):
        if st == 7:
            raise RuntimeError("a node below the root lies on two shards")
        if st != 0:
            raise ValueError("swz_merge_shard_node_tables: bad argument (max_nodes too small?)")

    check(L.swz_merge_shard_node_tables(n, nn, pl, pk, pc, 0, None, None, None, None, C.byref(num)))
    if count_only:
        return int(num.value)
    cap = int(num.value) if max_nodes is None else int(max_nodes)
    level = np.zeros(max(cap, 1), dtype=np.int8)
    key = np.zeros(max(cap, 1), dtype=np.uint64)
    count = np.zeros(max(cap, 1), dtype=np.uint64)
    shard = np.zeros(max(cap, 1), dtype=np.int32)
    check(L.swz_merge_shard_node_tables(n, nn, pl, pk, pc, cap, level.ctypes.data_as(_i8p), key.ctypes.data_as(_u64p),
                                        count.ctypes.data_as(_u64p), shard.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(num)))
    m = int(num.value)
    return level[:m], key[:m], count[:m], shard[:m]


def las_persist_nodes(directory, nodes, image, attrs, box_min, box_max, scale, naming=LAS_NAMING_POTREE, ctx=None):
    """One LAS file per node of a node table out of a host copy of the image las_pack_device wrote.  box_min / box_max
    (num_nodes x 3) and scale (num_nodes) are the nodes' boxes and scales; naming: LAS_NAMING_POTREE or LAS_NAMING_ENTWINE."""
    img = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1)
    nl, nk, nc = _node_columns(nodes, "level", "key", "count")
    mn = np.ascontiguousarray(box_min, dtype=np.float64).reshape(-1, 3)
    mx = np.ascontiguousarray(box_max, dtype=np.float64).reshape(-1, 3)
    sc = np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
    if not (mn.shape[0] == mx.shape[0] == sc.shape[0] == nl.shape[0] == nk.shape[0] == nc.shape[0]):
        raise ValueError("the node table, the boxes and the scales differ in length")
    L = load_library()
    st = L.swz_las_persist_nodes(ctx, os.fsencode(directory), nl.shape[0], nl.ctypes.data_as(_i8p), nk.ctypes.data_as(_u64p),
                                 nc.ctypes.data_as(_u64p), mn.ctypes.data_as(_dp), mx.ctypes.data_as(_dp), sc.ctypes.data_as(_dp),
                                 img.ctypes.data, img.shape[0], _las_mask(attrs), int(naming))
    if st != 0:
        raise SwzError(st, (L.swz_last_error(ctx) or b"").decode() if ctx else "swz_las_persist_nodes(%s) failed" % directory)


def ept_create_dirs(directory):
    """ept-data, ept-hierarchy and ept-sources under directory (create_ept_folder_structure)."""
    st = load_library().swz_ept_create_dirs(None, os.fsencode(directory))
    if st != 0:
        raise SwzError(st, "swz_ept_create_dirs(%s) failed" % directory)


def ept_hierarchy_write(directory, nodes):
    """swz_ept_hierarchy_write: directory/ept-hierarchy/*.json of a node table (dict of level / key / count)."""
    nl, nk, nc = _node_columns(nodes, "level", "key", "count")
    if not (nl.shape[0] == nk.shape[0] == nc.shape[0]):
        raise ValueError("the columns of the node table differ in length")
    st = load_library().swz_ept_hierarchy_write(None, os.fsencode(directory), nl.shape[0], nl.ctypes.data_as(_i8p),
                                                nk.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p))
    if st != 0:
        raise SwzError(st, "swz_ept_hierarchy_write(%s) failed" % directory)


def ept_json_write(path, bounds, conforming_bounds, points, attrs=(), span=0.0, srs=None, version=""):
    """swz_ept_json_write: ept.json.  bounds / conforming_bounds: (min, max); attrs: the attributes of the schema besides
    the position; srs: dict of authority / horizontal / wkt."""
    srs = srs or {}
    e = _EptJson(_vec3(bounds[0]), _vec3(bounds[1]), _vec3(conforming_bounds[0]), _vec3(conforming_bounds[1]), int(points),
                 _las_mask(attrs), 0, float(span), srs.get("authority", "").encode(), srs.get("horizontal", "").encode(),
                 srs.get("wkt", "").encode(), version.encode())
    st = load_library().swz_ept_json_write(None, os.fsencode(path), C.byref(e))
    if st != 0:
        raise SwzError(st, "swz_ept_json_write(%s) failed" % path)



LAS_FILE_OK, LAS_FILE_UNREADABLE, LAS_FILE_BAD_HEADER, LAS_FILE_COMPRESSED = 0, 1, 2, 3
# ---- a written data set found again and converted (swz_dataset_scan, swz_convert_dataset)
DATASET_ROOT_ABSENT, DATASET_ROOT_PROPERTIES, DATASET_ROOT_EPT = 0, 1, 2


class _DatasetInfo(C.Structure):
    _fields_ = [("format", C.c_int32), ("attribute_mask", C.c_uint32), ("root_source", C.c_uint32), ("spacing_at_root", C.c_float),
                ("root_min", C.c_double * 3), ("root_max", C.c_double * 3), ("num_nodes", C.c_uint64), ("points", C.c_uint64),
                ("max_level", C.c_int32), ("reserved", C.c_uint32)]


class _BinSegment(C.Structure):
    _fields_ = [("first_row", C.c_uint64), ("count", C.c_uint64), ("byte_offset", C.c_uint64), ("mask", C.c_uint32),
                ("reserved", C.c_uint32)]


class _PntsSegment(C.Structure):
    _fields_ = [("first_row", C.c_uint64), ("count", C.c_uint64), ("position_offset", C.c_uint64), ("rgb_offset", C.c_uint64),
                ("intensity_offset", C.c_uint64), ("mask", C.c_uint32), ("reserved", C.c_uint32)]


CONVERT_LOSSY_SOURCE = 1


class _ConvertParams(C.Structure):
    _fields_ = [("out", _OutputParams), ("max_depth", C.c_int32), ("root_given", C.c_uint32), ("root_min", C.c_double * 3),
                ("root_max", C.c_double * 3), ("spacing_at_root", C.c_float), ("source_flags", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class _ConvertStats(C.Structure):
    _fields_ = [("nodes", C.c_uint64), ("points", C.c_uint64), ("bytes_read", C.c_uint64), ("bytes_written", C.c_uint64),
                ("chunks", C.c_uint64), ("read_ms", C.c_double), ("unpack_ms", C.c_double), ("pack_ms", C.c_double),
                ("copy_ms", C.c_double), ("write_ms", C.c_double), ("wall_ms", C.c_double)]


def properties_json_write(directory, root_min, root_max, spacing_at_root, processed_points):
    """swz_properties_json_write: directory/properties.json as the reference's tiler writes it (host only)."""
    st = load_library().swz_properties_json_write(None, os.fsencode(directory), _vec3(root_min), _vec3(root_max), float(spacing_at_root),
                                                  int(processed_points))
    if st != 0:
        raise SwzError(st, "swz_properties_json_write(%s) failed" % directory)


def properties_json_read(directory):
    """swz_properties_json_read: dict(root_min, root_max, spacing_at_root, processed_points) of directory/properties.json."""
    mn, mx = (C.c_double * 3)(), (C.c_double * 3)()
    spacing, points = C.c_float(), C.c_uint64()
    st = load_library().swz_properties_json_read(None, os.fsencode(directory), mn, mx, C.byref(spacing), C.byref(points))
    if st != 0:
        raise SwzError(st, "swz_properties_json_read(%s) failed" % directory)
    return dict(root_min=np.array(list(mn)), root_max=np.array(list(mx)), spacing_at_root=float(spacing.value),
                processed_points=int(points.value))


def dataset_scan(directory, max_depth=None):
    """swz_dataset_scan (host, no GPU): the written data set in directory as a dict -- format (a key of OUTPUT_FORMATS),
    attrs / attribute_mask, nodes (level, key, count in the order of Tiler.node_table), points, max_level, root_source
    (DATASET_ROOT_*), and root_min / root_max / spacing_at_root unless the source is DATASET_ROOT_ABSENT.  max_depth: only
    the nodes of depth (level + 1) <= max_depth; None: all.  A refusal raises SwzError with the library's text."""
    L = load_library()
    depth = -1 if max_depth is None else int(max_depth)
    info, num = _DatasetInfo(), C.c_uint64()
    why = C.create_string_buffer(4096)
    st = L.swz_dataset_scan_why(os.fsencode(directory), depth, C.byref(info), 0, None, None, None, C.byref(num), why, len(why))
    if st != 0:
        raise SwzError(st, why.value.decode(errors="replace"))
    cap = max(int(num.value), 1)
    nl, nk, nc = np.empty(cap, dtype=np.int8), np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint64)
    st = L.swz_dataset_scan_why(os.fsencode(directory), depth, C.byref(info), cap, nl.ctypes.data_as(_i8p), nk.ctypes.data_as(_u64p),
                                nc.ctypes.data_as(_u64p), C.byref(num), why, len(why))
    if st != 0:
        raise SwzError(st, why.value.decode(errors="replace"))
    m = int(num.value)
    names = {v: k for k, v in OUTPUT_FORMATS.items()}
    out = dict(format=names[int(info.format)], attribute_mask=int(info.attribute_mask), attrs=attribute_names(info.attribute_mask),
               nodes=dict(level=nl[:m].copy(), key=nk[:m].copy(), count=nc[:m].copy()), points=int(info.points),
               max_level=int(info.max_level), root_source=int(info.root_source))
    if info.root_source != DATASET_ROOT_ABSENT:
        out.update(root_min=np.array(list(info.root_min)), root_max=np.array(list(info.root_max)),
                   spacing_at_root=float(info.spacing_at_root))
    return out


def bin_unpack_tile():
    """Output rows one workgroup of bin_unpack_segments_device takes (tests place their edges by it)."""
    return int(load_library().swz_bin_unpack_tile())


def pnts_unpack_tile():
    """Output rows one workgroup of pnts_unpack_segments_device takes."""
    return int(load_library().swz_pnts_unpack_tile())


def _ept_struct(ept):
    srs = ept.get("srs") or {}
    return _EptJson(_vec3(ept["bounds"][0]), _vec3(ept["bounds"][1]), _vec3(ept["conforming_bounds"][0]),
                    _vec3(ept["conforming_bounds"][1]), int(ept["points"]), _las_mask(ept.get("attrs", ())), 0,
                    float(ept.get("span", 0.0)), srs.get("authority", "").encode(), srs.get("horizontal", "").encode(),
                    srs.get("wkt", "").encode(), ept.get("version", "").encode())


def convert_dataset(ctx, src, dst, format, attrs=None, max_depth=None, rgb_from=RGB_FROM_COLOR, global_offset=None, chunk_points=0,
                    ept=None, tight_bounds=False, root_box=None, spacing=None, flags=0, lossy_source=False, source_flags=None,
                    _world=None):
    """swz_convert_dataset: the written data set in src (BIN, BINZ, LAS or ENTWINE_LAS node files; with lossy_source=True
    also 3DTILES, whose .pnts files hold float positions, RGB and intensity only) converted into dst in another format, node
    files unpacked and packed on the device.  source_flags: the raw word, instead of lossy_source.  format, rgb_from, global_offset, chunk_points, ept,
    tight_bounds, flags: as in Tiler.write_output; attrs: the columns to write, a subset of the source's (None: all it has);
    max_depth: only the nodes of depth <= max_depth; root_box ((min, max)) and spacing: the root box and spacing_at_root,
    overriding properties.json / ept.json of src -- required when src has neither.  Returns the stats as a dict (nodes,
    points, bytes_read, bytes_written, chunks, read_ms, unpack_ms, pack_ms, copy_ms, write_ms, wall_ms)."""
    fmt = OUTPUT_FORMATS[format] if isinstance(format, str) else int(format)
    out = _OutputParams(fmt, 0xFFFFFFFF if attrs is None else _las_mask(attrs), int(rgb_from),
                        int(flags) | (OUT_TIGHT_BOUNDS if tight_bounds else 0),
                        _vec3(global_offset if global_offset is not None else (0, 0, 0)), int(chunk_points), None)
    keep = None
    if ept is not None:
        keep = _ept_struct(ept)
        out.ept = C.pointer(keep)
    if (root_box is None) != (spacing is None):
        raise ValueError("convert_dataset: root_box and spacing go together")
    given = root_box is not None
    p = _ConvertParams(out, -1 if max_depth is None else int(max_depth), 1 if given else 0,
                       _vec3(root_box[0] if given else (0, 0, 0)), _vec3(root_box[1] if given else (0, 0, 0)),
                       float(spacing) if given else 0.0,
                       int(source_flags) if source_flags is not None else (CONVERT_LOSSY_SOURCE if lossy_source else 0),
                       (C.c_uint32 * 2)(0, 0))
    stats = _ConvertStats()
    if _world is not None:   # convert_dataset_world: (srs,)
        srs = _world[0]
        ctx._check(ctx._lib.swz_convert_dataset_world(ctx._ctx, os.fsencode(src), os.fsencode(dst), C.byref(p),
                                                      srs._ref() if srs is not None else None, C.byref(stats)))
    else:
        ctx._check(ctx._lib.swz_convert_dataset(ctx._ctx, os.fsencode(src), os.fsencode(dst), C.byref(p), C.byref(stats)))
    return {k: getattr(stats, k) for k, _ in _ConvertStats._fields_}


def convert_dataset_world(ctx, src, dst, source_projection=None, format="3DTILES", **kwargs):
    """swz_convert_dataset_world: the written data set in src converted into georeferenced 3D Tiles in dst -- every chunk's
    positions mapped to ECEF on the device (source_projection: a definition string or an Srs, as in Tiler.add_las_files;
    None: no projection), every .pnts file relative to its node's own origin (RTC_CENTER = the per-axis minimum of the
    node's mapped positions), the tileset with oriented boxes.  The other arguments and the returned stats are
    convert_dataset's; format must be 3DTILES and global_offset zero (both are refused by the library otherwise)."""
    return convert_dataset(ctx, src, dst, format, _world=(_as_srs(source_projection),), **kwargs)


# ---- a written data set queried by box and depth (swz_box_select_device, swz_dataset_query_nodes, swz_dataset_query)
class _QueryParams(C.Structure):
    _fields_ = [("box_min", C.c_double * 3), ("box_max", C.c_double * 3), ("max_depth", C.c_int32), ("attribute_mask", C.c_uint32),
                ("source_flags", C.c_uint32), ("reserved", C.c_uint32), ("chunk_points", C.c_uint64)]


class _QueryStats(C.Structure):
    _fields_ = [("nodes_scanned", C.c_uint64), ("nodes_read", C.c_uint64), ("points_read", C.c_uint64), ("points_out", C.c_uint64),
                ("bytes_read", C.c_uint64), ("chunks", C.c_uint64), ("read_ms", C.c_double), ("unpack_ms", C.c_double),
                ("select_ms", C.c_double), ("copy_ms", C.c_double), ("wall_ms", C.c_double)]


def box_select_tile():
    """Rows one workgroup of box_select_device takes (tests place their edges by it)."""
    return int(load_library().swz_box_select_tile())


def _query_params(box_min, box_max, max_depth, attrs, lossy_source, chunk_points, source_flags=None, reserved=0):
    return _QueryParams(_vec3(box_min), _vec3(box_max), -1 if max_depth is None else int(max_depth),
                        0xFFFFFFFF if attrs is None else _las_mask(attrs),
                        int(source_flags) if source_flags is not None else (CONVERT_LOSSY_SOURCE if lossy_source else 0),
                        int(reserved), int(chunk_points))


def _ref(struct):
    return None if struct is None else C.byref(struct)


def _query_nodes(entry, directory, params, *region_ref, with_read=False):
    """the node table of a query as a dict.  entry: swz_dataset_query_nodes_why, or swz_dataset_query_region_nodes_why with
    its region argument in region_ref, or (with_read) swz_dataset_query_filtered_nodes_why with its region and filter, whose
    table has one more array: read, a bool per node; once for the number of nodes, once for the table"""
    head = (os.fsencode(directory), C.byref(params)) + region_ref
    num, bound = C.c_uint64(), C.c_uint64()
    why = C.create_string_buffer(4096)

    def call(cap, *arrays):
        st = entry(*head, cap, *arrays, C.byref(num), C.byref(bound), why, len(why))
        if st != 0:
            raise SwzError(st, why.value.decode(errors="replace"))

    call(0, *[None] * (4 if with_read else 3))
    cap = max(int(num.value), 1)
    nl, nk, nc = np.empty(cap, dtype=np.int8), np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint64)
    rd = np.empty(cap, dtype=np.uint8)
    call(cap, nl.ctypes.data_as(_i8p), nk.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p), *([rd.ctypes.data] if with_read else []))
    m = int(num.value)
    out = dict(level=nl[:m].copy(), key=nk[:m].copy(), count=nc[:m].copy())
    if with_read:
        out["read"] = rd[:m].astype(bool)
    out["points_bound"] = int(bound.value)
    return out


def dataset_query_nodes(directory, box_min, box_max, max_depth=None, lossy_source=False, source_flags=None, reserved=0):
    """swz_dataset_query_nodes (host, no GPU): the nodes of the written data set in directory that a query of the closed box
    [box_min, box_max] reads, as dict(level, key, count -- in the order of dataset_scan --, points_bound: the sum of the
    counts, the capacity that always suffices).  A node drops out only if its widened box misses the query box.  max_depth:
    only the nodes of depth <= max_depth; lossy_source: admits a 3DTILES source (source_flags: the raw word instead;
    reserved is passed on).  A refusal raises SwzError with the library's text."""
    p = _query_params(box_min, box_max, max_depth, None, lossy_source, 0, source_flags, reserved)
    return _query_nodes(load_library().swz_dataset_query_nodes_why, directory, p)


def _dataset_query(ctx, directory, box_min, box_max, max_depth, attrs, lossy_source, chunk_points, return_nodes, capacity, region, filter,
                   entry):
    """dataset_query, dataset_query_region and dataset_query_filtered.  entry names the C function: swz_dataset_query (region
    and filter are not passed), swz_dataset_query_region (filter is not) or swz_dataset_query_filtered."""
    import torch

    if entry == "swz_dataset_query":
        table = dataset_query_nodes(directory, box_min, box_max, max_depth, lossy_source)
    else:
        table = dataset_query_region_nodes(directory, box_min, box_max, region, max_depth, lossy_source)
    names = attribute_names(dataset_scan(directory, max_depth)["attribute_mask"]) if attrs is None else list(attrs)
    rows = int(table["points_bound"]) if capacity is None else int(capacity)
    dev = torch.device("cuda", ctx.device)
    xyz = torch.empty((max(rows, 1), 3), dtype=torch.float64, device=dev)
    cols = {}
    for name in names:
        _, dt, width = ATTRIBUTES[name]
        cols[name] = torch.empty((max(rows, 1), width) if width > 1 else (max(rows, 1),), dtype=getattr(torch, np.dtype(dt).name), device=dev)
    node = torch.empty(max(rows, 1), dtype=torch.int32, device=dev) if return_nodes else None
    p = _query_params(box_min, box_max, max_depth, names, lossy_source, chunk_points)
    d_cols = device_columns({k: v.data_ptr() for k, v in cols.items()})
    count, stats = C.c_uint64(), _QueryStats()
    d_node = C.c_void_p(node.data_ptr()) if return_nodes else None
    rg = None if region is None else region._struct()
    fl = None if filter is None else filter._struct()
    selection = {"swz_dataset_query": (), "swz_dataset_query_region": (_ref(rg),), "swz_dataset_query_filtered": (_ref(rg), _ref(fl))}[entry]
    ctx._check(getattr(ctx._lib, entry)(ctx._ctx, os.fsencode(directory), C.byref(p), *selection, rows, C.c_void_p(xyz.data_ptr()),
                                        C.byref(d_cols), d_node, C.byref(count), C.byref(stats)))
    m = int(count.value)
    out = dict(xyz=xyz[:m], node=node[:m] if return_nodes else None, count=m,
               stats={k: getattr(stats, k) for k, _ in _QueryStats._fields_})
    out.update({k: v[:m] for k, v in cols.items()})
    return out


def dataset_query(ctx, directory, box_min, box_max, max_depth=None, attrs=None, lossy_source=False, chunk_points=0, return_nodes=False,
                  capacity=None):
    """swz_dataset_query: the points of the written data set in directory inside the closed box [box_min, box_max], of the nodes
    of depth <= max_depth (None: all), streamed from the node files and selected on the device.  attrs: the columns wanted, a
    subset of the source's (None: all it has); lossy_source: admits a 3DTILES source; chunk_points: as in Tiler.write_output.
    The outputs are torch tensors on the context's device with points_bound rows (dataset_query_nodes; capacity: another row
    count -- one that is too small is refused), trimmed to the count: dict(xyz, <column names>, node (with return_nodes: per
    point the index into dataset_query_nodes' table, else None), count, stats (the fields of swz_query_stats))."""
    return _dataset_query(ctx, directory, box_min, box_max, max_depth, attrs, lossy_source, chunk_points, return_nodes, capacity, None, None,
                          "swz_dataset_query")


# ---- the same by region: the box cut by planes or by a polygon in x-y (swz_region_select_device, swz_dataset_query_region*)
REGION_BOX, REGION_PLANES, REGION_POLYGON = 0, 1, 2
REGION_MAX_PLANES, REGION_MAX_VERTICES = 16, 1024


class _Region(C.Structure):
    _fields_ = [("kind", C.c_int32), ("count", C.c_uint32), ("values", C.POINTER(C.c_double)), ("reserved", C.c_uint64)]


class Region:
    """A swz_region: what cuts the closed box of a query further.  Region.planes(k x 4 rows a, b, c, d): the rows with
    ((a*x + b*y) + c*z) + d >= 0 for every plane (1 to 16; a frustum is six, frustum_planes).  Region.polygon(m x 2 vertices):
    the rows inside one outline in the x-y plane by the even-odd rule (3 to 1024 vertices; concave and self-intersecting
    outlines are defined), over the box's z range.  Region.box(): nothing more.  The formulas, operation for operation, are in
    include/swz_gpu.h.  Nothing is checked here: the library refuses what it does not take (count, reserved and a None for the
    values are passed on as they are)."""

    def __init__(self, kind, values=None, count=None, reserved=0):
        self.kind, self.reserved = int(kind), int(reserved)
        self.values = None if values is None else np.ascontiguousarray(values, dtype=np.float64)
        self.count = int(count) if count is not None else 0 if self.values is None or self.kind == REGION_BOX else len(self.values)

    @classmethod
    def box(cls):
        return cls(REGION_BOX)

    @classmethod
    def planes(cls, array_k4):
        return cls(REGION_PLANES, np.asarray(array_k4, dtype=np.float64).reshape(-1, 4))

    @classmethod
    def polygon(cls, array_m2):
        return cls(REGION_POLYGON, np.asarray(array_m2, dtype=np.float64).reshape(-1, 2))

    def _struct(self):
        """the ctypes struct; it points into self.values, which lives as long as self"""
        return _Region(self.kind, self.count, None if self.values is None else self.values.ctypes.data_as(_dp), self.reserved)


def frustum_planes(view_proj):
    """The six inward planes (rows a, b, c, d) of a row-major 4 x 4 view-projection matrix M, clip = M (x, y, z, 1), with the
    clip volume -w <= x, y, z <= w: the usual sums and differences of M's rows with its last row -- left, right, bottom, top,
    near, far --, every row divided by the length of its normal.  The doubles returned are the planes a query takes; nothing
    is promised about how exactly they follow the matrix."""
    m = np.asarray(view_proj, dtype=np.float64).reshape(4, 4)
    rows = np.array([m[3] + m[0], m[3] - m[0], m[3] + m[1], m[3] - m[1], m[3] + m[2], m[3] - m[2]])
    return rows / np.sqrt((rows[:, :3] ** 2).sum(axis=1))[:, None]


def _region_box(directory, box_min, box_max, region, max_depth):
    """the box of a region query: given, or for a polygon its x-y bounds and the root box's z"""
    if box_min is not None and box_max is not None:
        return box_min, box_max
    if region is None or region.kind != REGION_POLYGON or region.values is None or (box_min is None) != (box_max is None):
        raise ValueError("a region query needs box_min and box_max (only a polygon may leave both out)")
    scan = dataset_scan(directory, max_depth)
    if scan["root_source"] == DATASET_ROOT_ABSENT or scan["format"] == "3DTILES":
        raise ValueError("no box to derive: the source has no root box, or stores positions relative to an RTC_CENTER")
    xy = region.values.reshape(-1, 2)
    return ([xy[:, 0].min(), xy[:, 1].min(), scan["root_min"][2]], [xy[:, 0].max(), xy[:, 1].max(), scan["root_max"][2]])


def dataset_query_region_nodes(directory, box_min, box_max, region, max_depth=None, lossy_source=False, source_flags=None, reserved=0):
    """swz_dataset_query_region_nodes (host, no GPU): dataset_query_nodes for the box cut by region (a Region; None: the box
    alone).  A node drops out only if its widened box misses the query box or cannot hold a row the region accepts.  box_min
    and box_max may both be None for a polygon: its x-y bounds and the root box's z.  The dict is dataset_query_nodes'."""
    box_min, box_max = _region_box(directory, box_min, box_max, region, max_depth)
    p = _query_params(box_min, box_max, max_depth, None, lossy_source, 0, source_flags, reserved)
    rg = None if region is None else region._struct()
    return _query_nodes(load_library().swz_dataset_query_region_nodes_why, directory, p, _ref(rg))


def dataset_query_region(ctx, directory, box_min, box_max, region, max_depth=None, attrs=None, lossy_source=False, chunk_points=0,
                         return_nodes=False, capacity=None):
    """swz_dataset_query_region: dataset_query for the box cut by region (a Region; None: the box alone) -- the same keywords,
    the same result dict; node indexes dataset_query_region_nodes' table.  box_min and box_max may both be None for a polygon:
    its x-y bounds and the root box's z; planes need the box."""
    box_min, box_max = _region_box(directory, box_min, box_max, region, max_depth)
    return _dataset_query(ctx, directory, box_min, box_max, max_depth, attrs, lossy_source, chunk_points, return_nodes, capacity, region, None,
                          "swz_dataset_query_region")


# ---- the same with a filter: clauses over the attribute columns, evaluated on the device behind the region
FILTER_RANGE, FILTER_SET, FILTER_NOT, FILTER_MAX_CLAUSES = 0, 1, 0x100, 8


class _FilterClause(C.Structure):
    _fields_ = [("attribute", C.c_int32), ("kind", C.c_uint32), ("lo", C.c_double), ("hi", C.c_double), ("set", C.c_uint64 * 4)]


class _Filter(C.Structure):
    _fields_ = [("count", C.c_uint32), ("reserved", C.c_uint32), ("clause", _FilterClause * FILTER_MAX_CLAUSES)]


class Filter:
    """A swz_filter: up to 8 clauses over the scalar attribute columns; a row passes iff it passes every clause.
    Filter().range("gps_time", lo, hi): lo <= value <= hi as doubles, closed, +-inf for an open end (a NaN value fails);
    .any_of("classification", [2, 9]): the value is one of these (one-byte columns; scan_angle_rank -1 is bit 255);
    .none_of("classification", [7, 18]): it is none of them.  An attribute is a name of ATTRIBUTES or its index.  The methods
    return self.  Nothing is checked here beyond what cannot be stored (a ninth clause, a set value outside a byte): the library
    refuses what it does not take (check()), and clause(...) appends a raw one."""

    def __init__(self, reserved=0):
        self.clauses, self.reserved, self.count = [], int(reserved), None   # count: None is len(clauses)

    @staticmethod
    def _index(attribute):
        return int(attribute) if isinstance(attribute, (int, np.integer)) else ATTRIBUTES[attribute][0]

    def clause(self, attribute, kind, lo=0.0, hi=0.0, bits=(0, 0, 0, 0)):
        if len(self.clauses) >= FILTER_MAX_CLAUSES:
            raise ValueError("a filter holds %d clauses at the most" % FILTER_MAX_CLAUSES)
        self.clauses.append((self._index(attribute), int(kind), float(lo), float(hi), tuple(int(w) for w in bits)))
        return self

    def range(self, attribute, lo, hi, negate=False):
        return self.clause(attribute, FILTER_RANGE | (FILTER_NOT if negate else 0), lo, hi)

    @staticmethod
    def _bits(values):
        words = [0, 0, 0, 0]
        for v in values:
            v = int(v)
            if not -128 <= v <= 255:
                raise ValueError("a set holds the values of one byte")
            words[(v & 255) >> 6] |= 1 << (v & 63)
        return words

    def any_of(self, attribute, values):
        return self.clause(attribute, FILTER_SET, bits=self._bits(values))

    def none_of(self, attribute, values):
        return self.clause(attribute, FILTER_SET | FILTER_NOT, bits=self._bits(values))

    def attributes(self):
        """the mask of the attributes the clauses name"""
        mask = 0
        for c in self.clauses:
            mask |= 1 << c[0] if 0 <= c[0] < 32 else 0
        return mask

    def _struct(self):
        f = _Filter(len(self.clauses) if self.count is None else int(self.count), self.reserved)
        for k, (attribute, kind, lo, hi, bits) in enumerate(self.clauses):
            f.clause[k] = _FilterClause(attribute, kind, lo, hi, (C.c_uint64 * 4)(*bits))
        return f

    def check(self):
        """swz_filter_check (host, no GPU): raises SwzError with the library's text if the library refuses the filter"""
        why = C.create_string_buffer(1024)
        f = self._struct()
        st = load_library().swz_filter_check(C.byref(f), why, len(why))
        if st != 0:
            raise SwzError(st, why.value.decode(errors="replace"))
        return self


def dataset_query_filtered(ctx, directory, box_min, box_max, region=None, filter=None, max_depth=None, attrs=None, lossy_source=False,
                           chunk_points=0, return_nodes=False, capacity=None):
    """swz_dataset_query_filtered: dataset_query_region for the rows that also pass filter (a Filter; None: no filter) -- the same
    keywords, the same result dict.  attrs are the columns returned; the columns the filter names are read for it whether
    attrs holds them or not.  node indexes dataset_query_region_nodes' table, and stats["points_read"] - stats["points_out"] is
    what region and filter refused.  Where dataset_summarize has left node-summaries.swz in directory, the nodes the filter cannot
    reach (dataset_query_filtered_nodes) are not read: the outputs are the same bytes, stats["nodes_read"], ["points_read"],
    ["bytes_read"] and ["chunks"] shrink."""
    box_min, box_max = _region_box(directory, box_min, box_max, region, max_depth)
    if filter is not None:
        filter.check()   # (before the query scans the directory for its table)
    return _dataset_query(ctx, directory, box_min, box_max, max_depth, attrs, lossy_source, chunk_points, return_nodes, capacity, region, filter,
                          "swz_dataset_query_filtered")


# ---- per-node attribute summaries: node-summaries.swz beside a written data set lets a filtered query skip node files
SUMMARY_HAS_NAN = 1
SUMMARY_SCALARS = 0xFFC
# an entry (swz_attr_summary) as numpy sees it: 56 bytes
SUMMARY_DTYPE = np.dtype([("lo", "<f8"), ("hi", "<f8"), ("set", "<u8", (4,)), ("flags", "<u4"), ("reserved", "<u4")])


class _SummarizeStats(C.Structure):
    _fields_ = [("nodes", C.c_uint64), ("points", C.c_uint64), ("bytes_read", C.c_uint64), ("chunks", C.c_uint64), ("read_ms", C.c_double),
                ("unpack_ms", C.c_double), ("summary_ms", C.c_double), ("copy_ms", C.c_double), ("wall_ms", C.c_double)]


def _summary_mask(attrs):
    """names or a mask => the mask; nothing is checked (the library refuses what it does not take)"""
    if isinstance(attrs, (int, np.integer)):
        return int(attrs)
    mask = 0
    for name in attrs:
        mask |= 1 << ATTRIBUTES[name][0]
    return mask


def node_summaries_tile():
    """Rows one workgroup of node_summaries_device takes (tests place their edges by it)."""
    return int(load_library().swz_node_summaries_tile())


def dataset_summaries_write(directory, format, attrs, nodes, entries):
    """swz_dataset_summaries_write (host, no GPU): directory/node-summaries.swz out of a node table (dict of level / key / count in
    (level, Morton index) order) and entries, an array of SUMMARY_DTYPE of shape (nodes, columns): entry (k, j) is node k and
    the j-th of attrs (names or a mask) in ascending attribute index.  format: a key of OUTPUT_FORMATS or its value."""
    fmt = OUTPUT_FORMATS[format] if isinstance(format, str) else int(format)
    nl, nk, nc = _node_columns(nodes, "level", "key", "count")
    mask = _summary_mask(attrs)
    ent = np.ascontiguousarray(entries, dtype=SUMMARY_DTYPE).reshape(-1)
    if ent.shape[0] != nl.shape[0] * bin(mask & 0xFFFFFFFF).count("1"):
        raise ValueError("entries must hold one entry per node and column of the mask")
    why = C.create_string_buffer(1024)
    st = load_library().swz_dataset_summaries_write(os.fsencode(directory), fmt, mask, nl.shape[0], nl.ctypes.data_as(_i8p), nk.ctypes.data_as(_u64p),
                                                    nc.ctypes.data_as(_u64p), ent.ctypes.data, why, len(why))
    if st != 0:
        raise SwzError(st, why.value.decode(errors="replace"))


def dataset_summaries_read(directory):
    """swz_dataset_summaries_read (host, no GPU): None when directory holds no node-summaries.swz, else dict(format (a key of
    OUTPUT_FORMATS), attribute_mask, attrs, points, nodes (level, key, count), entries (SUMMARY_DTYPE, nodes x columns)).  A
    file that fails its checks raises SwzError with the library's text."""
    L = load_library()
    present, fmt, mask, num, points = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    why = C.create_string_buffer(1024)

    def call(cap, *arrays):
        st = L.swz_dataset_summaries_read(os.fsencode(directory), C.byref(present), C.byref(fmt), C.byref(mask), C.byref(num), C.byref(points),
                                          cap, *arrays, why, len(why))
        if st != 0:
            raise SwzError(st, why.value.decode(errors="replace"))

    call(0, None, None, None, None)
    if not present.value:
        return None
    m, cols = int(num.value), bin(mask.value).count("1")
    nl, nk, nc = np.empty(max(m, 1), dtype=np.int8), np.empty(max(m, 1), dtype=np.uint64), np.empty(max(m, 1), dtype=np.uint64)
    ent = np.zeros(max(m * cols, 1), dtype=SUMMARY_DTYPE)
    call(m, nl.ctypes.data_as(_i8p), nk.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p), ent.ctypes.data)
    names = {v: k for k, v in OUTPUT_FORMATS.items()}
    return dict(format=names[int(fmt.value)], attribute_mask=int(mask.value), attrs=attribute_names(mask.value), points=int(points.value),
                nodes=dict(level=nl[:m].copy(), key=nk[:m].copy(), count=nc[:m].copy()), entries=ent[:m * cols].reshape(m, cols).copy())


def dataset_summarize(ctx, directory, lossy_source=False, chunk_points=0, source_flags=None):
    """swz_dataset_summarize: every node file of the written data set in directory streamed as a query streams it, the scalar
    columns summarised per node on the device, and directory/node-summaries.swz written.  lossy_source admits a 3DTILES source
    (intensity is summarised, if the files carry it); chunk_points as in Tiler.write_output.  Returns the stats as a dict (nodes,
    points, bytes_read, chunks, read_ms, unpack_ms, summary_ms, copy_ms, wall_ms)."""
    flags = int(source_flags) if source_flags is not None else (CONVERT_LOSSY_SOURCE if lossy_source else 0)
    stats = _SummarizeStats()
    ctx._check(ctx._lib.swz_dataset_summarize(ctx._ctx, os.fsencode(directory), flags, int(chunk_points), C.byref(stats)))
    return {k: getattr(stats, k) for k, _ in _SummarizeStats._fields_}


def dataset_query_filtered_nodes(directory, box_min, box_max, region=None, filter=None, max_depth=None, lossy_source=False, source_flags=None,
                                 reserved=0):
    """swz_dataset_query_filtered_nodes (host, no GPU): dataset_query_region_nodes' table, unchanged, with read -- a bool per
    node: False for the nodes that directory's node-summaries.swz shows the filter (a Filter; None: no filter) cannot reach --
    and points_bound, the sum of the counts of the nodes that are read.  Without the file or without a filter every node is
    read.  A file that does not describe the data set (another count, a missing node, another format) is refused as stale."""
    box_min, box_max = _region_box(directory, box_min, box_max, region, max_depth)
    p = _query_params(box_min, box_max, max_depth, None, lossy_source, 0, source_flags, reserved)
    rg = None if region is None else region._struct()
    fl = None if filter is None else filter._struct()
    return _query_nodes(load_library().swz_dataset_query_filtered_nodes_why, directory, p, _ref(rg), _ref(fl), with_read=True)


# ---- a written data set rasterized: count, min, max and mean of a value per cell of a grid in x-y (swz_raster_*, swz_dataset_rasterize)
RASTER_VALUE_Z = -1
RASTER_MAX_CELLS = 1 << 26
# a cell (swz_raster_cell) as numpy sees it: 32 bytes
RASTER_CELL_DTYPE = np.dtype([("count", "<u8"), ("sum", "<i8"), ("min_code", "<u8"), ("max_code", "<u8")])


class _RasterGrid(C.Structure):
    _fields_ = [("nx", C.c_uint32), ("ny", C.c_uint32), ("value", C.c_int32), ("reserved", C.c_uint32)]


class _RasterFrame(C.Structure):
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("cw", C.c_double), ("ch", C.c_double), ("v0", C.c_double), ("scale", C.c_double),
                ("nx", C.c_uint32), ("ny", C.c_uint32), ("value", C.c_int32), ("reserved", C.c_uint32)]


class _RasterCell(C.Structure):
    _fields_ = [("count", C.c_uint64), ("sum", C.c_int64), ("min_code", C.c_uint64), ("max_code", C.c_uint64)]


def raster_tile():
    """Rows one workgroup of raster_accumulate_device takes (tests place their edges by it)."""
    return int(load_library().swz_raster_tile())


def _raster_value(value):
    """"z", an attribute's name, or the raw number => swz_raster_grid::value; nothing is checked"""
    if isinstance(value, (int, np.integer)):
        return int(value)
    return RASTER_VALUE_Z if value == "z" else ATTRIBUTES[value][0]


def _raster_frame_struct(frame):
    return _RasterFrame(*[frame[k] for k, _ in _RasterFrame._fields_])


def raster_frame_of(box_min, box_max, nx, ny, value="z", reserved=0):
    """swz_raster_frame_of (host, no GPU): the frame of an nx x ny grid over the x-y rectangle of the closed box, for the value
    "z" or a scalar attribute of one or two bytes (a name of ATTRIBUTES or its index): dict(x0, y0, cw, ch, v0, scale, nx, ny,
    value, reserved).  What the library refuses -- no cell, more than RASTER_MAX_CELLS, a box that is not finite or inverted, a
    flat axis with several cells, gps_time / rgb / normal -- raises SwzError with its text."""
    grid = _RasterGrid(int(nx), int(ny), _raster_value(value), int(reserved))
    frame = _RasterFrame()
    why = C.create_string_buffer(1024)
    st = load_library().swz_raster_frame_of(_vec3(box_min), _vec3(box_max), C.byref(grid), C.byref(frame), why, len(why))
    if st != 0:
        raise SwzError(st, why.value.decode(errors="replace"))
    return {k: getattr(frame, k) for k, _ in _RasterFrame._fields_}


def raster_finish(frame, cells):
    """swz_raster_finish (host, no GPU): a table of frame["nx"] * frame["ny"] cells (RASTER_CELL_DTYPE) decoded into
    dict(count, min, max, mean), arrays of shape (ny, nx), row iy ascending with y.  An empty cell: 0, +inf, -inf, NaN."""
    f = _raster_frame_struct(frame)
    n = int(frame["nx"]) * int(frame["ny"])
    table = np.ascontiguousarray(cells, dtype=RASTER_CELL_DTYPE).reshape(-1)
    if table.shape[0] != n:
        raise ValueError("cells must hold nx * ny cells")
    count = np.empty(n, dtype=np.uint64)
    lo, hi, mean = (np.empty(n, dtype=np.float64) for _ in range(3))
    st = load_library().swz_raster_finish(C.byref(f), table.ctypes.data, count.ctypes.data_as(_u64p), lo.ctypes.data_as(_dp),
                                          hi.ctypes.data_as(_dp), mean.ctypes.data_as(_dp))
    if st != 0:
        raise SwzError(st, "swz_raster_finish: a frame of no cell or of more than RASTER_MAX_CELLS")
    shape = (int(frame["ny"]), int(frame["nx"]))
    return dict(count=count.reshape(shape), min=lo.reshape(shape), max=hi.reshape(shape), mean=mean.reshape(shape))


def _raster_box(directory, box_min, box_max, region, max_depth):
    """the box of a raster: given; or, with both left out, a polygon's x-y bounds and the root box's z, else the root box"""
    if box_min is not None and box_max is not None:
        return box_min, box_max
    if (box_min is None) != (box_max is None):
        raise ValueError("box_min and box_max are given together or left out together")
    if region is not None and region.kind == REGION_POLYGON and region.values is not None:
        return _region_box(directory, None, None, region, max_depth)
    scan = dataset_scan(directory, max_depth)
    if scan["root_source"] == DATASET_ROOT_ABSENT or scan["format"] == "3DTILES":
        raise ValueError("no box to derive: the source has no root box, or stores positions relative to an RTC_CENTER")
    return list(scan["root_min"]), list(scan["root_max"])


def dataset_rasterize(ctx, directory, box_min, box_max, nx, ny, value="z", region=None, filter=None, max_depth=None, lossy_source=False,
                      chunk_points=0):
    """swz_dataset_rasterize: the rows dataset_query_filtered selects -- the closed box, cut by region (a Region) and filter (a
    Filter), of the nodes of depth <= max_depth -- rastered on the device into an nx x ny grid over the box's x-y rectangle:
    per cell the count and the min, max and mean of value ("z", or a scalar attribute of one or two bytes).  No point leaves
    the device; the result is the grid.  box_min and box_max may both be None: the root box of the data set, or for a polygon
    its x-y bounds and the root box's z.  Returns dict(count, min, max, mean, sum -- numpy arrays of shape (ny, nx), row iy
    ascending with y; sum is the integer sum of llrint((v - v0) * scale) --, cells (the raw table, RASTER_CELL_DTYPE), frame
    (raster_frame_of's dict) and stats (the fields of swz_query_stats; points_out is the sum of the counts)).  The table is
    bit-exact: it depends on no order and no chunking.  An empty cell has count 0, min +inf, max -inf, mean NaN."""
    box_min, box_max = _raster_box(directory, box_min, box_max, region, max_depth)
    if filter is not None:
        filter.check()   # (before the directory is scanned)
    grid = _RasterGrid(int(nx), int(ny), _raster_value(value), 0)
    cells = np.zeros(max(int(nx) * int(ny), 1) if int(nx) * int(ny) <= RASTER_MAX_CELLS else 1, dtype=RASTER_CELL_DTYPE)
    p = _query_params(box_min, box_max, max_depth, None, lossy_source, chunk_points)
    rg = None if region is None else region._struct()
    fl = None if filter is None else filter._struct()
    frame, stats = _RasterFrame(), _QueryStats()
    ctx._check(ctx._lib.swz_dataset_rasterize(ctx._ctx, os.fsencode(directory), C.byref(p), _ref(rg), _ref(fl), C.byref(grid), cells.ctypes.data,
                                              C.byref(frame), C.byref(stats)))
    fr = {k: getattr(frame, k) for k, _ in _RasterFrame._fields_}
    out = raster_finish(fr, cells)
    out.update(sum=cells["sum"].reshape(out["count"].shape).copy(), cells=cells, frame=fr,
               stats={k: getattr(stats, k) for k, _ in _QueryStats._fields_})
    return out


LAS_SCAN_SKIP_UNREADABLE = 1


class _LasFileInfo(C.Structure):
    _fields_ = [("point_count", C.c_uint64), ("offset_to_point_data", C.c_uint64), ("layout", _LasLayout),
                ("attribute_mask", C.c_uint32), ("status", C.c_int32)]


class _LasDataset(C.Structure):
    _fields_ = [("total_points", C.c_uint64), ("readable_files", C.c_uint64), ("tight_min", C.c_double * 3),
                ("tight_max", C.c_double * 3), ("cubic_min", C.c_double * 3), ("cubic_max", C.c_double * 3),
                ("origin_min", C.c_double * 3), ("origin_max", C.c_double * 3), ("center", C.c_double * 3),
                ("attribute_mask", C.c_uint32), ("reserved", C.c_uint32)]


class _LasSegment(C.Structure):
    _fields_ = [("first_row", C.c_uint64), ("count", C.c_uint64), ("byte_offset", C.c_uint64), ("layout", _LasLayout)]


class _InputParams(C.Structure):
    _fields_ = [("batch_points", C.c_uint64), ("attribute_mask", C.c_uint32), ("shift_to_center", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class _InputStats(C.Structure):
    _fields_ = [("files", C.c_uint64), ("points", C.c_uint64), ("batches", C.c_uint64), ("bytes_read", C.c_uint64),
                ("read_ms", C.c_double), ("copy_ms", C.c_double), ("decode_ms", C.c_double), ("tile_ms", C.c_double),
                ("wait_ms", C.c_double), ("wall_ms", C.c_double)]


def _path_array(paths):
    enc = [os.fsencode(p) for p in paths]
    return (C.c_char_p * max(len(enc), 1))(*enc), len(enc)


def attribute_names(mask):
    """the names of ATTRIBUTES whose bits are set in mask"""
    return [name for name, (idx, _, _) in ATTRIBUTES.items() if int(mask) >> idx & 1]


SRS_LONGLAT, SRS_TMERC = 0, 1
SRS_ECEF, SRS_WGS84 = 0, 1


class _Srs(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("a", C.c_double), ("f", C.c_double), ("e2", C.c_double),
                ("n", C.c_double), ("lat_0", C.c_double), ("lon_0", C.c_double), ("k_0", C.c_double), ("x_0", C.c_double),
                ("y_0", C.c_double), ("radius", C.c_double), ("xi_0", C.c_double), ("beta", C.c_double * 6),
                ("delta", C.c_double * 6)]


class Srs:
    """swz_srs_parse: a source projection, swz.Srs("+proj=utm +zone=32 +datum=WGS84").  Raises SwzError, naming the token,
    for everything the library does not map itself.  fields(): the struct as a dict."""

    def __init__(self, definition):
        self.definition = str(definition)
        self._s = _Srs()
        why = C.create_string_buffer(512)
        st = load_library().swz_srs_parse_why(self.definition.encode(), C.byref(self._s), why, len(why))
        if st != 0:
            raise SwzError(st, why.value.decode(errors="replace"))

    def fields(self):
        out = {}
        for name, _ in _Srs._fields_:
            v = getattr(self._s, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out

    def _ref(self):
        return C.byref(self._s)


def _as_srs(srs):
    return None if srs is None else (srs if isinstance(srs, Srs) else Srs(srs))


def _check_target(target):
    if target not in (SRS_ECEF, SRS_WGS84):
        raise ValueError("target must be SRS_ECEF or SRS_WGS84")


def srs_transform(srs, xyz, target=SRS_ECEF):
    """swz_srs_transform: positions (n, 3) in the source projection -> a new float64 array in ECEF (metres) or WGS84 (longitude
    and latitude in radians, height), on the host."""
    _check_target(target)
    out = np.array(xyz, dtype=np.float64, order="C").reshape(-1, 3)
    st = load_library().swz_srs_transform(_as_srs(srs)._ref(), int(target), out.ctypes.data_as(_dp), out.shape[0])
    if st != 0:
        raise SwzError(st, "swz_srs_transform failed")
    return out


def srs_transform_box(srs, box_min, box_max, target=SRS_ECEF):
    """swz_srs_transform_box: min / max per axis of the eight mapped corners.  Returns (min, max)."""
    _check_target(target)
    lo, hi = (C.c_double * 3)(), (C.c_double * 3)()
    st = load_library().swz_srs_transform_box(_as_srs(srs)._ref(), int(target), _vec3(box_min), _vec3(box_max), lo, hi)
    if st != 0:
        raise SwzError(st, "swz_srs_transform_box failed")
    return np.array(list(lo)), np.array(list(hi))


def srs_tile():
    """The rows one workgroup of srs_transform_device takes at a time."""
    return int(load_library().swz_srs_tile())


def las_scan_files(paths, skip_unreadable=False, ctx=None, srs=None):
    """swz_las_scan_files: the headers of a data set of uncompressed LAS files (host only).  Returns (files, dataset):
    files is a list of dicts (count, offset_to_point_data, point_format, record_bytes, scale, offset, min, max, attrs,
    status), dataset a dict (total_points, readable_files, tight / cubic / origin boxes as (min, max) of float64 arrays,
    center, attrs: the names common to all readable files, attribute_mask).  srs (a string or an Srs): the boxes of the data
    set are those of the files' boxes in ECEF (swz_las_scan_files_srs); the files' entries keep their headers' values."""
    arr, n = _path_array(paths)
    infos = (_LasFileInfo * max(n, 1))()
    ds = _LasDataset()
    L = load_library()
    flags = LAS_SCAN_SKIP_UNREADABLE if skip_unreadable else 0
    srs = _as_srs(srs)
    if srs is None:
        st = L.swz_las_scan_files(ctx, arr, n, flags, infos, C.byref(ds))
    else:
        st = L.swz_las_scan_files_srs(ctx, arr, n, flags, srs._ref(), infos, C.byref(ds))
    if st != 0:
        raise SwzError(st, L.swz_last_error(ctx).decode() if ctx else "swz_las_scan_files failed")
    files = []
    for i in range(n):
        f, lay = infos[i], infos[i].layout
        files.append(dict(count=int(f.point_count), offset_to_point_data=int(f.offset_to_point_data),
                          point_format=int(lay.point_format), record_bytes=int(lay.record_bytes), scale=list(lay.scale),
                          offset=list(lay.offset), min=list(lay.min), max=list(lay.max),
                          attrs=attribute_names(f.attribute_mask), attribute_mask=int(f.attribute_mask), status=int(f.status)))
    vec = lambda v: np.array(list(v), dtype=np.float64)
    dataset = dict(total_points=int(ds.total_points), readable_files=int(ds.readable_files),
                   tight=(vec(ds.tight_min), vec(ds.tight_max)), cubic=(vec(ds.cubic_min), vec(ds.cubic_max)),
                   origin=(vec(ds.origin_min), vec(ds.origin_max)), center=vec(ds.center),
                   attrs=attribute_names(ds.attribute_mask), attribute_mask=int(ds.attribute_mask))
    return files, dataset


def input_batches(file_counts, batch_points, min_last=0):
    """swz_input_batches: the first point of every batch of the concatenated files, and the total as the last entry."""
    cnt = np.ascontiguousarray(file_counts, dtype=np.uint64).reshape(-1)
    num = C.c_uint64()
    L = load_library()
    st = L.swz_input_batches(cnt.shape[0], cnt.ctypes.data_as(_u64p), int(batch_points), int(min_last), 0, None, C.byref(num))
    if st != 0:
        raise SwzError(st, "swz_input_batches failed")
    first = np.empty(int(num.value) + 1, dtype=np.uint64)
    st = L.swz_input_batches(cnt.shape[0], cnt.ctypes.data_as(_u64p), int(batch_points), int(min_last), int(num.value),
                             first.ctypes.data_as(_u64p), C.byref(num))
    if st != 0:
        raise SwzError(st, "swz_input_batches failed")
    return first


def las_input_tile():
    """The points one workgroup of las_decode_segments_device takes."""
    return int(load_library().swz_las_input_tile())


def tiler_merge_tile():
    """Elements of a run that one workgroup of the multi-batch tiler's merge ranks (tests place their edges by it)."""
    return int(load_library().swz_tiler_merge_tile())


def tiler_merge_lds():
    """The longest bracket of the other run that the merge searches out of LDS."""
    return int(load_library().swz_tiler_merge_lds())


def tiler_gather_lds():
    """The most segments a workgroup's 256 outputs may span for the file gather to search them out of LDS."""
    return int(load_library().swz_tiler_gather_lds())


# swz_tiler_path_counts: the SWZ_TILER_PATH_* indices of include/swz_gpu.h, in order
TILER_PATHS = ("pull_in_place", "pull_gathered", "pull_whole_file", "rekey", "resort", "compact_full", "linearize_moved",
               "append_behind", "table_merge_nf0", "table_merge_heads0")


def library_path():
    return os.environ.get("SWZ_GPU_LIBRARY", os.path.join(_HERE, "lib", "libswz_gpu.so"))


# the all-gather callback of swz_shard_joint_root_begin: int (*)(void* arg, const void* mine, uint64_t bytes, void* all)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)

_lib = None
_dp, _u64p, _u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
_i8p, _u8p = C.POINTER(C.c_int8), C.POINTER(C.c_uint8)


def _preload_hip_runtime():
    """A PyTorch-ROCm wheel ships its own libamdhip64.so and loads it by path, so a process that loads
    libswz_gpu.so first (resolving the system's libamdhip64.so.7) and imports torch later would run two HIP
    runtimes, the second of which finds no devices.  Loading torch's copy first (same SONAME) makes both use one.
    Without torch installed the system runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """Loads libswz_gpu.so; raises OSError when it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise OSError("libswz_gpu.so not found at %s -- build it with `make -C schwarzwald_amd/csrc` "
                      "(there is no CPU fallback)" % path)
    _preload_hip_runtime()
    L = C.CDLL(path)
    vp = C.c_void_p
    L.swz_abi_version.restype = C.c_int
    if L.swz_abi_version() != ABI_VERSION:
        raise OSError("libswz_gpu.so has ABI version %d, this binding is written for %d (include/swz_gpu.h) -- rebuild it "
                      "with `make -C schwarzwald_amd/csrc`" % (L.swz_abi_version(), ABI_VERSION))
    L.swz_create.argtypes = [C.POINTER(vp), C.c_int]
    L.swz_destroy.argtypes = [vp]
    L.swz_last_error.restype = C.c_char_p
    L.swz_last_error.argtypes = [vp]
    L.swz_set_stream.argtypes = [vp, vp]
    L.swz_release_workspace.argtypes = [vp]
    L.swz_workspace_bytes.restype = C.c_uint64
    L.swz_workspace_bytes.argtypes = [vp]
    L.swz_morton_encode.argtypes = [vp, _dp, C.c_uint64, _dp, _dp, _u64p]
    L.swz_morton_encode_device.argtypes = [vp, vp, C.c_uint64, _dp, _dp, vp]
    L.swz_sort_by_key.argtypes = [vp, _u64p, C.c_uint64, _u32p, _u64p]
    L.swz_sort_by_key_device.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.swz_sample_points.argtypes = [vp, C.c_int, C.c_uint64, _u64p, _u32p, C.c_uint64, _dp, C.c_uint64, C.c_uint64,
                                    C.c_int32, _dp, _dp, C.c_float, C.c_int, _u8p, _u64p]
    L.swz_tile.argtypes = [vp, _dp, C.c_uint64, _dp, _dp, C.POINTER(_TileParams), _u64p, _u32p, _i8p, _u32p,
                           C.POINTER(_TileStats)]
    L.swz_tile_device.argtypes = [vp, vp, C.c_uint64, _dp, _dp, C.POINTER(_TileParams), vp, vp, vp, vp,
                                  C.POINTER(_TileStats)]
    L.swz_tile_nodes_begin_device.argtypes = [vp, vp, C.c_uint64, _dp, _dp, C.POINTER(_TileParams), _u64p, _u64p, C.POINTER(_TileStats)]
    L.swz_tile_nodes_end_device.argtypes = [vp, vp, vp, vp, C.c_uint64, _i8p, _u64p, _u64p, _u64p]
    L.swz_build_node_lists.argtypes = [vp, _u64p, _i8p, C.c_uint64, _u32p, C.c_uint64, _i8p, _u64p, _u64p, _u64p,
                                       _u64p]
    L.swz_generate_uniform_device.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
    L.swz_build_node_lists_device.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, _i8p, _u64p, _u64p, _u64p, _u64p]
    L.swz_attribute_row_bytes.restype = C.c_uint32
    L.swz_attribute_row_bytes.argtypes = [C.c_int]
    cols = C.POINTER(_AttributeColumns)
    L.swz_gather_payload_device.argtypes = [vp, vp, vp, C.c_uint64, vp, cols, vp, cols]
    L.swz_bin_write_node.argtypes = [vp, C.c_char_p, C.c_uint64, _dp, cols, C.c_int]
    L.swz_bin_read_header.argtypes = [vp, C.c_char_p, C.c_int, _u32p, _u64p]
    L.swz_bin_read_node.argtypes = [vp, C.c_char_p, C.c_int, _dp, cols]
    L.swz_bin_persist_nodes.argtypes = [vp, C.c_char_p, C.c_uint64, _i8p, _u64p, _u64p, _u64p, _dp, cols, C.c_int]
    L.swz_bin_layout.argtypes = [C.c_uint64, _u64p, C.c_uint32, _u64p, _u64p, _u64p, _u64p]
    L.swz_bin_pack_tile.argtypes = []
    L.swz_bin_pack_tile.restype = C.c_uint32
    L.swz_bin_pack_device.argtypes = [vp, vp, vp, C.c_uint64, vp, cols, C.c_uint64, _u64p, _u64p, C.c_uint32, vp, C.c_uint64]
    L.swz_bin_persist_nodes_image.argtypes = [vp, C.c_char_p, C.c_uint64, _i8p, _u64p, _u64p, vp, C.c_uint64, C.c_uint32, C.c_int]
    L.swz_properties_json_write.argtypes = [vp, C.c_char_p, _dp, _dp, C.c_float, C.c_uint64]
    L.swz_properties_json_read.argtypes = [vp, C.c_char_p, _dp, _dp, C.POINTER(C.c_float), _u64p]
    L.swz_tiler_write_properties.argtypes = [vp, C.c_char_p]
    L.swz_dataset_scan.argtypes = [vp, C.c_char_p, C.c_int32, C.POINTER(_DatasetInfo), C.c_uint64, _i8p, _u64p, _u64p, _u64p]
    L.swz_dataset_scan_why.argtypes = [C.c_char_p, C.c_int32, C.POINTER(_DatasetInfo), C.c_uint64, _i8p, _u64p, _u64p, _u64p, C.c_char_p,
                                       C.c_uint64]
    L.swz_bin_unpack_tile.argtypes = []
    L.swz_bin_unpack_tile.restype = C.c_uint32
    L.swz_bin_unpack_segments_device.argtypes = [vp, vp, C.c_uint64, C.POINTER(_BinSegment), C.c_uint64, vp, cols]
    L.swz_pnts_unpack_tile.argtypes = []
    L.swz_pnts_unpack_tile.restype = C.c_uint32
    L.swz_pnts_unpack_segments_device.argtypes = [vp, vp, C.c_uint64, C.POINTER(_PntsSegment), C.c_uint64, vp, cols]
    L.swz_pnts_unpack_segments_device.restype = C.c_int
    L.swz_pnts_parse_image.argtypes = [vp, vp, C.c_uint64, _u64p, _u32p, _dp, _u64p, _u64p, _u64p]
    L.swz_pnts_parse_image.restype = C.c_int
    L.swz_convert_dataset.argtypes = [vp, C.c_char_p, C.c_char_p, C.POINTER(_ConvertParams), C.POINTER(_ConvertStats)]
    L.swz_box_select_tile.argtypes = []
    L.swz_box_select_tile.restype = C.c_uint32
    L.swz_box_select_device.argtypes = [vp, vp, C.c_uint64, cols, C.c_uint32, _dp, _dp, C.c_uint64, vp, cols, vp, _u64p]
    L.swz_dataset_query_nodes.argtypes = [vp, C.c_char_p, C.POINTER(_QueryParams), C.c_uint64, _i8p, _u64p, _u64p, _u64p, _u64p]
    L.swz_dataset_query_nodes_why.argtypes = [C.c_char_p, C.POINTER(_QueryParams), C.c_uint64, _i8p, _u64p, _u64p, _u64p, _u64p, C.c_char_p,
                                              C.c_uint64]
    L.swz_dataset_query.argtypes = [vp, C.c_char_p, C.POINTER(_QueryParams), C.c_uint64, vp, cols, vp, _u64p, C.POINTER(_QueryStats)]
    rgp = C.POINTER(_Region)
    L.swz_region_select_device.argtypes = [vp, vp, C.c_uint64, cols, C.c_uint32, _dp, _dp, rgp, C.c_uint64, vp, cols, vp, _u64p]
    L.swz_dataset_query_region_nodes.argtypes = [vp, C.c_char_p, C.POINTER(_QueryParams), rgp, C.c_uint64, _i8p, _u64p, _u64p, _u64p, _u64p]
    L.swz_dataset_query_region_nodes_why.argtypes = [C.c_char_p, C.POINTER(_QueryParams), rgp, C.c_uint64, _i8p, _u64p, _u64p, _u64p, _u64p,
                                                     C.c_char_p, C.c_uint64]
    L.swz_dataset_query_region.argtypes = [vp, C.c_char_p, C.POINTER(_QueryParams), rgp, C.c_uint64, vp, cols, vp, _u64p, C.POINTER(_QueryStats)]
    flp = C.POINTER(_Filter)
    L.swz_filter_check.argtypes = [flp, C.c_char_p, C.c_uint64]
    L.swz_filter_select_device.argtypes = [vp, vp, C.c_uint64, cols, C.c_uint32, _dp, _dp, rgp, flp, C.c_uint64, vp, cols, vp, _u64p]
    L.swz_dataset_query_filtered.argtypes = [vp, C.c_char_p, C.POINTER(_QueryParams), rgp, flp, C.c_uint64, vp, cols, vp, _u64p,
                                             C.POINTER(_QueryStats)]
    for name in ("swz_filter_check", "swz_filter_select_device", "swz_dataset_query_filtered"):
        getattr(L, name).restype = C.c_int
    L.swz_node_summaries_tile.argtypes = []
    L.swz_node_summaries_tile.restype = C.c_uint32
    L.swz_node_summaries_device.argtypes = [vp, C.c_uint64, cols, C.c_uint32, C.c_uint64, _u64p, _u64p, vp]
    L.swz_dataset_summaries_write.argtypes = [C.c_char_p, C.c_int32, C.c_uint32, C.c_uint64, _i8p, _u64p, _u64p, vp, C.c_char_p, C.c_uint64]
    L.swz_dataset_summaries_read.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _u32p, _u64p, _u64p, C.c_uint64, _i8p, _u64p,
                                             _u64p, vp, C.c_char_p, C.c_uint64]
    L.swz_dataset_summarize.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_uint64, C.POINTER(_SummarizeStats)]
    L.swz_dataset_query_filtered_nodes.argtypes = [vp, C.c_char_p, C.POINTER(_QueryParams), rgp, flp, C.c_uint64, _i8p, _u64p, _u64p, vp, _u64p,
                                                   _u64p]
    L.swz_dataset_query_filtered_nodes_why.argtypes = [C.c_char_p, C.POINTER(_QueryParams), rgp, flp, C.c_uint64, _i8p, _u64p, _u64p, vp, _u64p,
                                                       _u64p, C.c_char_p, C.c_uint64]
    for name in ("swz_node_summaries_device", "swz_dataset_summaries_write", "swz_dataset_summaries_read", "swz_dataset_summarize",
                 "swz_dataset_query_filtered_nodes", "swz_dataset_query_filtered_nodes_why"):
        getattr(L, name).restype = C.c_int
    rfp = C.POINTER(_RasterFrame)
    L.swz_raster_tile.argtypes = []
    L.swz_raster_tile.restype = C.c_uint32
    L.swz_raster_frame_of.argtypes = [_dp, _dp, C.POINTER(_RasterGrid), rfp, C.c_char_p, C.c_uint64]
    L.swz_raster_finish.argtypes = [rfp, vp, _u64p, _dp, _dp, _dp]
    L.swz_raster_clear_device.argtypes = [vp, rfp, vp]
    L.swz_raster_accumulate_device.argtypes = [vp, vp, C.c_uint64, vp, _dp, _dp, rfp, vp]
    L.swz_dataset_rasterize.argtypes = [vp, C.c_char_p, C.POINTER(_QueryParams), rgp, flp, C.POINTER(_RasterGrid), vp, rfp, C.POINTER(_QueryStats)]
    for name in ("swz_raster_frame_of", "swz_raster_finish", "swz_raster_clear_device", "swz_raster_accumulate_device", "swz_dataset_rasterize"):
        getattr(L, name).restype = C.c_int
    for name in ("swz_region_select_device", "swz_dataset_query_region_nodes", "swz_dataset_query_region_nodes_why", "swz_dataset_query_region"):
        getattr(L, name).restype = C.c_int
    for name in ("swz_box_select_device", "swz_dataset_query_nodes", "swz_dataset_query_nodes_why", "swz_dataset_query"):
        getattr(L, name).restype = C.c_int
    L.swz_tiler_write_output.argtypes = [vp, C.c_char_p, C.POINTER(_OutputParams), C.POINTER(_OutputStats)]
    L.swz_output_chunks.argtypes = [C.c_uint64, _u64p, C.c_uint64, C.c_uint64, _u64p, _u64p]
    L.swz_merge_shard_node_tables.argtypes = [C.c_int, _u64p, C.POINTER(_i8p), C.POINTER(_u64p), C.POINTER(_u64p), C.c_uint64, _i8p,
                                              _u64p, _u64p, C.POINTER(C.c_int32), _u64p]
    for name in ("swz_bin_layout", "swz_bin_pack_device", "swz_bin_persist_nodes_image", "swz_tiler_write_output",
                 "swz_output_chunks", "swz_merge_shard_node_tables"):
        getattr(L, name).restype = C.c_int
    L.swz_node_name.argtypes = [C.c_int8, C.c_uint64, C.c_char_p]
    L.swz_node_name_entwine.argtypes = [C.c_int8, C.c_uint64, C.c_char_p]
    L.swz_node_from_entwine_name.argtypes = [C.c_char_p, _i8p, _u64p]
    L.swz_node_bounds.argtypes = [C.c_int8, C.c_uint64, _dp, _dp, _dp, _dp]
    L.swz_node_geometric_error.argtypes = [C.c_int8, C.c_float]
    L.swz_node_geometric_error.restype = C.c_double
    L.swz_tileset_build.argtypes = [C.c_uint64, _i8p, _u64p, _dp, _dp, C.c_float, _dp, C.c_uint64,
                                    C.POINTER(_TilesetNode), _u64p]
    L.swz_tileset_build.restype = C.c_int
    L.swz_tileset_build_boxes.argtypes = [C.c_uint64, _i8p, _u64p, _dp, _dp, _dp, _dp, C.c_float, _dp, C.c_uint64,
                                          C.POINTER(_TilesetNode), _u64p]
    L.swz_tileset_build_boxes.restype = C.c_int
    L.swz_node_boxes_tile.argtypes = []
    L.swz_node_boxes_tile.restype = C.c_uint32
    L.swz_node_boxes_device.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, _u64p, _u64p, _dp, _dp]
    L.swz_node_boxes_device.restype = C.c_int
    L.swz_tiler_node_boxes.argtypes = [vp, C.c_uint64, _dp, _dp, _u64p]
    L.swz_tiler_node_boxes.restype = C.c_int
    L.swz_las_stored_box.argtypes = [_dp, _dp, _dp, C.c_double, _dp, _dp]
    L.swz_las_stored_box.restype = C.c_int
    L.swz_output_flags_check.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_char_p)]
    L.swz_output_flags_check.restype = C.c_int
    L.swz_pnts_layout.argtypes = [C.c_uint64, _u64p, C.c_uint32, C.c_int, _u64p, _u64p, _u64p, _u64p, _u64p]
    L.swz_pnts_pack_device.argtypes = [vp, vp, vp, C.c_uint64, vp, cols, C.c_uint64, _u64p, _u64p, C.c_uint32, C.c_int, vp,
                                       C.c_uint64]
    L.swz_pnts_write_node.argtypes = [vp, C.c_char_p, C.c_uint64, vp, C.c_uint64, C.c_uint32, _dp]
    L.swz_pnts_write_node_rows.argtypes = [vp, C.c_char_p, C.c_uint64, _dp, cols, C.c_uint32, C.c_int, _dp]
    L.swz_pnts_persist_nodes.argtypes = [vp, C.c_char_p, C.c_uint64, _i8p, _u64p, _u64p, vp, C.c_uint64, C.c_uint32, _dp]
    L.swz_pnts_read_header.argtypes = [vp, C.c_char_p, _u64p, _u32p, _dp]
    L.swz_pnts_read_node.argtypes = [vp, C.c_char_p, _dp, cols]
    L.swz_pnts_rgb_from_intensity.argtypes = [C.c_int, C.c_uint16]
    L.swz_pnts_rgb_from_intensity.restype = C.c_uint8
    L.swz_tileset_write.argtypes = [vp, C.POINTER(_TilesetNode), C.c_uint64, C.c_char_p]
    L.swz_pnts_pack_origin_device.argtypes = L.swz_pnts_pack_device.argtypes + [_dp]
    L.swz_pnts_persist_nodes_rtc.argtypes = [vp, C.c_char_p, C.c_uint64, _i8p, _u64p, _u64p, vp, C.c_uint64, C.c_uint32, _dp]
    L.swz_tileset_oriented_boxes.argtypes = [C.POINTER(_Srs), C.POINTER(_TilesetNode), C.c_uint64, _dp]
    L.swz_tileset_write_oriented.argtypes = [vp, C.POINTER(_TilesetNode), C.c_uint64, _dp, C.c_char_p]
    L.swz_srs_project_node_boxes_device.argtypes = [vp, C.POINTER(_Srs), vp, C.c_uint64, C.c_uint64, _u64p, _u64p, _dp, _dp]
    L.swz_convert_dataset_world.argtypes = [vp, C.c_char_p, C.c_char_p, C.POINTER(_ConvertParams), C.POINTER(_Srs), C.POINTER(_ConvertStats)]
    for name in ("swz_pnts_pack_origin_device", "swz_pnts_persist_nodes_rtc", "swz_tileset_oriented_boxes", "swz_tileset_write_oriented",
                 "swz_srs_project_node_boxes_device", "swz_convert_dataset_world"):
        getattr(L, name).restype = C.c_int
    for name in ("swz_pnts_layout", "swz_pnts_pack_device", "swz_pnts_write_node", "swz_pnts_write_node_rows",
                 "swz_pnts_persist_nodes", "swz_pnts_read_header", "swz_pnts_read_node", "swz_tileset_write"):
        getattr(L, name).restype = C.c_int
    L.swz_las_decode_device.argtypes = [vp, vp, C.c_uint64, C.POINTER(_LasLayout), vp, cols]
    L.swz_las_scan_files.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint32, C.POINTER(_LasFileInfo), C.POINTER(_LasDataset)]
    L.swz_input_batches.argtypes = [C.c_uint64, _u64p, C.c_uint64, C.c_uint64, C.c_uint64, _u64p, _u64p]
    L.swz_las_input_tile.argtypes = []
    L.swz_las_input_tile.restype = C.c_uint32
    L.swz_las_decode_segments_device.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(_LasSegment), _dp, vp, cols]
    L.swz_tiler_add_las_files.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(_InputParams), C.POINTER(_InputStats)]
    srsp = C.POINTER(_Srs)
    L.swz_srs_parse.argtypes = [vp, C.c_char_p, srsp]
    L.swz_srs_parse_why.argtypes = [C.c_char_p, srsp, C.c_char_p, C.c_uint64]
    L.swz_srs_transform.argtypes = [srsp, C.c_int, _dp, C.c_uint64]
    L.swz_srs_transform_device.argtypes = [vp, srsp, C.c_int, vp, C.c_uint64]
    L.swz_srs_transform_box.argtypes = [srsp, C.c_int, _dp, _dp, _dp, _dp]
    L.swz_srs_tile.argtypes = []
    L.swz_srs_tile.restype = C.c_uint32
    L.swz_las_scan_files_srs.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint32, srsp, C.POINTER(_LasFileInfo), C.POINTER(_LasDataset)]
    L.swz_las_decode_segments_srs_device.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(_LasSegment), _dp, vp, cols, srsp]
    L.swz_tiler_set_source_srs.argtypes = [vp, srsp]
    for name in ("swz_srs_parse", "swz_srs_parse_why", "swz_srs_transform", "swz_srs_transform_device", "swz_srs_transform_box",
                 "swz_las_scan_files_srs", "swz_las_decode_segments_srs_device", "swz_tiler_set_source_srs"):
        getattr(L, name).restype = C.c_int
    for name in ("swz_las_scan_files", "swz_input_batches", "swz_las_decode_segments_device", "swz_tiler_add_las_files"):
        getattr(L, name).restype = C.c_int
    L.swz_las_scale_from_bounds.argtypes = [_dp, _dp]
    L.swz_las_scale_from_bounds.restype = C.c_double
    L.swz_las_record_layout.argtypes = [C.c_uint32, _u32p, _u32p]
    L.swz_las_image_layout.argtypes = [C.c_uint64, _u64p, C.c_uint32, _u64p, _u64p, _u64p]
    L.swz_las_pack_tile.argtypes = []
    L.swz_las_pack_tile.restype = C.c_uint32
    L.swz_las_pack_device.argtypes = [vp, vp, vp, C.c_uint64, vp, cols, C.c_uint64, _u64p, _u64p, _dp, _dp, C.c_uint32, vp, C.c_uint64]
    L.swz_las_write_node.argtypes = [vp, C.c_char_p, C.c_uint64, vp, C.c_uint32, _dp, _dp, C.c_double]
    L.swz_las_write_node_rows.argtypes = [vp, C.c_char_p, C.c_uint64, _dp, cols, C.c_uint32, _dp, _dp, C.c_double]
    L.swz_las_persist_nodes.argtypes = [vp, C.c_char_p, C.c_uint64, _i8p, _u64p, _u64p, _dp, _dp, _dp, vp, C.c_uint64, C.c_uint32,
                                        C.c_int]
    L.swz_las_read_header.argtypes = [vp, C.c_char_p, _u64p, _u32p, _u32p, _u32p, C.POINTER(_LasLayout)]
    L.swz_las_read_node.argtypes = [vp, C.c_char_p, _dp, cols]
    L.swz_ept_create_dirs.argtypes = [vp, C.c_char_p]
    L.swz_ept_hierarchy_write.argtypes = [vp, C.c_char_p, C.c_uint64, _i8p, _u64p, _u64p]
    L.swz_ept_json_write.argtypes = [vp, C.c_char_p, C.POINTER(_EptJson)]
    for name in ("swz_las_record_layout", "swz_las_image_layout", "swz_las_pack_device", "swz_las_write_node", "swz_las_write_node_rows",
                 "swz_las_persist_nodes", "swz_las_read_header", "swz_las_read_node", "swz_ept_create_dirs", "swz_ept_hierarchy_write",
                 "swz_ept_json_write"):
        getattr(L, name).restype = C.c_int
    L.swz_partition_by_octant_device.argtypes = [vp, vp, C.c_uint64, vp, _u64p]
    L.swz_shard_begin_device.argtypes = [vp, vp, C.c_uint64, _dp, _dp, C.POINTER(_TileParams), C.POINTER(_ShardInfo),
                                         _u64p]
    L.swz_shard_presort_device.argtypes = [vp, vp, C.c_uint64, _dp, _dp, C.POINTER(_TileParams), C.c_uint64]
    L.swz_shard_root_taken_device.argtypes = [vp, vp]
    L.swz_shard_finish_device.argtypes = [vp, vp, vp, vp, C.POINTER(_TileStats)]
    L.swz_shard_fast_begin_device.argtypes = [vp, vp, C.c_uint64, _dp, _dp, C.POINTER(_TileParams), _u32p]
    L.swz_shard_fast_run.argtypes = [vp, C.c_int32, _u64p]
    L.swz_shard_fast_root_candidates_device.argtypes = [vp, vp, vp]
    L.swz_shard_fast_set_root_device.argtypes = [vp, vp]
    L.swz_shard_fast_finish_device.argtypes = [vp, vp, vp, vp, vp, C.POINTER(_TileStats)]
    L.swz_sample_points_device.argtypes = [vp, C.c_int, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_int32, _dp, _dp,
                                           C.c_float, C.c_int, vp, _u64p]
    L.swz_tiler_create.argtypes = [vp, _dp, _dp, C.POINTER(_TileParams), C.c_uint64, C.POINTER(vp)]
    L.swz_tiler_destroy.argtypes = [vp]
    L.swz_tiler_add_batch_device.argtypes = [vp, vp, C.c_uint64, C.POINTER(_TileStats)]
    L.swz_tiler_stage_batch.argtypes = [vp, vp, C.c_uint64, cols]
    L.swz_tiler_tile_staged.argtypes = [vp, C.POINTER(_TileStats)]
    L.swz_tiler_add_batch.argtypes = [vp, vp, C.c_uint64, cols, C.POINTER(_TileStats)]
    L.swz_tiler_finalize.argtypes = [vp, C.POINTER(_TileStats)]
    L.swz_tiler_get_info.argtypes = [vp, C.POINTER(_TilerInfo)]
    L.swz_tiler_export_device.argtypes = [vp, vp, vp, vp]
    L.swz_tiler_node_table.argtypes = [vp, C.c_uint64, _i8p, _u64p, _u64p, _u64p, _u64p]
    L.swz_tiler_pools_device.argtypes = [vp, C.POINTER(vp), cols]
    L.swz_tiler_shard_begin_device.argtypes = [vp, vp, C.c_uint64, cols, C.POINTER(_TilerShardInfo), _u64p]
    L.swz_tiler_shard_finish.argtypes = [vp, C.POINTER(_TileStats)]
    L.swz_tiler_level_count.argtypes = [vp, C.c_int, _u64p]
    L.swz_tiler_poison.argtypes = [vp, C.c_char_p]
    L.swz_tiler_pool_residency.argtypes = [vp, _u64p, _u64p]
    L.swz_tiler_store_residency.argtypes = [vp, _u64p, _u64p]
    L.swz_tiler_path_counts.argtypes = [vp, _u64p, C.c_uint32]
    L.swz_tiler_path_counts.restype = C.c_int
    for name in ("swz_tiler_merge_tile", "swz_tiler_merge_lds", "swz_tiler_gather_lds"):
        getattr(L, name).argtypes = []
        getattr(L, name).restype = C.c_uint32
    L.swz_shard_joint_root_possible.argtypes = [vp, C.POINTER(_TileParams), _dp, _dp]
    L.swz_shard_joint_root_begin.argtypes = [vp, C.c_int, C.c_int, EXCHANGE_FN, vp]
    L.swz_shard_joint_root_probe.argtypes = [vp, C.c_int, C.c_int, EXCHANGE_FN, vp, C.POINTER(C.c_int)]
    L.swz_shard_joint_root_meet.argtypes = [vp, C.c_int]
    L.swz_shard_joint_root_end.argtypes = [vp]
    L.swz_tiler_shard_fast_histogram.argtypes = [vp, _u32p]
    L.swz_fast_start_level_from_counts.argtypes = [_u64p, C.c_uint32, C.POINTER(C.c_int32)]
    L.swz_tiler_shard_set_start_level.argtypes = [vp, C.c_int32]
    L.swz_tiler_shard_fast_finalize_local.argtypes = [vp, C.POINTER(_TileStats)]
    L.swz_tiler_shard_fast_set_root.argtypes = [vp, vp]
    L.swz_tiler_level_positions_device.argtypes = [vp, C.c_int, vp]
    L.swz_host_alloc_pinned.argtypes = [C.c_uint64, C.POINTER(vp)]
    L.swz_host_free_pinned.argtypes = [vp]
    L.swz_profile_enable.argtypes = [vp, C.c_int]
    L.swz_profile_reset.argtypes = [vp]
    L.swz_profile_get.argtypes = [vp, C.POINTER(_KernelStat), C.c_uint32, _u32p]
    for name in ("swz_create", "swz_destroy", "swz_set_stream", "swz_release_workspace", "swz_morton_encode",
                 "swz_morton_encode_device", "swz_sort_by_key", "swz_sort_by_key_device", "swz_sample_points",
                 "swz_tile", "swz_tile_device", "swz_tile_nodes_begin_device", "swz_tile_nodes_end_device", "swz_build_node_lists", "swz_generate_uniform_device",
                 "swz_profile_enable", "swz_profile_reset", "swz_profile_get", "swz_partition_by_octant_device",
                 "swz_shard_begin_device", "swz_shard_root_taken_device", "swz_shard_finish_device",
                 "swz_build_node_lists_device", "swz_gather_payload_device", "swz_bin_write_node",
                 "swz_bin_read_header", "swz_bin_read_node", "swz_bin_persist_nodes", "swz_node_name",
                 "swz_las_decode_device", "swz_shard_presort_device", "swz_node_name_entwine",
                 "swz_node_from_entwine_name", "swz_node_bounds", "swz_tiler_create", "swz_tiler_destroy",
                 "swz_tiler_add_batch_device", "swz_tiler_stage_batch", "swz_tiler_tile_staged", "swz_tiler_add_batch",
                 "swz_tiler_finalize", "swz_tiler_get_info", "swz_tiler_export_device", "swz_tiler_node_table",
                 "swz_tiler_pools_device", "swz_host_alloc_pinned", "swz_host_free_pinned",
                 "swz_tiler_shard_begin_device", "swz_tiler_shard_finish", "swz_tiler_level_count",
                 "swz_tiler_level_positions_device", "swz_tiler_poison", "swz_tiler_pool_residency", "swz_tiler_store_residency",
                 "swz_tiler_shard_fast_histogram", "swz_fast_start_level_from_counts", "swz_tiler_shard_set_start_level",
                 "swz_tiler_shard_fast_finalize_local", "swz_tiler_shard_fast_set_root", "swz_shard_joint_root_possible",
                 "swz_shard_joint_root_begin", "swz_shard_joint_root_probe", "swz_shard_joint_root_meet", "swz_shard_joint_root_end",
                 "swz_shard_fast_begin_device", "swz_shard_fast_run", "swz_shard_fast_root_candidates_device",
                 "swz_shard_fast_set_root_device", "swz_shard_fast_finish_device", "swz_sample_points_device"):
        getattr(L, name).restype = C.c_int
    _lib = L
    return L


def _vec3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _stats_dict(s):
    return dict(num_nodes=int(s.num_nodes), points_visited=int(s.points_visited), max_level=int(s.max_level),
                fast_start_levels=int(s.fast_start_levels), num_levels=int(s.num_levels),
                min_distance_rounds=int(s.min_distance_rounds))


class Context:
    """One swz_ctx (one GPU).  Not thread-safe: serialise calls per context."""

    def __init__(self, device=0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        self.device = int(device)
        st = self._lib.swz_create(C.byref(self._ctx), int(device))
        if st != 0:
            raise SwzError(st, self._lib.swz_last_error(None).decode())

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.swz_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st):
        if st != 0:
            raise SwzError(st, self._lib.swz_last_error(self._ctx).decode())

    # ------------------------------------------------------------------ plumbing
    def set_stream(self, hip_stream):
        """Run on an existing HIP stream (an integer handle such as torch.cuda.current_stream().cuda_stream; 0 is the
        device's default stream, which is PyTorch's default).  None restores the context's own non-blocking stream."""
        handle = C.c_void_p(-1) if hip_stream is None else C.c_void_p(int(hip_stream))
        self._check(self._lib.swz_set_stream(self._ctx, handle))

    def set_option(self, name, value):
        """Debug / tuning switch of this context (what the SWZ_* environment variables seed at creation); None removes it."""
        self._lib.swz_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        self._check(self._lib.swz_set_option(self._ctx, name.encode(), None if value is None else str(value).encode()))

    def copy_to_host(self, d_ptr, nbytes):
        """nbytes of device memory as a numpy uint8 array (swz_copy_to_host: for pointers the library hands out)"""
        out = np.empty(int(nbytes), dtype=np.uint8)
        self._lib.swz_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        self._check(self._lib.swz_copy_to_host(self._ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(int(d_ptr)), int(nbytes)))
        return out

    def release_workspace(self):
        self._check(self._lib.swz_release_workspace(self._ctx))

    def workspace_bytes(self):
        return int(self._lib.swz_workspace_bytes(self._ctx))

    def profile_enable(self, on=True):
        self._check(self._lib.swz_profile_enable(self._ctx, 1 if on else 0))

    def profile_reset(self):
        self._check(self._lib.swz_profile_reset(self._ctx))

    def profile_get(self):
        """{class: launches, total_ms, algorithmic_bytes}.  mq_tables_ahead, mq_prebuild_taken, mq_prebuild_dropped,
        mq_tables_late and mq_tables_at_setup are counts only (swz_profile_get in include/swz_gpu.h): their times are 0."""
        buf = (_KernelStat * 64)()
        num = C.c_uint32()
        self._check(self._lib.swz_profile_get(self._ctx, buf, 64, C.byref(num)))
        return {buf[i].name.decode(): dict(launches=int(buf[i].launches), total_ms=float(buf[i].total_ms),
                                           algorithmic_bytes=int(buf[i].algorithmic_bytes))
                for i in range(min(num.value, 64))}

    # ------------------------------------------------------------------ host-buffer entry points
    def morton_encode(self, xyz, bmin, bmax):
        """index_points<21>(ClampToBounds).  Returns (keys, clamped_xyz); the input is not modified."""
        x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3).copy()
        keys = np.empty(x.shape[0], dtype=np.uint64)
        self._check(self._lib.swz_morton_encode(self._ctx, x.ctypes.data_as(_dp), x.shape[0], _vec3(bmin),
                                                _vec3(bmax), keys.ctypes.data_as(_u64p)))
        return keys, x

    def sort_by_key(self, keys):
        """Returns (perm, sorted_keys): perm orders the input by (key, original index)."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        perm = np.empty(k.shape[0], dtype=np.uint32)
        ks = np.empty(k.shape[0], dtype=np.uint64)
        self._check(self._lib.swz_sort_by_key(self._ctx, k.ctypes.data_as(_u64p), k.shape[0],
                                              perm.ctypes.data_as(_u32p), ks.ctypes.data_as(_u64p)))
        return perm, ks

    def sample_points(self, sampler, max_points_per_node, keys, idx, xyz, node_key, node_level, root_min, root_max,
                      spacing_at_root, behaviour=TAKE_ALL_WHEN_COUNT_BELOW_MAX_POINTS):
        """sample_points(...) of Sampling.h:799-821 on a Morton-sorted range.  Returns the taken flags."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        taken = np.zeros(k.shape[0], dtype=np.uint8)
        num = C.c_uint64()
        self._check(self._lib.swz_sample_points(self._ctx, sampler, max_points_per_node, k.ctypes.data_as(_u64p),
                                                i.ctypes.data_as(_u32p), k.shape[0], x.ctypes.data_as(_dp),
                                                x.shape[0], int(node_key), int(node_level), _vec3(root_min),
                                                _vec3(root_max), C.c_float(spacing_at_root), behaviour,
                                                taken.ctypes.data_as(_u8p), C.byref(num)))
        assert int(num.value) == int(taken.sum())
        return taken

    def tile(self, xyz, bmin, bmax, params):
        x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3).copy()
        n = x.shape[0]
        keys = np.empty(n, dtype=np.uint64)
        perm = np.empty(n, dtype=np.uint32)
        level = np.empty(n, dtype=np.int8)
        dup = np.zeros(n, dtype=np.uint32)
        stats = _TileStats()
        p = params._c()
        self._check(self._lib.swz_tile(self._ctx, x.ctypes.data_as(_dp), n, _vec3(bmin), _vec3(bmax), C.byref(p),
                                       keys.ctypes.data_as(_u64p), perm.ctypes.data_as(_u32p),
                                       level.ctypes.data_as(_i8p), dup.ctypes.data_as(_u32p), C.byref(stats)))
        return TileResult(keys, perm, level, dup, _stats_dict(stats), x)

    def build_node_lists(self, keys_sorted, level):
        k = np.ascontiguousarray(keys_sorted, dtype=np.uint64)
        lv = np.ascontiguousarray(level, dtype=np.int8)
        n = k.shape[0]
        order = np.empty(n, dtype=np.uint32)
        cap = max(n, 1)
        nl = np.empty(cap, dtype=np.int8)
        nk = np.empty(cap, dtype=np.uint64)
        no = np.empty(cap, dtype=np.uint64)
        nc = np.empty(cap, dtype=np.uint64)
        num = C.c_uint64()
        self._check(self._lib.swz_build_node_lists(self._ctx, k.ctypes.data_as(_u64p), lv.ctypes.data_as(_i8p), n,
                                                   order.ctypes.data_as(_u32p), cap, nl.ctypes.data_as(_i8p),
                                                   nk.ctypes.data_as(_u64p), no.ctypes.data_as(_u64p),
                                                   nc.ctypes.data_as(_u64p), C.byref(num)))
        m = int(num.value)
        return order, dict(level=nl[:m].copy(), key=nk[:m].copy(), offset=no[:m].copy(), count=nc[:m].copy())

    # ------------------------------------------------------------------ device-resident entry points
    def generate_uniform_device(self, seed, first_point, n, d_xyz):
        self._check(self._lib.swz_generate_uniform_device(self._ctx, int(seed), int(first_point), int(n),
                                                          C.c_void_p(d_xyz)))

    def morton_encode_device(self, d_xyz, n, bmin, bmax, d_keys):
        self._check(self._lib.swz_morton_encode_device(self._ctx, C.c_void_p(d_xyz), int(n), _vec3(bmin),
                                                       _vec3(bmax), C.c_void_p(d_keys)))

    def sort_by_key_device(self, d_keys, n, d_perm, d_keys_sorted=None):
        self._check(self._lib.swz_sort_by_key_device(self._ctx, C.c_void_p(d_keys), int(n), C.c_void_p(d_perm),
                                                     C.c_void_p(d_keys_sorted)))

    def tile_nodes_device(self, d_xyz, n, bmin, bmax, params, alloc):
        """One batch as node files (swz_tile_nodes_begin_device / _end_device): works where tile() fails with
        ERR_REROOT_UNSUPPORTED.  alloc(num_stored) returns the device pointers (d_keys, d_ids, d_level) for the files'
        contents (any may be None).  Returns (stats, node table: level / key / offset / count arrays, num_stored)."""
        p = params._c()
        stats = _TileStats()
        ns, nn = C.c_uint64(), C.c_uint64()
        self._check(self._lib.swz_tile_nodes_begin_device(self._ctx, C.c_void_p(d_xyz), int(n), _vec3(bmin), _vec3(bmax), C.byref(p),
                                                          C.byref(ns), C.byref(nn), C.byref(stats)))
        try:
            d_keys, d_ids, d_level = alloc(int(ns.value))
        except BaseException:
            self._lib.swz_tile_nodes_end_device(self._ctx, None, None, None, 0, None, None, None, None)
            raise
        cap = max(int(nn.value), 1)
        nl = np.empty(cap, dtype=np.int8)
        nk = np.empty(cap, dtype=np.uint64)
        no = np.empty(cap, dtype=np.uint64)
        nc = np.empty(cap, dtype=np.uint64)
        self._check(self._lib.swz_tile_nodes_end_device(self._ctx, C.c_void_p(d_keys), C.c_void_p(d_ids), C.c_void_p(d_level), cap,
                                                        nl.ctypes.data_as(_i8p), nk.ctypes.data_as(_u64p), no.ctypes.data_as(_u64p),
                                                        nc.ctypes.data_as(_u64p)))
        m = int(nn.value)
        return _stats_dict(stats), dict(level=nl[:m].copy(), key=nk[:m].copy(), offset=no[:m].copy(), count=nc[:m].copy()), int(ns.value)

    def tile_device(self, d_xyz, n, bmin, bmax, params, d_keys, d_perm, d_level, d_dup=None):
        stats = _TileStats()
        p = params._c()
        self._check(self._lib.swz_tile_device(self._ctx, C.c_void_p(d_xyz), int(n), _vec3(bmin), _vec3(bmax),
                                              C.byref(p), C.c_void_p(d_keys), C.c_void_p(d_perm),
                                              C.c_void_p(d_level), C.c_void_p(d_dup), C.byref(stats)))
        return _stats_dict(stats)

    def build_node_lists_device(self, d_keys_sorted, d_level, n, d_order):
        """Device version of build_node_lists: d_order (u32 x n, device) receives the order; returns the node table."""
        cap = max(int(n), 1)
        nl = np.empty(cap, dtype=np.int8)
        nk = np.empty(cap, dtype=np.uint64)
        no = np.empty(cap, dtype=np.uint64)
        nc = np.empty(cap, dtype=np.uint64)
        num = C.c_uint64()
        self._check(self._lib.swz_build_node_lists_device(self._ctx, C.c_void_p(d_keys_sorted), C.c_void_p(d_level), int(n),
                                                          C.c_void_p(d_order), cap, nl.ctypes.data_as(_i8p),
                                                          nk.ctypes.data_as(_u64p), no.ctypes.data_as(_u64p),
                                                          nc.ctypes.data_as(_u64p), C.byref(num)))
        m = int(num.value)
        return dict(level=nl[:m].copy(), key=nk[:m].copy(), offset=no[:m].copy(), count=nc[:m].copy())

    def gather_payload_device(self, d_perm, d_order, n, d_xyz, d_attrs_in, d_xyz_out, d_attrs_out):
        """Row i of every output column = row perm[order[i]] of the input column (dicts name -> device pointer)."""
        cin, cout = device_columns(d_attrs_in), device_columns(d_attrs_out)
        self._check(self._lib.swz_gather_payload_device(self._ctx, C.c_void_p(d_perm), C.c_void_p(d_order), int(n),
                                                        C.c_void_p(d_xyz), C.byref(cin), C.c_void_p(d_xyz_out),
                                                        C.byref(cout)))

    def las_decode_device(self, d_records, n, scale, offset, bmin, bmax, point_format, record_bytes, d_xyz, d_attrs=None):
        """Raw LAS 1.2 point records (formats 0-3, device memory) -> positions and attribute columns on the device."""
        lay = _LasLayout(_vec3(scale), _vec3(offset), _vec3(bmin), _vec3(bmax), int(point_format), int(record_bytes))
        cols = device_columns(d_attrs)
        self._check(self._lib.swz_las_decode_device(self._ctx, C.c_void_p(d_records), int(n), C.byref(lay),
                                                    C.c_void_p(d_xyz), C.byref(cols)))

    def srs_transform_device(self, srs, d_xyz, n=None, target=SRS_ECEF):
        """swz_srs_transform_device: n rows of 24 bytes at d_xyz (a device pointer, or a contiguous float64 torch tensor of
        shape (n, 3)) from the source projection to ECEF or WGS84, in place."""
        _check_target(target)
        if hasattr(d_xyz, "data_ptr"):
            if not d_xyz.is_contiguous() or d_xyz.element_size() != 8 or d_xyz.numel() % 3:
                raise ValueError("srs_transform_device: a contiguous float64 tensor of rows of three")
            n = d_xyz.numel() // 3 if n is None else n
            d_xyz = d_xyz.data_ptr()
        self._check(self._lib.swz_srs_transform_device(self._ctx, _as_srs(srs)._ref(), int(target), C.c_void_p(d_xyz), int(n)))

    def las_decode_segments_device(self, d_raw, raw_bytes, segments, d_xyz, d_attrs=None, shift_center=None, srs=None):
        """swz_las_decode_segments_device: raw point records of several files (device memory, any alignment) -> positions and
        attribute columns in one launch.  segments: dicts of first_row, count, byte_offset, scale, offset, min, max,
        point_format, record_bytes (the keys of a las_scan_files entry).  srs (a string or an Srs): positions go through the
        source projection to ECEF after the clamp and before the shift (swz_las_decode_segments_srs_device)."""
        segs = (_LasSegment * max(len(segments), 1))()
        for i, g in enumerate(segments):
            segs[i] = _LasSegment(int(g["first_row"]), int(g["count"]), int(g["byte_offset"]),
                                  _LasLayout(_vec3(g["scale"]), _vec3(g["offset"]), _vec3(g["min"]), _vec3(g["max"]),
                                             int(g["point_format"]), int(g["record_bytes"])))
        cols = device_columns(d_attrs)
        center = None if shift_center is None else _vec3(shift_center)
        srs = _as_srs(srs)
        if srs is not None:
            self._check(self._lib.swz_las_decode_segments_srs_device(self._ctx, C.c_void_p(d_raw), int(raw_bytes), len(segments), segs,
                                                                     center, C.c_void_p(d_xyz), C.byref(cols), srs._ref()))
            return
        self._check(self._lib.swz_las_decode_segments_device(self._ctx, C.c_void_p(d_raw), int(raw_bytes), len(segments), segs, center,
                                                             C.c_void_p(d_xyz), C.byref(cols)))

    def bin_unpack_segments_device(self, d_raw, raw_bytes, segments, d_xyz, d_attrs=None):
        """swz_bin_unpack_segments_device: uncompressed BIN file images (device memory, any alignment) -> positions and
        attribute columns in one launch.  segments: dicts of first_row, count, byte_offset and attrs (names or a mask: the
        arrays the image holds).  d_xyz may be None; d_attrs: dict name -> device pointer of the columns to fill (zeros where
        a segment lacks the array)."""
        segs = (_BinSegment * max(len(segments), 1))()
        for i, g in enumerate(segments):
            segs[i] = _BinSegment(int(g["first_row"]), int(g["count"]), int(g["byte_offset"]), _las_mask(g.get("attrs", ())), 0)
        cols = device_columns(d_attrs)
        self._check(self._lib.swz_bin_unpack_segments_device(self._ctx, C.c_void_p(d_raw), int(raw_bytes), segs, len(segments),
                                                             C.c_void_p(d_xyz), C.byref(cols)))

    def pnts_unpack_segments_device(self, d_raw, raw_bytes, segments, d_xyz, d_attrs=None):
        """swz_pnts_unpack_segments_device: the arrays of .pnts files (device memory, any alignment and order) -> positions
        (the stored floats widened) and the rgb / intensity columns in one launch.  segments: dicts of first_row, count,
        position_offset, rgb_offset, intensity_offset (absolute in d_raw) and attrs (names or a mask: the arrays the segment
        holds); `reserved` is passed on.  d_xyz may be None; d_attrs: dict name -> device pointer of the columns to fill
        (zeros where a segment lacks the array)."""
        segs = (_PntsSegment * max(len(segments), 1))()
        for i, g in enumerate(segments):
            attrs = g.get("attrs", ())
            mask = int(attrs) if isinstance(attrs, (int, np.integer)) else _pnts_mask(attrs)
            segs[i] = _PntsSegment(int(g["first_row"]), int(g["count"]), int(g["position_offset"]), int(g.get("rgb_offset", 0)),
                                   int(g.get("intensity_offset", 0)), mask, int(g.get("reserved", 0)))
        cols = device_columns(d_attrs)
        self._check(self._lib.swz_pnts_unpack_segments_device(self._ctx, C.c_void_p(d_raw), int(raw_bytes), segs, len(segments),
                                                              C.c_void_p(d_xyz), C.byref(cols)))

    def _select_device(self, call, selection, attrs, d_xyz, n, box_min, box_max, capacity, d_xyz_out, d_attrs, d_attrs_out, d_row_out):
        """box_select_device, region_select_device and filter_select_device.  call: the C function; selection: the structs (or
        None) it takes behind the box -- none, the region, or region and filter; attrs: names or a mask."""
        cin, cout = device_columns(d_attrs), device_columns(d_attrs_out)
        count = C.c_uint64()
        st = call(self._ctx, C.c_void_p(d_xyz), int(n), C.byref(cin), _las_mask(attrs), _vec3(box_min), _vec3(box_max),
                  *[_ref(x) for x in selection], int(capacity), C.c_void_p(d_xyz_out), C.byref(cout), C.c_void_p(d_row_out), C.byref(count))
        if st != 0:
            err = SwzError(st, self._lib.swz_last_error(self._ctx).decode())
            err.needed = int(count.value)
            raise err
        return int(count.value)

    def box_select_device(self, d_xyz, n, box_min, box_max, capacity, d_xyz_out, d_attrs=None, d_attrs_out=None, attrs=None,
                          d_row_out=None):
        """swz_box_select_device: the rows of d_xyz (n rows on the device) inside the closed box [box_min, box_max], compacted
        in their order into d_xyz_out, with the columns attrs (names or a mask; None: those of d_attrs) moved from d_attrs to
        d_attrs_out (dicts name -> device pointer) and, where d_row_out is given, every output row's input row (u32).
        d_xyz_out None with capacity 0 counts only.  Returns the count; a count above capacity raises SwzError ("capacity")
        whose `needed` attribute is the count, and touches no output."""
        return self._select_device(self._lib.swz_box_select_device, (), list(d_attrs or ()) if attrs is None else attrs, d_xyz, n, box_min,
                                   box_max, capacity, d_xyz_out, d_attrs, d_attrs_out, d_row_out)

    def region_select_device(self, d_xyz, n, box_min, box_max, region, capacity, d_xyz_out, d_attrs=None, d_attrs_out=None, attrs=None,
                             d_row_out=None):
        """swz_region_select_device: box_select_device for the box cut by region (a Region; None: the box alone, the bytes of
        box_select_device).  Everything else -- order, count-only mode, the capacity refusal and its `needed` -- is
        box_select_device's."""
        rg = None if region is None else region._struct()
        return self._select_device(self._lib.swz_region_select_device, (rg,), list(d_attrs or ()) if attrs is None else attrs, d_xyz, n,
                                   box_min, box_max, capacity, d_xyz_out, d_attrs, d_attrs_out, d_row_out)

    def filter_select_device(self, d_xyz, n, box_min, box_max, region, filter, capacity, d_xyz_out, d_attrs=None, d_attrs_out=None,
                             attrs=None, d_row_out=None):
        """swz_filter_select_device: region_select_device for the rows that also pass filter (a Filter; None: the bytes of
        region_select_device).  d_attrs holds the columns of attrs (default: those of d_attrs_out) and the filter's; only the
        columns of attrs are written."""
        rg = None if region is None else region._struct()
        fl = None if filter is None else filter._struct()
        return self._select_device(self._lib.swz_filter_select_device, (rg, fl), list(d_attrs_out or ()) if attrs is None else attrs, d_xyz, n,
                                   box_min, box_max, capacity, d_xyz_out, d_attrs, d_attrs_out, d_row_out)

    def dataset_query_filtered(self, directory, box_min, box_max, region=None, filter=None, **kwargs):
        """dataset_query_filtered(self, directory, box_min, box_max, region, filter, ...)"""
        return dataset_query_filtered(self, directory, box_min, box_max, region, filter, **kwargs)

    def raster_clear_device(self, frame, d_cells):
        """swz_raster_clear_device: presets the frame's nx * ny cells at d_cells (a device pointer; 32 bytes per cell)."""
        f = _raster_frame_struct(frame)
        self._check(self._lib.swz_raster_clear_device(self._ctx, C.byref(f), C.c_void_p(d_cells)))

    def raster_accumulate_device(self, d_xyz, n, box_min, box_max, frame, d_cells, d_value=None):
        """swz_raster_accumulate_device: adds the rows of d_xyz (n rows on the device) inside the closed box to the table at
        d_cells, which it does not clear; frame is raster_frame_of's for this box; d_value is the device pointer of the value's
        column (None for z)."""
        f = _raster_frame_struct(frame)
        self._check(self._lib.swz_raster_accumulate_device(self._ctx, C.c_void_p(d_xyz), int(n), C.c_void_p(d_value), _vec3(box_min),
                                                           _vec3(box_max), C.byref(f), C.c_void_p(d_cells)))

    def dataset_rasterize(self, directory, box_min, box_max, nx, ny, **kwargs):
        """dataset_rasterize(self, directory, box_min, box_max, nx, ny, ...)"""
        return dataset_rasterize(self, directory, box_min, box_max, nx, ny, **kwargs)

    def node_summaries_device(self, n, d_attrs, nodes, attrs=None):
        """swz_node_summaries_device: per node of the table (dict of offset / count over n rows in stored order) and per column
        of attrs (names or a mask; default: those of d_attrs, a dict name -> device pointer) one entry of SUMMARY_DTYPE, shape
        (nodes, columns), columns in ascending attribute index: the set of values of a one-byte column with lo / hi derived
        from it, the exact min and max of a uint16 column or of the GPS times (NaN left out and flagged)."""
        cin = device_columns(d_attrs)
        mask = _summary_mask(list(d_attrs or ()) if attrs is None else attrs)
        no, nc = _node_columns(nodes, "offset", "count")
        cols = bin(mask & 0xFFFFFFFF).count("1")
        out = np.zeros((nc.shape[0], cols), dtype=SUMMARY_DTYPE)
        self._check(self._lib.swz_node_summaries_device(self._ctx, int(n), C.byref(cin), mask, nc.shape[0], no.ctypes.data_as(_u64p),
                                                        nc.ctypes.data_as(_u64p), out.ctypes.data if out.size else None))
        return out

    def dataset_summarize(self, directory, **kwargs):
        """dataset_summarize(self, directory, ...)"""
        return dataset_summarize(self, directory, **kwargs)

    def dataset_query_region(self, directory, box_min, box_max, region, **kwargs):
        """dataset_query_region(self, directory, box_min, box_max, region, ...)"""
        return dataset_query_region(self, directory, box_min, box_max, region, **kwargs)

    def dataset_query(self, directory, box_min, box_max, **kwargs):
        """dataset_query(self, directory, box_min, box_max, ...)"""
        return dataset_query(self, directory, box_min, box_max, **kwargs)

    def convert_dataset(self, src, dst, format, **kwargs):
        """convert_dataset(self, src, dst, format, ...)"""
        return convert_dataset(self, src, dst, format, **kwargs)

    def convert_dataset_world(self, src, dst, source_projection=None, **kwargs):
        """convert_dataset_world(self, src, dst, source_projection, ...)"""
        return convert_dataset_world(self, src, dst, source_projection, **kwargs)

    def srs_project_node_boxes_device(self, srs, d_xyz, n, nodes):
        """swz_srs_project_node_boxes_device: n rows of 24 bytes at d_xyz (a device pointer), in stored order, mapped in place
        to ECEF through srs (a string or an Srs; None: they stay), and (box_min, box_max), num_nodes x 3 float64 each: the
        exact componentwise min and max of the mapped rows [offset, offset + count) of every node of the table; a node
        without points has +inf / -inf.  All n rows are mapped, those outside every node too."""
        srs = _as_srs(srs)
        no, nc = _node_columns(nodes, "offset", "count")
        lo = np.empty((nc.shape[0], 3), dtype=np.float64)
        hi = np.empty((nc.shape[0], 3), dtype=np.float64)
        self._check(self._lib.swz_srs_project_node_boxes_device(self._ctx, srs._ref() if srs is not None else None, C.c_void_p(d_xyz),
                                                                int(n), nc.shape[0], no.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p),
                                                                lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp)))
        return lo, hi

    def pnts_pack_origin_device(self, d_perm, d_order, n, d_xyz, d_attrs, nodes, d_image, image_bytes, node_origin, attrs=(),
                                rgb_from=RGB_FROM_COLOR):
        """swz_pnts_pack_origin_device: pnts_pack_device with positions stored relative to node_origin (num_nodes x 3): the
        subtraction in double, then the narrowing."""
        cin = device_columns(d_attrs)
        no, nc = _node_columns(nodes, "offset", "count")
        org = np.ascontiguousarray(node_origin, dtype=np.float64).reshape(-1)
        if org.shape[0] != 3 * nc.shape[0]:
            raise ValueError("node_origin must hold 3 values per node")
        self._check(self._lib.swz_pnts_pack_origin_device(self._ctx, C.c_void_p(d_perm), C.c_void_p(d_order), int(n), C.c_void_p(d_xyz),
                                                          C.byref(cin), nc.shape[0], no.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p),
                                                          _pnts_mask(attrs), int(rgb_from), C.c_void_p(d_image), int(image_bytes),
                                                          org.ctypes.data_as(_dp)))

    def pnts_persist_nodes_rtc(self, directory, nodes, image, node_rtc_center, attrs=()):
        """swz_pnts_persist_nodes_rtc: pnts_persist_nodes with an RTC_CENTER per node (num_nodes x 3)."""
        img = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1)
        nl, nk, nc = _node_columns(nodes, "level", "key", "count")
        rtc = np.ascontiguousarray(node_rtc_center, dtype=np.float64).reshape(-1)
        if rtc.shape[0] != 3 * nc.shape[0]:
            raise ValueError("node_rtc_center must hold 3 values per node")
        self._check(self._lib.swz_pnts_persist_nodes_rtc(self._ctx, os.fsencode(directory), nl.shape[0], nl.ctypes.data_as(_i8p),
                                                         nk.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p), img.ctypes.data, img.shape[0],
                                                         _pnts_mask(attrs), rtc.ctypes.data_as(_dp)))

    def bin_persist_nodes(self, directory, nodes, xyz, attrs=None, compressed=False):
        """bin_persist_nodes with this context's writer threads and error text."""
        bin_persist_nodes(directory, nodes, xyz, attrs, compressed, ctx=self._ctx)

    def bin_pack_device(self, d_perm, d_order, n, d_xyz, d_attrs, nodes, d_image, image_bytes, attrs=()):
        """swz_bin_pack_device: the BIN files of all nodes of a table, laid out as bin_layout says, written into d_image
        (device, image_bytes bytes) by one kernel.  d_order None = identity (a tiler's export ids as d_perm)."""
        cin = device_columns(d_attrs)
        no, nc = _node_columns(nodes, "offset", "count")
        self._check(self._lib.swz_bin_pack_device(self._ctx, C.c_void_p(d_perm), C.c_void_p(d_order), int(n), C.c_void_p(d_xyz),
                                                  C.byref(cin), nc.shape[0], no.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p),
                                                  _las_mask(attrs), C.c_void_p(d_image), int(image_bytes)))

    def bin_persist_nodes_image(self, directory, nodes, image, attrs=(), compressed=False):
        """bin_persist_nodes_image with this context's writer threads and error text."""
        bin_persist_nodes_image(directory, nodes, image, attrs, compressed, ctx=self._ctx)

    def pnts_pack_device(self, d_perm, d_order, n, d_xyz, d_attrs, nodes, d_image, image_bytes, attrs=(), rgb_from=RGB_FROM_COLOR):
        """swz_pnts_pack_device: the .pnts bodies of all nodes of a table, laid out as pnts_layout says, written into
        d_image (device, image_bytes bytes) in one pass.  d_order None = identity (a tiler's export ids as d_perm)."""
        cin = device_columns(d_attrs)
        no, nc = _node_columns(nodes, "offset", "count")
        self._check(self._lib.swz_pnts_pack_device(self._ctx, C.c_void_p(d_perm), C.c_void_p(d_order), int(n), C.c_void_p(d_xyz),
                                                   C.byref(cin), nc.shape[0], no.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p),
                                                   _pnts_mask(attrs), int(rgb_from), C.c_void_p(d_image), int(image_bytes)))

    def node_boxes_device(self, d_perm, d_order, n, d_xyz, nodes):
        """swz_node_boxes_device: (box_min, box_max), num_nodes x 3 float64 each -- the exact componentwise min and max of
        the rows d_xyz[d_perm[d_order[offset + i]]] of every node of the table; a node without points has +inf / -inf.
        d_order None = identity (a tiler's export ids as d_perm)."""
        no, nc = _node_columns(nodes, "offset", "count")
        lo = np.empty((nc.shape[0], 3), dtype=np.float64)
        hi = np.empty((nc.shape[0], 3), dtype=np.float64)
        self._check(self._lib.swz_node_boxes_device(self._ctx, C.c_void_p(d_perm), C.c_void_p(d_order), int(n), C.c_void_p(d_xyz),
                                                    nc.shape[0], no.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p),
                                                    lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp)))
        return lo, hi

    def pnts_persist_nodes(self, directory, nodes, image, attrs=(), rtc_center=None):
        """One .pnts file per node of a node table out of a host copy of the image pnts_pack_device wrote."""
        img = np.ascontiguousarray(image, dtype=np.uint8).reshape(-1)
        nl, nk, nc = _node_columns(nodes, "level", "key", "count")
        rtc = _vec3(rtc_center) if rtc_center is not None else None
        self._check(self._lib.swz_pnts_persist_nodes(self._ctx, os.fsencode(directory), nl.shape[0], nl.ctypes.data_as(_i8p),
                                                     nk.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p), img.ctypes.data, img.shape[0],
                                                     _pnts_mask(attrs), rtc))

    def las_pack_device(self, d_perm, d_order, n, d_xyz, d_attrs, nodes, las_offset, las_scale, d_image, image_bytes, attrs=()):
        """swz_las_pack_device: the LAS point records of all nodes of a table, laid out as las_image_layout says, written
        into d_image (device, image_bytes bytes) by one kernel.  las_offset (num_nodes x 3) and las_scale (num_nodes): the
        box minimum and the scale of every node.  d_order None = identity (a tiler's export ids as d_perm)."""
        cin = device_columns(d_attrs)
        no, nc = _node_columns(nodes, "offset", "count")
        lo = np.ascontiguousarray(las_offset, dtype=np.float64).reshape(-1, 3)
        ls = np.ascontiguousarray(las_scale, dtype=np.float64).reshape(-1)
        if not (no.shape[0] == nc.shape[0] == lo.shape[0] == ls.shape[0]):
            raise ValueError("the node table, the offsets and the scales differ in length")
        self._check(self._lib.swz_las_pack_device(self._ctx, C.c_void_p(d_perm), C.c_void_p(d_order), int(n), C.c_void_p(d_xyz),
                                                  C.byref(cin), nc.shape[0], no.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p),
                                                  lo.ctypes.data_as(_dp), ls.ctypes.data_as(_dp), _las_mask(attrs), C.c_void_p(d_image),
                                                  int(image_bytes)))

    def las_persist_nodes(self, directory, nodes, image, attrs, box_min, box_max, scale, naming=LAS_NAMING_POTREE):
        """las_persist_nodes with this context's writer threads and error text."""
        las_persist_nodes(directory, nodes, image, attrs, box_min, box_max, scale, naming, ctx=self._ctx)

    # ------------------------------------------------------------------ sharded batches (one context per GPU)
    def partition_by_octant_device(self, d_keys, n, d_perm):
        """Groups point indices by level-0 octant (stable).  Returns the 8 octant counts."""
        counts = (C.c_uint64 * 8)()
        self._check(self._lib.swz_partition_by_octant_device(self._ctx, C.c_void_p(d_keys), int(n),
                                                             C.c_void_p(d_perm), counts))
        return [int(v) for v in counts]

    def shard_presort_device(self, d_xyz_local, n, bmin, bmax, params, ghost_capacity):
        """The ghost-independent part of shard_begin_device (index + sort + gather), done ahead of time."""
        p = params._c()
        self._check(self._lib.swz_shard_presort_device(self._ctx, C.c_void_p(d_xyz_local), int(n), _vec3(bmin), _vec3(bmax),
                                                       C.byref(p), int(ghost_capacity)))

    def shard_begin_device(self, d_xyz_local, n, bmin, bmax, params, global_points, d_ghost_xyz=None, num_ghosts=0):
        """Indexes + sorts the shard and samples the root node.  Returns how many local points the root took."""
        info = _ShardInfo(int(global_points), C.c_void_p(d_ghost_xyz), int(num_ghosts))
        p = params._c()
        taken = C.c_uint64()
        self._check(self._lib.swz_shard_begin_device(self._ctx, C.c_void_p(d_xyz_local), int(n), _vec3(bmin),
                                                     _vec3(bmax), C.byref(p), C.byref(info), C.byref(taken)))
        return int(taken.value)

    def shard_root_taken_device(self, d_xyz_out):
        self._check(self._lib.swz_shard_root_taken_device(self._ctx, C.c_void_p(d_xyz_out)))

    def shard_finish_device(self, d_keys, d_perm, d_level):
        stats = _TileStats()
        self._check(self._lib.swz_shard_finish_device(self._ctx, C.c_void_p(d_keys), C.c_void_p(d_perm),
                                                      C.c_void_p(d_level), C.byref(stats)))
        return _stats_dict(stats)

    # -- FAST (TilingAlgorithmV3) on a sharded batch (include/swz_gpu.h, swz_shard_fast_*)
    def shard_fast_begin_device(self, d_xyz_local, n, bmin, bmax, params):
        """Indexes + sorts the shard's points.  Returns its points per 6-octant prefix (8^6 counts)."""
        counts = np.zeros(1 << 18, dtype=np.uint32)
        p = params._c()
        self._check(self._lib.swz_shard_fast_begin_device(self._ctx, C.c_void_p(d_xyz_local), int(n), _vec3(bmin), _vec3(bmax),
                                                          C.byref(p), counts.ctypes.data_as(_u32p)))
        return counts

    def shard_fast_run(self, start_level):
        """The levels from the start level down and the local reconstruction.  Returns the points of this shard's level-0 nodes."""
        out = C.c_uint64()
        self._check(self._lib.swz_shard_fast_run(self._ctx, int(start_level), C.byref(out)))
        return int(out.value)

    def shard_fast_root_candidates_device(self, d_keys, d_xyz):
        self._check(self._lib.swz_shard_fast_root_candidates_device(self._ctx, C.c_void_p(d_keys), C.c_void_p(d_xyz)))

    def shard_fast_set_root_device(self, d_taken):
        self._check(self._lib.swz_shard_fast_set_root_device(self._ctx, C.c_void_p(d_taken)))

    def shard_fast_finish_device(self, d_keys, d_perm, d_level, d_dup):
        stats = _TileStats()
        self._check(self._lib.swz_shard_fast_finish_device(self._ctx, C.c_void_p(d_keys), C.c_void_p(d_perm), C.c_void_p(d_level),
                                                           C.c_void_p(d_dup), C.byref(stats)))
        return _stats_dict(stats)

    def sample_points_device(self, sampler, max_points_per_node, d_keys, d_idx, n, d_xyz, num_points, node_key, node_level, root_min,
                             root_max, spacing_at_root, behaviour, d_taken):
        """swz_sample_points on device buffers.  Returns the number of taken points."""
        num = C.c_uint64()
        self._check(self._lib.swz_sample_points_device(self._ctx, int(sampler), int(max_points_per_node), C.c_void_p(d_keys),
                                                       C.c_void_p(d_idx), int(n), C.c_void_p(d_xyz), int(num_points), int(node_key),
                                                       int(node_level), _vec3(root_min), _vec3(root_max), C.c_float(spacing_at_root),
                                                       int(behaviour), C.c_void_p(d_taken), C.byref(num)))
        return int(num.value)

    # -- the MIN_DISTANCE root of a sharded batch swept by all ranks at once (one process per GPU; include/swz_gpu.h)
    def shard_joint_root_possible(self, bmin, bmax, params):
        p = params._c()
        return bool(self._lib.swz_shard_joint_root_possible(self._ctx, C.byref(p), _vec3(bmin), _vec3(bmax)))

    def shard_joint_root_begin(self, shard, num_shards, all_gather_bytes):
        """all_gather_bytes(mine: bytes) -> list of every rank's bytes, in rank order (a collective of the driver)."""
        def cb(_arg, mine, nbytes, out):
            try:
                parts = all_gather_bytes(C.string_at(mine, nbytes))
                C.memmove(out, b"".join(parts), nbytes * len(parts))
                return 0
            except Exception:  # the library turns this into an error status on every rank
                return 1
        self._joint_cb = EXCHANGE_FN(cb)  # must outlive the calls that use it
        self._check(self._lib.swz_shard_joint_root_begin(self._ctx, int(shard), int(num_shards), self._joint_cb, None))

    def shard_joint_root_probe(self, shard, num_shards, all_gather_bytes):
        """Collective: True when every rank can map and read the lower ranks' device memory (the joint root needs that)."""
        def cb(_arg, mine, nbytes, out):
            try:
                parts = all_gather_bytes(C.string_at(mine, nbytes))
                C.memmove(out, b"".join(parts), nbytes * len(parts))
                return 0
            except Exception:
                return 1
        fn = EXCHANGE_FN(cb)
        usable = C.c_int(0)
        self._check(self._lib.swz_shard_joint_root_probe(self._ctx, int(shard), int(num_shards), fn, None, C.byref(usable)))
        return bool(usable.value)

    def shard_joint_root_meet(self, ok=True):
        self._check(self._lib.swz_shard_joint_root_meet(self._ctx, 1 if ok else 0))

    def shard_joint_root_end(self):
        self._check(self._lib.swz_shard_joint_root_end(self._ctx))
        self._joint_cb = None


def fast_start_level_from_counts(counts, fast_concurrency):
    """The start level TilingAlgorithmV3 derives from the 2^18-bin prefix histogram of a batch's keys
    (TilingAlgorithms.cpp:1473-1535); counts: the histogram summed over all shards."""
    L = load_library()
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    assert c.shape[0] == 1 << 18
    out = C.c_int32(-1)
    st = L.swz_fast_start_level_from_counts(c.ctypes.data_as(_u64p), int(fast_concurrency), C.byref(out))
    if st != 0:
        raise SwzError(st, "swz_fast_start_level_from_counts failed")
    return int(out.value)


def pinned_empty(shape, dtype):
    """numpy array over page-locked host memory (swz_host_alloc_pinned).  The memory is released when the array
    and all its views are gone; keep it alive while asynchronous copies from it are in flight."""
    import weakref
    L = load_library()
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    nbytes = max(count * dt.itemsize, 1)
    ptr = C.c_void_p()
    st = L.swz_host_alloc_pinned(nbytes, C.byref(ptr))
    if st != 0:
        raise SwzError(st, "swz_host_alloc_pinned(%d bytes) failed" % nbytes)
    buf = (C.c_char * nbytes).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=dt, count=count).reshape(shape)
    weakref.finalize(arr, L.swz_host_free_pinned, C.c_void_p(ptr.value))
    return arr


class Tiler:
    """swz_tiler: one data set tiled batch after batch on one context (multi-batch semantics of the reference's
    TilingAlgorithm objects, TilingAlgorithms.cpp:50-109, 272-275, 1362-1453, 1661-1784)."""

    def __init__(self, ctx, bmin, bmax, params, capacity_hint=0):
        self._ctx = ctx
        self._lib = ctx._lib
        self._t = C.c_void_p()
        p = params._c()
        ctx._check(self._lib.swz_tiler_create(ctx._ctx, _vec3(bmin), _vec3(bmax), C.byref(p), int(capacity_hint),
                                              C.byref(self._t)))
        self._keep = []

    def poison(self, why="poisoned by the caller"):
        """Marks the tiler failed (what a failing batch does by itself): every later call raises ERR_TILER_FAILED."""
        self._ctx._check(self._lib.swz_tiler_poison(self._t, why.encode()))

    def pool_residency(self):
        """(bytes of the pools in device memory, bytes spilled to mapped page-locked host memory)"""
        dev, host = C.c_uint64(), C.c_uint64()
        self._ctx._check(self._lib.swz_tiler_pool_residency(self._t, C.byref(dev), C.byref(host)))
        return int(dev.value), int(host.value)

    def reserve(self, total_points):
        """room in the pools for total_points points of the data set, now (swz_tiler_reserve)"""
        self._lib.swz_tiler_reserve.argtypes = [C.c_void_p, C.c_uint64]
        self._ctx._check(self._lib.swz_tiler_reserve(self._t, int(total_points)))

    def store_residency(self):
        """(bytes of the node store in device memory, bytes placed in mapped page-locked host memory)"""
        dev, host = C.c_uint64(), C.c_uint64()
        self._ctx._check(self._lib.swz_tiler_store_residency(self._t, C.byref(dev), C.byref(host)))
        return int(dev.value), int(host.value)

    def path_counts(self):
        """swz_tiler_path_counts: {name of TILER_PATHS: how often the tiler's batches took that way through the node store}"""
        out = (C.c_uint64 * len(TILER_PATHS))()
        self._ctx._check(self._lib.swz_tiler_path_counts(self._t, out, len(TILER_PATHS)))
        return {name: int(out[i]) for i, name in enumerate(TILER_PATHS)}

    def close(self):
        if getattr(self, "_t", None):
            if getattr(self._ctx, "_ctx", None):  # a context that is gone took the tiler's memory with it
                self._lib.swz_tiler_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add_batch_device(self, d_xyz, n):
        stats = _TileStats()
        self._ctx._check(self._lib.swz_tiler_add_batch_device(self._t, C.c_void_p(d_xyz), int(n), C.byref(stats)))
        return _stats_dict(stats)

    def stage_batch(self, xyz, attrs=None):
        """Asynchronous copy of a host batch (use pinned_empty arrays for real overlap) into the device pools."""
        x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        cols, keep = _host_columns(attrs, x.shape[0])
        self._ctx._check(self._lib.swz_tiler_stage_batch(self._t, C.c_void_p(x.ctypes.data), x.shape[0], C.byref(cols)))
        self._keep.append((x, keep))  # (after the check: a refused batch is not staged, tile_staged pops one per staged batch)

    def tile_staged(self):
        stats = _TileStats()
        self._ctx._check(self._lib.swz_tiler_tile_staged(self._t, C.byref(stats)))
        if self._keep:
            self._keep.pop(0)
        return _stats_dict(stats)

    def add_batch(self, xyz, attrs=None):
        self.stage_batch(xyz, attrs)
        return self.tile_staged()

    def finalize(self):
        stats = _TileStats()
        self._ctx._check(self._lib.swz_tiler_finalize(self._t, C.byref(stats)))
        return _stats_dict(stats)

    def info(self):
        i = _TilerInfo()
        self._ctx._check(self._lib.swz_tiler_get_info(self._t, C.byref(i)))
        return {k: getattr(i, k) for k, _ in _TilerInfo._fields_}

    def node_table(self):
        cap = max(int(self.info()["num_nodes"]), 1)
        nl = np.empty(cap, dtype=np.int8)
        nk = np.empty(cap, dtype=np.uint64)
        no = np.empty(cap, dtype=np.uint64)
        nc = np.empty(cap, dtype=np.uint64)
        num = C.c_uint64()
        self._ctx._check(self._lib.swz_tiler_node_table(self._t, cap, nl.ctypes.data_as(_i8p), nk.ctypes.data_as(_u64p),
                                                        no.ctypes.data_as(_u64p), nc.ctypes.data_as(_u64p), C.byref(num)))
        m = int(num.value)
        return dict(level=nl[:m].copy(), key=nk[:m].copy(), offset=no[:m].copy(), count=nc[:m].copy())

    def node_boxes(self):
        """swz_tiler_node_boxes: (box_min, box_max), num_nodes x 3 float64 each, the boxes of the nodes' points in the order
        of node_table, reduced on the device from the pools (a node without points: +inf / -inf)."""
        cap = max(int(self.info()["num_nodes"]), 1)
        lo = np.empty((cap, 3), dtype=np.float64)
        hi = np.empty((cap, 3), dtype=np.float64)
        num = C.c_uint64()
        self._ctx._check(self._lib.swz_tiler_node_boxes(self._t, cap, lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp), C.byref(num)))
        m = int(num.value)
        return lo[:m].copy(), hi[:m].copy()

    def export_device(self, d_keys, d_ids, d_level):
        self._ctx._check(self._lib.swz_tiler_export_device(self._t, C.c_void_p(d_keys), C.c_void_p(d_ids),
                                                           C.c_void_p(d_level)))

    # -- one tiler per GPU of a multi-GPU run (schwarzwald_amd/sharded.py drives these)
    def shard_begin_device(self, d_xyz, n, d_attrs, global_new_points, global_root_stored, d_ghost_xyz=None, num_ghosts=0):
        """Indexes + sorts this shard's part of the batch and decides the root node.  Returns the points of the
        root's file on this shard afterwards."""
        info = _TilerShardInfo(int(global_new_points), int(global_root_stored), C.c_void_p(d_ghost_xyz), int(num_ghosts))
        cols = device_columns(d_attrs)
        out = C.c_uint64()
        self._ctx._check(self._lib.swz_tiler_shard_begin_device(self._t, C.c_void_p(d_xyz), int(n), C.byref(cols),
                                                                C.byref(info), C.byref(out)))
        return int(out.value)

    def shard_finish(self):
        stats = _TileStats()
        self._ctx._check(self._lib.swz_tiler_shard_finish(self._t, C.byref(stats)))
        return _stats_dict(stats)

    # -- FAST (TilingAlgorithmV3) on a sharded data set: the driver sums the shards' prefix histograms, derives the start
    # level, and at the end samples the root from the level-0 files of all shards (sharded.ShardedBatchTiler)
    def shard_fast_histogram(self):
        counts = np.zeros(1 << 18, dtype=np.uint32)
        self._ctx._check(self._lib.swz_tiler_shard_fast_histogram(self._t, counts.ctypes.data_as(_u32p)))
        return counts

    def shard_set_start_level(self, start_level):
        self._ctx._check(self._lib.swz_tiler_shard_set_start_level(self._t, int(start_level)))

    def shard_fast_finalize_local(self):
        stats = _TileStats()
        self._ctx._check(self._lib.swz_tiler_shard_fast_finalize_local(self._t, C.byref(stats)))
        return _stats_dict(stats)

    def shard_fast_set_root(self, d_taken):
        self._ctx._check(self._lib.swz_tiler_shard_fast_set_root(self._t, C.c_void_p(d_taken)))

    def level_count(self, level):
        out = C.c_uint64()
        self._ctx._check(self._lib.swz_tiler_level_count(self._t, int(level), C.byref(out)))
        return int(out.value)

    def level_positions_device(self, level, d_xyz_out):
        self._ctx._check(self._lib.swz_tiler_level_positions_device(self._t, int(level), C.c_void_p(d_xyz_out)))

    def write_output(self, directory, format, attrs=(), rgb_from=RGB_FROM_COLOR, global_offset=None, chunk_points=0, ept=None,
                     tight_bounds=False, flags=0):
        """swz_tiler_write_output: every node file of the tiler, and the format's metadata, into directory.  format: a key of
        OUTPUT_FORMATS; attrs: the attribute columns to write (names or a mask), a subset of what the batches carried;
        rgb_from / global_offset: 3DTILES; chunk_points: stored points per chunk (0 = default); ept: ENTWINE_LAS, the keyword
        arguments of ept_json_write as a dict (bounds, conforming_bounds, points, ...) or None for no ept.json.  Returns the
        stats as a dict (nodes, stored_points, bytes_written, chunks, pack_ms, copy_ms, write_ms, wall_ms).  tight_bounds:
        SWZ_OUT_TIGHT_BOUNDS -- tileset boxes, LAS header extents and ept.json's boundsConforming are the boxes of the points,
        reduced on the device, not the octree cubes; refused for BIN / BINZ.  flags: further bits of the params' flags."""
        fmt = OUTPUT_FORMATS[format] if isinstance(format, str) else int(format)
        p = _OutputParams(fmt, _las_mask(attrs), int(rgb_from), int(flags) | (OUT_TIGHT_BOUNDS if tight_bounds else 0),
                          _vec3(global_offset if global_offset is not None else (0, 0, 0)), int(chunk_points), None)
        keep = None
        if ept is not None:
            srs = ept.get("srs") or {}
            keep = _EptJson(_vec3(ept["bounds"][0]), _vec3(ept["bounds"][1]), _vec3(ept["conforming_bounds"][0]),
                            _vec3(ept["conforming_bounds"][1]), int(ept["points"]), _las_mask(ept.get("attrs", ())), 0,
                            float(ept.get("span", 0.0)), srs.get("authority", "").encode(), srs.get("horizontal", "").encode(),
                            srs.get("wkt", "").encode(), ept.get("version", "").encode())
            p.ept = C.pointer(keep)
        stats = _OutputStats()
        self._ctx._check(self._lib.swz_tiler_write_output(self._t, os.fsencode(directory), C.byref(p), C.byref(stats)))
        return {k: getattr(stats, k) for k, _ in _OutputStats._fields_}

    def write_properties(self, directory):
        """swz_tiler_write_properties: directory/properties.json (root box, spacing_at_root, points added) -- what
        convert_dataset and the reference's converter find the root of a BIN, BINZ, LAS or 3DTILES data set with."""
        self._ctx._check(self._lib.swz_tiler_write_properties(self._t, os.fsencode(directory)))

    def set_source_srs(self, srs):
        """swz_tiler_set_source_srs: add_las_files projects its input to ECEF (a string or an Srs; None clears).  Refused once
        the tiler holds points."""
        srs = _as_srs(srs)
        self._ctx._check(self._lib.swz_tiler_set_source_srs(self._t, None if srs is None else srs._ref()))

    def add_las_files(self, paths, batch_points=0, attrs=None, shift_to_center=False, skip_unreadable=False, source_projection=None):
        """swz_tiler_add_las_files: a data set of uncompressed LAS files read, decoded on the device straight into the pools
        and tiled, batch after batch.  attrs: the attribute columns to carry (names or a mask; None = all the files have in
        common); batch_points 0 = 10 M.  Does not finalize.  Returns the stats as a dict (files, points, batches, bytes_read,
        read_ms, copy_ms, decode_ms, tile_ms, wait_ms, wall_ms).  source_projection (a string or an Srs): set_source_srs before
        the call -- the root box and the shift are then ECEF's (las_scan_files(srs=...)) --, so it can only be given to the
        call that brings the first points.  If the call is refused before a point is read the projection is cleared again and
        the tiler is as it was; once the call has brought points THE TILER KEEPS THE PROJECTION for its life (the library
        allows neither set nor clear on a tiler that holds points): a later add_las_files without source_projection projects
        too, which is what one data set in one CRS needs."""
        arr, n = _path_array(paths)
        mask = 0xFFFFFFFF if attrs is None else _las_mask(attrs)
        p = _InputParams(int(batch_points), mask, 1 if shift_to_center else 0, LAS_SCAN_SKIP_UNREADABLE if skip_unreadable else 0, 0)
        stats = _InputStats()
        if source_projection is not None:
            self.set_source_srs(source_projection)
        try:
            self._ctx._check(self._lib.swz_tiler_add_las_files(self._t, arr, n, C.byref(p), C.byref(stats)))
        except SwzError:
            if source_projection is not None and stats.points == 0 and self.info()["num_points"] == 0:
                self._lib.swz_tiler_set_source_srs(self._t, None)   # refused before a point was read: as it was
            raise
        return {k: getattr(stats, k) for k, _ in _InputStats._fields_}

    def pools_device(self):
        """(device pointer of the clamped positions by point id, dict name -> device pointer of the attribute pools)"""
        xyz = C.c_void_p()
        cols = _AttributeColumns()
        self._ctx._check(self._lib.swz_tiler_pools_device(self._t, C.byref(xyz), C.byref(cols)))
        attrs = {name: int(cols.column[idx]) for name, (idx, _, _) in ATTRIBUTES.items() if cols.column[idx]}
        return int(xyz.value or 0), attrs
