"""LAS node files and Entwine metadata (core/io/LASPersistence.cpp:16-271, core/io/EntwinePersistence.cpp:31-130, 197-333).

The expected bytes are written out by hand here: the 227-byte LAS 1.2 header with struct.pack, the point records with
numpy structured dtypes.  Quantisation is np.trunc(q + 0.5) / np.trunc(q - 0.5) on q = (x - offset) / scale in float64:
numpy's subtraction, division and addition are the same IEEE operations as the library's, so equality is exact and there
is no tolerance.  Outside int32 the library saturates and NaN becomes 0 (the reference's cast is undefined there).

CPU part: the scale rule, the layouts, the two host writers against the hand-written file, quantisation and attribute bits
on hard values, the reader on good, foreign and malformed files, the records decoded by the oracle's LAS decoder, the
hierarchy files and ept.json.  GPU part: swz_las_pack_device against the numpy image of synthetic node tables (no tiling
involved), its refusals, and tile -> node lists -> pack -> copy -> files -> hierarchy against the rows the oracle assigns.
"""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import oracle_lib as O
from test_pnts_persistence import _hard_positions, _oracle_node_rows

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ERR_BAD_ARG = 2
# the four record lengths: 20, 28, 26, 34 bytes
MASKS = [("intensity",), ("intensity", "gps_time"), ("rgb", "intensity"), ("rgb", "intensity", "gps_time")]
ALL = ("rgb", "intensity", "classification", "edge_of_flight_line", "gps_time", "number_of_returns", "return_number",
       "point_source_id", "scan_direction_flag", "scan_angle_rank", "user_data")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


# ------------------------------------------------------------------------------------------ the format, by hand
def _format(names):
    return ("gps_time" in names) + 2 * ("rgb" in names)


def _dtype(fmt):
    fields = [("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("intensity", "<u2"), ("bits", "u1"), ("classification", "u1"),
              ("scan_angle_rank", "i1"), ("user_data", "u1"), ("point_source_id", "<u2")]
    if fmt & 1:
        fields.append(("gps_time", "<f8"))
    if fmt & 2:
        fields.append(("rgb", "<u2", (3,)))
    dt = np.dtype(fields)
    assert dt.itemsize == 20 + 8 * (fmt & 1) + 6 * (fmt >> 1)
    return dt


def _quantize(x, offset, scale):
    with np.errstate(invalid="ignore", over="ignore"):
        q = (np.asarray(x, np.float64) - offset) / scale
        v = np.where(q >= 0, np.trunc(q + 0.5), np.trunc(q - 0.5))
    v = np.where(np.isnan(v), 0.0, np.clip(v, I32_MIN, I32_MAX))
    return v.astype(np.int64).astype(np.int32)


def _records(xyz, attrs, names, offset, scale):
    """The point records of rows (positions + dict of columns) of which the columns `names` are written."""
    fmt = _format(names)
    n = len(xyz)
    rec = np.zeros(n, dtype=_dtype(fmt))
    xyz = np.asarray(xyz, np.float64).reshape(n, 3)
    for k, f in enumerate("XYZ"):
        rec[f] = _quantize(xyz[:, k], offset[k], scale)
    get = lambda name: np.asarray(attrs[name]).astype(np.int64) if name in names else np.zeros(n, np.int64)
    rec["intensity"] = get("intensity")
    rec["bits"] = (get("return_number") & 7) | (get("number_of_returns") & 7) << 3 | (get("scan_direction_flag") & 1) << 6 | \
                  (get("edge_of_flight_line") & 1) << 7
    rec["classification"] = get("classification") & 31
    rec["scan_angle_rank"] = get("scan_angle_rank")
    rec["user_data"] = get("user_data")
    rec["point_source_id"] = get("point_source_id")
    if fmt & 1:
        rec["gps_time"] = attrs["gps_time"]
    if fmt & 2:
        rec["rgb"] = np.asarray(attrs["rgb"]).astype(np.uint16) << 8
    return rec.tobytes()


def _header(count, fmt, box_min, box_max, scale, data_at=227):
    h = struct.pack("<4sHHIHH8sBB32s32sHHHIIBHI5I", b"LASF", 0, 0, 0, 0, 0, bytes(8), 1, 2, bytes(32), b"pointcloud_tiler", 0, 0,
                    227, data_at, 0, fmt, 20 + 8 * (fmt & 1) + 6 * (fmt >> 1), count, count, 0, 0, 0, 0)
    h += struct.pack("<12d", scale, scale, scale, box_min[0], box_min[1], box_min[2], box_max[0], box_min[0], box_max[1], box_min[1],
                     box_max[2], box_min[2])
    assert len(h) == 227
    return h


def _columns(rng, n):
    return {
        "rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
        "intensity": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16),
        "classification": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "edge_of_flight_line": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "gps_time": rng.random(n) * 1e9,
        "number_of_returns": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "return_number": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "point_source_id": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16),
        "scan_direction_flag": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "scan_angle_rank": rng.integers(-128, 127, n, endpoint=True).astype(np.int8),
        "user_data": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
    }


def _hard_quotients():
    """quotients (x - offset) / scale for offset 0 and a scale that is a power of two: the products are exact"""
    return np.array([0.5, 1.5, 2.5, 1234567.5, -0.5, -1.5, -2.5, -1234567.5, 0.49999999999999994, -0.49999999999999994,
                     2.0 ** 31 - 1.5, 2.0 ** 31 - 0.5, -2.0 ** 31 - 0.5, 1e300, -1e300, np.nan, -0.0, 0.0, -7.25, 2.0 ** 31 - 1, -2.0 ** 31])


def _hard_xyz(scale):
    q = _hard_quotients()
    xyz = np.stack([q * scale, np.roll(q, 1) * scale, np.roll(q, 2) * scale], axis=1)
    assert np.array_equal(np.nan_to_num(xyz[:, 0] / scale, nan=7.0), np.nan_to_num(q, nan=7.0))   # the quotients are these
    return xyz


# ------------------------------------------------------------------------------------------ CPU: scale and layouts
def test_scale_rule_at_and_beside_every_threshold():
    import schwarzwald_amd as swz
    up = lambda v: float(np.nextafter(v, np.inf))
    down = lambda v: float(np.nextafter(v, -np.inf))
    for d, want in [(0.0, 0.0001), (down(1.0), 0.0001), (1.0, 0.0001), (up(1.0), 0.001), (down(100000.0), 0.001), (100000.0, 0.001),
                    (up(100000.0), 0.001), (down(1000000.0), 0.001), (1000000.0, 0.001), (up(1000000.0), 0.01), (1e12, 0.01)]:
        for axis in range(3):
            mn, mx = [5.0, -3.0, 0.0], [5.0, -3.0, 0.0]
            mn[axis] = 0.0       # a box that is a segment along one axis: its diagonal is exactly d
            mx[axis] = d
            assert swz.las_scale_from_bounds(mn, mx) == want, (d, axis)
    # the diagonal, not an edge: sqrt(3) * 0.6 > 1
    assert swz.las_scale_from_bounds([0, 0, 0], [0.6, 0.6, 0.6]) == 0.001
    assert swz.las_scale_from_bounds([0, 0, 0], [0.5, 0.5, 0.5]) == 0.0001


def test_record_layout_of_all_masks():
    import schwarzwald_amd as swz
    other = [a for a in ALL if a not in ("rgb", "gps_time")]
    for gps in (0, 1):
        for rgb in (0, 1):
            names = (["gps_time"] if gps else []) + (["rgb"] if rgb else [])
            want = (gps + 2 * rgb, 20 + 8 * gps + 6 * rgb)
            assert swz.las_record_layout(names) == want
            assert swz.las_record_layout(names + other) == want
            assert swz.las_record_layout(names + ["normal"]) == want        # accepted and ignored
    assert swz.las_record_layout(()) == (0, 20)
    with pytest.raises(swz.SwzError):
        swz.las_record_layout(1 << 12)


def test_image_layout_of_counts_and_record_lengths():
    import schwarzwald_amd as swz
    counts = [0, 1, 2, 3, 5, 7, 8, 4097]
    for names in MASKS:
        rb = 20 + 8 * ("gps_time" in names) + 6 * ("rgb" in names)
        got = swz.las_image_layout(counts, names)
        at = 0
        for k, c in enumerate(counts):
            size = (c * rb + 7) // 8 * 8
            assert got["offset"][k] == at and got["size"][k] == size and at % 8 == 0, (names, c)
            at += size
        assert got["total"] == at
    assert swz.las_image_layout([1], ("rgb", "gps_time"))["size"][0] == 40
    assert swz.las_image_layout([], ())["total"] == 0
    with pytest.raises(swz.SwzError):
        swz.las_image_layout([1 << 32], ())        # number_of_point_records is a u32


# ------------------------------------------------------------------------------------------ CPU: the host writers
@pytest.mark.parametrize("names", MASKS + [ALL, ()])
@pytest.mark.parametrize("n", [1, 2, 333])
def test_host_writers_against_the_hand_written_file(tmp_path, names, n):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(200 + n)
    box_min, box_max = [-1000.0, -1000.5, -999.25], [1000.0, 1000.0, 1000.0]
    xyz = _hard_positions(rng, n)
    cols = _columns(rng, n)
    scale = swz.las_scale_from_bounds(box_min, box_max)
    assert scale == 0.001
    body = _records(xyz, cols, names, box_min, scale)
    want = _header(n, _format(names), box_min, box_max, scale) + body
    p_rows, p_body = str(tmp_path / "rows.las"), str(tmp_path / "body.las")
    swz.las_write_node_rows(p_rows, xyz, cols, box_min, box_max, scale, write=names)
    swz.las_write_node(p_body, n, np.frombuffer(body, np.uint8), names, box_min, box_max, scale)
    assert open(p_rows, "rb").read() == want
    assert open(p_body, "rb").read() == want
    # a packed body with the image's padding behind it writes the same file
    swz.las_write_node(p_body, n, np.frombuffer(body + bytes(-len(body) % 8), np.uint8), names, box_min, box_max, scale)
    assert open(p_body, "rb").read() == want


@pytest.mark.parametrize("scale", [0.5, 0.25])
def test_quantisation_on_hard_values(tmp_path, scale):
    import schwarzwald_amd as swz
    xyz = _hard_xyz(scale)
    q = _hard_quotients()
    want = {0.5: 1, 1.5: 2, 2.5: 3, -0.5: -1, -1.5: -2, -2.5: -3, 0.49999999999999994: 1, -0.49999999999999994: -1,
            2.0 ** 31 - 1.5: I32_MAX, 2.0 ** 31 - 0.5: I32_MAX, -2.0 ** 31 - 0.5: I32_MIN, 1e300: I32_MAX, -1e300: I32_MIN, -7.25: -7,
            2.0 ** 31 - 1: I32_MAX, -2.0 ** 31: I32_MIN, 1234567.5: 1234568, -1234567.5: -1234568}
    got_np = _quantize(xyz[:, 0], 0.0, scale)
    for v, x in zip(q, got_np):      # the test's own quantiser first
        assert x == (0 if (np.isnan(v) or v == 0) else want[float(v)]), v
    p = str(tmp_path / "q.las")
    box = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    swz.las_write_node_rows(p, xyz, {}, *box, scale)
    rec = np.frombuffer(open(p, "rb").read()[227:], _dtype(0))
    assert np.array_equal(rec["X"], got_np)
    assert np.array_equal(rec["Y"], np.roll(got_np, 1)) and np.array_equal(rec["Z"], np.roll(got_np, 2))
    # points below the offset, and an offset that is not representable as a short decimal
    off = [0.1, 1e6 + 0.3, -0.7]
    rng = np.random.default_rng(5)
    pts = np.asarray(off) + (rng.random((500, 3)) - 0.75) * 1000.0
    pts[:len(q)] = _hard_positions(rng, len(q))
    swz.las_write_node_rows(p, pts, {}, off, [2e6, 2e6, 2e6], 0.001)
    assert open(p, "rb").read() == _header(500, 0, off, [2e6, 2e6, 2e6], 0.001) + _records(pts, {}, (), off, 0.001)
    rec = np.frombuffer(open(p, "rb").read()[227:], _dtype(0))
    assert (rec["X"] < 0).sum() > 100


def test_attribute_bits_of_every_value(tmp_path):
    import schwarzwald_amd as swz
    n = 256
    v = np.arange(n)
    cols = {"return_number": v.astype(np.uint8), "number_of_returns": v[::-1].astype(np.uint8),
            "classification": v.astype(np.uint8), "edge_of_flight_line": v.astype(np.uint8),
            "scan_direction_flag": (v // 2).astype(np.uint8), "scan_angle_rank": (v - 128).astype(np.int8),
            "rgb": np.stack([np.resize([0, 1, 255], n), np.resize([255, 0, 1], n), np.resize([1, 255, 0], n)], axis=1).astype(np.uint8),
            "user_data": v.astype(np.uint8), "point_source_id": (v * 257).astype(np.uint16), "intensity": (65535 - v * 256).astype(np.uint16)}
    names = tuple(cols)
    p = str(tmp_path / "bits.las")
    swz.las_write_node_rows(p, np.zeros((n, 3)), cols, *UNIT, 0.0001)
    data = open(p, "rb").read()
    assert data == _header(n, 2, *UNIT, 0.0001) + _records(np.zeros((n, 3)), cols, names, UNIT[0], 0.0001)
    rec = np.frombuffer(data[227:], _dtype(2))
    assert np.array_equal(rec["bits"] & 7, v & 7) and np.array_equal((rec["bits"] >> 3) & 7, v[::-1] & 7)     # three bits survive
    assert np.array_equal(rec["bits"] >> 6 & 1, (v // 2) & 1) and np.array_equal(rec["bits"] >> 7, v & 1)          # one bit
    assert np.array_equal(rec["classification"], v & 31)                                                           # five, flags zero
    assert np.array_equal(rec["scan_angle_rank"], v - 128)
    assert set(np.unique(rec["rgb"])) == {0, 256, 65280}
    # a column that is present but not named by the mask stays zero, like an untouched laszip_point
    swz.las_write_node_rows(p, np.zeros((n, 3)), cols, *UNIT, 0.0001, write=("rgb",))
    rec = np.frombuffer(open(p, "rb").read()[227:], _dtype(2))
    assert not rec["bits"].any() and not rec["classification"].any() and not rec["intensity"].any() and rec["rgb"].any()


def test_bad_arguments_of_the_writers_and_the_empty_node(tmp_path):
    import schwarzwald_amd as swz
    p = str(tmp_path / "x.las")
    one = np.zeros((1, 3))
    for kwargs in (dict(attrs={}, write=("rgb",)), dict(attrs={"rgb": np.zeros((1, 3), np.uint8)}, write=("rgb", "gps_time")),
                   dict(attrs={}, write=1 << 12)):
        with pytest.raises(swz.SwzError) as e:
            swz.las_write_node_rows(p, one, kwargs["attrs"], *UNIT, 0.001, write=kwargs["write"])
        assert e.value.code == ERR_BAD_ARG
    for scale in (0.0, -0.001, float("inf"), float("nan")):
        with pytest.raises(swz.SwzError):
            swz.las_write_node_rows(p, one, {}, *UNIT, scale)
        with pytest.raises(swz.SwzError):
            swz.las_write_node(p, 1, np.zeros(20, np.uint8), (), *UNIT, scale)
    with pytest.raises(swz.SwzError):
        swz.las_write_node_rows(p, one, {}, [0, float("nan"), 0], [1, 1, 1], 0.001)
    with pytest.raises(swz.SwzError):
        swz.las_write_node_rows(p, one, {}, [0, 0, 0], [1, float("inf"), 1], 0.001)
    assert not os.path.exists(p)
    swz.las_write_node_rows(p, one, {}, *UNIT, 0.001, write=("normal",))      # normals: accepted, dropped
    assert open(p, "rb").read() == _header(1, 0, *UNIT, 0.001) + bytes(20)
    os.remove(p)
    swz.las_write_node(str(tmp_path / "none.las"), 0, np.empty(0, np.uint8), (), *UNIT, 0.001)
    swz.las_write_node_rows(str(tmp_path / "none2.las"), np.empty((0, 3)), {}, *UNIT, 0.001)
    assert list(tmp_path.iterdir()) == []
    gone = str(tmp_path / "does" / "not" / "exist" / "r.las")
    with pytest.raises(swz.SwzError):
        swz.las_write_node_rows(gone, one, {}, *UNIT, 0.001)


# ------------------------------------------------------------------------------------------ CPU: the reader
_BITS = {"return_number": 7, "number_of_returns": 7, "classification": 31, "edge_of_flight_line": 1, "scan_direction_flag": 1}


def _stored(column, name, names):
    """what a reader gets back of a column: the bits the record keeps, zeros when the mask left it out"""
    if name not in names:
        return np.zeros_like(column)
    return column & np.uint8(_BITS[name]) if name in _BITS else column


@pytest.mark.parametrize("names", MASKS + [ALL])
def test_reader_round_trip_and_the_oracles_decoder(tmp_path, names):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(11)
    n = 500
    box_min, box_max = [-40.0, 10.0, 1000.0], [60.0, 110.0, 1100.0]
    xyz = np.asarray(box_min) + rng.random((n, 3)) * 100.0
    xyz[0], xyz[1] = box_min, box_max
    cols = _columns(rng, n)
    scale = swz.las_scale_from_bounds(box_min, box_max)
    p = str(tmp_path / "rt.las")
    swz.las_write_node_rows(p, xyz, cols, box_min, box_max, scale, write=names)
    head = swz.las_read_header(p)
    fmt = _format(names)
    assert head == dict(count=n, point_format=fmt, record_bytes=_dtype(fmt).itemsize, offset_to_point_data=227, scale=[scale] * 3,
                        offset=box_min, min=box_min, max=box_max)
    got_xyz, got = swz.las_read_node(p)
    # half a quantisation step, one rounding each in the quotient and in offset + X * scale
    tol = 0.5 * scale + 2 * np.spacing(np.abs(xyz).max())
    assert np.abs(got_xyz - xyz).max() <= tol
    assert got_xyz.min(axis=0).tolist() == box_min and got_xyz.max(axis=0).tolist() == box_max   # clamped into the header box
    assert ("gps_time" in got) == bool(fmt & 1) and ("rgb" in got) == bool(fmt & 2) and "normal" not in got
    for name, arr in got.items():
        want = _stored(cols[name], name, names)
        assert np.array_equal(arr, want), name
    # the same records through the checker's decoder (which tests/test_las_decode.py checks against hand-written records)
    data = open(p, "rb").read()
    o_xyz, o_attrs = O.las_decode(np.frombuffer(data[227:], np.uint8), n, head["scale"], head["offset"], head["min"], head["max"],
                                  head["point_format"], head["record_bytes"])
    assert np.array_equal(o_xyz, got_xyz)
    assert np.abs(o_xyz - xyz).max() <= tol
    for name, arr in o_attrs.items():
        want = _stored(cols[name], name, names)
        assert np.array_equal(arr, want), name


def test_reader_skips_vlr_bytes_and_extra_record_bytes(tmp_path):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(12)
    n = 7
    xyz = rng.random((n, 3))
    cols = _columns(rng, n)
    names = ("rgb", "intensity", "gps_time")
    body = np.frombuffer(_records(xyz, cols, names, UNIT[0], 0.0001), np.uint8).reshape(n, 34)
    wide = np.concatenate([body, np.full((n, 5), 0xEE, np.uint8)], axis=1).tobytes()       # 39-byte records: 5 extra bytes each
    head = bytearray(_header(n, 3, *UNIT, 0.0001, data_at=227 + 54))
    head[105:107] = struct.pack("<H", 39)
    head[100:104] = struct.pack("<I", 1)
    p = tmp_path / "vlr.las"
    p.write_bytes(bytes(head) + b"\xEE" * 54 + wide + b"\xEE" * 11)
    h = swz.las_read_header(str(p))
    assert h["offset_to_point_data"] == 281 and h["record_bytes"] == 39 and h["count"] == n
    got_xyz, got = swz.las_read_node(str(p))
    assert np.abs(got_xyz - xyz).max() <= 0.00005 + 1e-15
    assert np.array_equal(got["rgb"], cols["rgb"]) and np.array_equal(got["gps_time"], cols["gps_time"])
    assert np.array_equal(got["intensity"], cols["intensity"])


def test_reader_refuses_malformed_files(tmp_path):
    import schwarzwald_amd as swz
    n = 3
    body = bytes(range(1, 27)) * n
    good = _header(n, 2, *UNIT, 0.001) + body

    def patched(at, fmt, value):
        b = bytearray(good)
        b[at:at + struct.calcsize(fmt)] = struct.pack(fmt, value)
        return bytes(b)

    cases = {
        "good": good,
        "empty file": b"",
        "shorter than the signature": good[:3],
        "cut inside the header": good[:100],
        "header minus one byte": good[:226],
        "header only": good[:227],
        "cut inside the first record": good[:227 + 10],
        "cut inside the last record": good[:-1],
        "one record short": good[:-26],
        "wrong signature": b"LASX" + good[4:],
        "header size passes the file": patched(94, "<H", 60000),
        "header size below 227": patched(94, "<H", 100),
        "data offset passes the file": patched(96, "<I", len(good) + 1),
        "data offset huge": patched(96, "<I", 0xFFFFFFFF),
        "data offset inside the header": patched(96, "<I", 100),
        "data offset leaves too few bytes": patched(96, "<I", 228),
        "record length below the format's": patched(105, "<H", 25),
        "record length zero": patched(105, "<H", 0),
        "format 4": patched(104, "<B", 4),
        "format 6": patched(104, "<B", 6),
        "format 255": patched(104, "<B", 255),
        "count passes the end": patched(107, "<I", n + 1),
        "count huge": patched(107, "<I", 0xFFFFFFFF),
    }
    L = swz.load_library()
    for name, data in cases.items():
        p = tmp_path / "case.las"
        p.write_bytes(data)
        if name == "good":
            assert swz.las_read_node(str(p))[0].shape == (n, 3)
            continue
        with pytest.raises(swz.SwzError) as e:
            swz.las_read_header(str(p))
        assert e.value.code == ERR_BAD_ARG, name
        xyz = np.full((n, 3), 7.0)
        rgb = np.full((n, 3), 9, np.uint8)
        cols = swz.api._AttributeColumns()
        cols.column[0] = rgb.ctypes.data
        assert L.swz_las_read_node(None, str(p).encode(), xyz.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cols)) == ERR_BAD_ARG, name
        assert np.all(xyz == 7.0) and np.all(rgb == 9), name
        count, fmt = C.c_uint64(77), C.c_uint32(77)
        assert L.swz_las_read_header(None, str(p).encode(), C.byref(count), C.byref(fmt), None, None, None) == ERR_BAD_ARG, name
        assert count.value == 77 and fmt.value == 77, name
    with pytest.raises(swz.SwzError):
        swz.las_read_node(str(tmp_path / "missing.las"))


def test_refused_format_names_the_device_decoder(tmp_path):
    import schwarzwald_amd as swz
    L = swz.load_library()
    data = bytearray(_header(1, 0, *UNIT, 0.001) + bytes(40))
    data[104] = 7
    p = tmp_path / "f7.las"
    p.write_bytes(bytes(data))
    # the text of a failure is kept in a context; without one only the code comes back, so look for the text in the library
    lib_bytes = open(swz.library_path(), "rb").read()
    assert b"swz_las_decode_device decodes the others" in lib_bytes
    assert L.swz_las_read_header(None, str(p).encode(), None, None, None, None, None) == ERR_BAD_ARG


# ------------------------------------------------------------------------------------------ CPU: Entwine
def _key(digits):
    key = 0
    for l, ch in enumerate(digits):
        key |= int(ch) << (3 * (20 - l))
    return len(digits) - 1, key


def _entwine(digits):
    x = y = z = 0
    for ch in digits:
        o = int(ch)
        x, y, z = x * 2 + (o >> 2 & 1), y * 2 + (o >> 1 & 1), z * 2 + (o & 1)
    return "%d-%d-%d-%d" % (len(digits), x, y, z)


def test_entwine_names_of_this_test_are_the_librarys():
    import schwarzwald_amd as swz
    for digits in ("", "0", "7", "3041", "30412", "3041265710", "30412657101"):
        assert swz.node_name_entwine(*_key(digits)) == _entwine(digits)


def test_hierarchy_files_split_every_five_levels(tmp_path):
    import schwarzwald_amd as swz
    # depths 0, 1, 4, 5, 6, 10, 11; the depth-10 node under 7... has no depth-5 ancestor in the table; "12" has count 0
    table = {"": 100, "3": 11, "3041": 12, "30412": 13, "304126": 14, "3041265710": 15, "30412657101": 16, "7654321076": 17, "12": 0,
             "30413": 18}
    level, key = zip(*[_key(d) for d in table])
    swz.ept_create_dirs(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["ept-data", "ept-hierarchy", "ept-sources"]
    swz.ept_create_dirs(str(tmp_path))       # existing directories are kept
    swz.ept_hierarchy_write(str(tmp_path), dict(level=level, key=key, count=list(table.values())))
    E = _entwine
    want = {
        "0-0-0-0.json": {E(""): 100, E("3"): 11, E("3041"): 12, E("30412"): -1, E("76543"): -1, E("30413"): -1},
        E("30412") + ".json": {E("30412"): 13, E("304126"): 14, E("3041265710"): -1},
        E("30413") + ".json": {E("30413"): 18},
        E("3041265710") + ".json": {E("3041265710"): 15, E("30412657101"): 16},
        E("76543") + ".json": {E("7654321076"): -1},
        E("7654321076") + ".json": {E("7654321076"): 17},
    }
    got = {f: json.loads((tmp_path / "ept-hierarchy" / f).read_text()) for f in os.listdir(tmp_path / "ept-hierarchy")}
    assert got == want
    for f in got:
        text = (tmp_path / "ept-hierarchy" / f).read_text()
        assert " " not in text and "\n" not in text
    assert sum(v for g in got.values() for v in g.values() if v > 0) == sum(table.values())
    # nothing but empty nodes: no file at all; a missing directory is an error
    swz.ept_create_dirs(str(tmp_path / "e2"))
    swz.ept_hierarchy_write(str(tmp_path / "e2"), dict(level=[0], key=[0], count=[0]))
    assert os.listdir(tmp_path / "e2" / "ept-hierarchy") == []
    with pytest.raises(swz.SwzError):
        swz.ept_hierarchy_write(str(tmp_path / "nowhere"), dict(level=[-1], key=[0], count=[1]))
    with pytest.raises(swz.SwzError):
        swz.ept_hierarchy_write(str(tmp_path), dict(level=[21], key=[0], count=[1]))


def test_ept_json_member_by_member(tmp_path):
    import schwarzwald_amd as swz
    p = tmp_path / "ept.json"
    bounds = ([-0.1, 1 / 3, 4.5e6 + 1e-9], [1e21, 2.5, 5e6])
    conforming = ([0.0, 0.5, 4.6e6], [123456789.125, 2.0, 4.9e6])
    srs = {"authority": "EPSG", "horizontal": "25832", "wkt": 'PROJCS["ETRS89 / UTM",\n\tUNIT["metre",1]] \\ end'}
    swz.ept_json_write(str(p), bounds, conforming, 123456789012, ALL + ("normal",), 128.0, srs, "1.0.0")
    text = p.read_text()
    doc = json.loads(text)
    assert list(doc) == ["bounds", "boundsConforming", "dataType", "hierarchyType", "points", "schema", "span", "srs", "version"]
    assert doc["bounds"] == bounds[0] + bounds[1] and doc["boundsConforming"] == conforming[0] + conforming[1]
    assert doc["dataType"] == "las" and doc["hierarchyType"] == "json" and doc["points"] == 123456789012
    assert doc["span"] == 128 and doc["srs"] == srs and list(doc["srs"]) == ["authority", "horizontal", "wkt"] and doc["version"] == "1.0.0"
    u = lambda name, size: {"name": name, "size": size, "type": "unsigned"}
    assert doc["schema"] == [
        {"name": "X", "size": 4, "type": "signed", "offset": 0, "scale": 1}, {"name": "Y", "size": 4, "type": "signed", "offset": 0, "scale": 1},
        {"name": "Z", "size": 4, "type": "signed", "offset": 0, "scale": 1}, u("Red", 2), u("Green", 2), u("Blue", 2),
        {"name": "NX", "size": 4, "type": "float"}, {"name": "NY", "size": 4, "type": "float"}, {"name": "NZ", "size": 4, "type": "float"},
        u("Intensity", 2), u("Classification", 1), u("EdgeOfFlightLine", 1), {"name": "GpsTime", "size": 8, "type": "float"},
        u("NumberOfReturns", 1), u("ReturnNumber", 1), u("PointSourceID", 2), u("ScanDirectionFlag", 1),
        {"name": "ScanAngleRank", "size": 1, "type": "signed"}, u("UserData", 1)]
    assert " " not in text[:text.index('"srs"')] and "\n" not in text           # compact
    swz.ept_json_write(str(p), UNIT, UNIT, 0)
    doc = json.loads(p.read_text())
    assert [e["name"] for e in doc["schema"]] == ["X", "Y", "Z"] and doc["srs"] == {"authority": "", "horizontal": "", "wkt": ""}
    assert doc["version"] == "" and doc["points"] == 0 and doc["span"] == 0
    with pytest.raises(swz.SwzError):
        swz.ept_json_write(str(p), ([0, 0, float("nan")], [1, 1, 1]), UNIT, 0)
    with pytest.raises(swz.SwzError):
        swz.ept_json_write(str(tmp_path / "no" / "dir" / "ept.json"), UNIT, UNIT, 0)


def test_persist_nodes_names_and_files_without_a_device(tmp_path):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(13)
    digits = ["", "3", "30", "301"]
    counts = np.array([5, 0, 2, 3], np.uint64)
    level, key = zip(*[_key(d) for d in digits])
    nodes = dict(level=level, key=key, count=counts)
    names = ("rgb", "intensity")
    boxes = [swz.node_bounds(l, k, *UNIT) for l, k in zip(level, key)]
    mn, mx = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
    scales = np.array([swz.las_scale_from_bounds(a, b) for a, b in zip(mn, mx)])
    assert set(scales) == {0.001, 0.0001}
    lay = swz.las_image_layout(counts, names)
    image = np.full(lay["total"], 0xA5, np.uint8)
    rows = {}
    for k, c in enumerate(counts):
        c = int(c)
        xyz, cols = rng.random((c, 3)), _columns(rng, c)
        rows[k] = (xyz, cols)
        body = _records(xyz, cols, names, mn[k], scales[k])
        image[int(lay["offset"][k]):int(lay["offset"][k]) + len(body)] = np.frombuffer(body, np.uint8)
    for naming, want_names in ((swz.LAS_NAMING_POTREE, ["r.las", "r30.las", "r301.las"]),
                               (swz.LAS_NAMING_ENTWINE, [_entwine(d) + ".las" for d in ("", "30", "301")])):
        d = tmp_path / str(naming)
        d.mkdir()
        swz.las_persist_nodes(str(d), nodes, image, names, mn, mx, scales, naming)
        assert sorted(os.listdir(d)) == sorted(want_names)
        for f, k in zip(want_names, (0, 2, 3)):
            xyz, cols = rows[k]
            assert (d / f).read_bytes() == _header(int(counts[k]), 2, mn[k], mx[k], scales[k]) + _records(xyz, cols, names, mn[k], scales[k])
    with pytest.raises(swz.SwzError):
        swz.las_persist_nodes(str(tmp_path), nodes, image[:-8], names, mn, mx, scales)
    with pytest.raises(swz.SwzError):
        swz.las_persist_nodes(str(tmp_path), nodes, image, names, mn, mx, scales, naming=2)
    with pytest.raises(swz.SwzError):
        swz.las_persist_nodes(str(tmp_path), nodes, image, names, mn, mx, scales * 0)


# ------------------------------------------------------------------------------------------ GPU: the pack kernel
GUARD = 4096


def _image(counts, offsets, scales, las_off, rows, xyz, cols, names):
    parts = []
    for k, (c, o) in enumerate(zip(counts, offsets)):
        r = rows[int(o):int(o + c)]
        body = _records(xyz[r], {a: v[r] for a, v in cols.items()}, names, las_off[k], scales[k]) if c else b""
        parts.append(body + bytes(-len(body) % 8))
    return b"".join(parts)


@pytest.fixture(scope="module")
def source():
    """Source rows on the device, shared by the pack tests: more rows than any test lists, hard positions up front."""
    import torch
    import schwarzwald_amd as swz
    tile = swz.las_pack_tile()
    rng = np.random.default_rng(21)
    src = 8 * tile
    xyz = _hard_positions(rng, src)
    cols = _columns(rng, src)
    dev = torch.device("cuda:0")
    d = {"xyz": torch.from_numpy(xyz).to(dev)}
    for name, arr in cols.items():
        flat = np.ascontiguousarray(arr)
        d[name] = torch.from_numpy(flat.view(np.uint8).reshape(-1)).to(dev)
    torch.cuda.synchronize()
    return dict(tile=tile, src=src, xyz=xyz, cols=cols, d=d, rng=rng)


def _pack_and_compare(ctx, S, counts, offsets, n, names, perm, order, scales, las_off, xyz=None, d_xyz=None):
    import torch
    import schwarzwald_amd as swz
    xyz = S["xyz"] if xyz is None else xyz
    d_xyz = S["d"]["xyz"] if d_xyz is None else d_xyz
    rows = perm[order] if order is not None else perm
    want = _image(counts, offsets, scales, las_off, rows, xyz, S["cols"], names)
    total = swz.las_image_layout(counts, names)["total"]
    assert len(want) == total
    d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda:0")
    d_order = torch.from_numpy(order.view(np.int32)).to("cuda:0") if order is not None else None
    buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    attrs = {a: S["d"][a].data_ptr() for a in names}
    ctx.las_pack_device(d_perm.data_ptr(), d_order.data_ptr() if order is not None else None, n, d_xyz.data_ptr(), attrs,
                        dict(offset=offsets, count=counts), las_off, scales, buf.data_ptr() + GUARD, total, attrs=names)
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + total:] == 0xA5), names
    image = got[GUARD:GUARD + total].tobytes()
    if image != want:
        bad = np.flatnonzero(np.frombuffer(image, np.uint8) != np.frombuffer(want, np.uint8))
        lay = swz.las_image_layout(counts, names)
        k = int(np.searchsorted(lay["offset"], bad[0], side="right") - 1)
        pytest.fail("mask %s: %d bytes differ, first at %d = node %d (count %d, rows from %d) + %d"
                    % (names, len(bad), bad[0], k, counts[k], offsets[k], bad[0] - lay["offset"][k]))


def _node_params(rng, m):
    """offsets and scales that differ between neighbouring nodes"""
    scales = np.resize([0.001, 0.5, 0.0001, 0.25, 0.01], m).astype(np.float64)
    las_off = (rng.random((m, 3)) - 0.5) * 100.0
    return scales, las_off


@pytest.mark.gpu
@pytest.mark.parametrize("names", MASKS + [ALL])
def test_gpu_pack_one_node_of_every_edge_size(source, names):
    import schwarzwald_amd as swz
    S = source
    T = S["tile"]
    rng = np.random.default_rng(22)
    with swz.Context(0) as ctx:
        for n in (1, T - 1, T, T + 1, 3 * T + 5):
            counts, offsets = np.array([n], np.uint64), np.array([0], np.uint64)
            perm = rng.permutation(S["src"]).astype(np.uint32)[:n]
            scales, las_off = _node_params(rng, 1)
            _pack_and_compare(ctx, S, counts, offsets, n, names, perm, rng.permutation(n).astype(np.uint32), scales, las_off)
            _pack_and_compare(ctx, S, counts, offsets, n, names, perm, None, scales, las_off)


def _mixed_table(T):
    """nodes of 1, 2 and 3 points around one of 2 T + 1 that spans three blocks, gaps of unlisted rows between nodes and
    behind the last, empty nodes, node boundaries at and next to block edges"""
    counts, offsets = [], []
    at = 3                                   # rows in front of the first node
    for c in [1, 2, 3, 1, 0, 2] * 6 + [2 * T + 1] + [3, 2, 1] * 4 + [0, T - 7, 1, 1, T, 2]:
        counts.append(c)
        offsets.append(at)
        at += c + (2 if len(counts) % 5 == 0 else 0)
    return np.array(counts, np.uint64), np.array(offsets, np.uint64), at + 9


@pytest.mark.gpu
@pytest.mark.parametrize("names", MASKS + [ALL])
@pytest.mark.parametrize("with_order", [True, False])
def test_gpu_pack_mixed_table_with_gaps(source, names, with_order):
    import schwarzwald_amd as swz
    S = source
    T = S["tile"]
    rng = np.random.default_rng(23)
    counts, offsets, n = _mixed_table(T)
    assert n <= S["src"] and counts.max() == 2 * T + 1
    perm = rng.permutation(S["src"]).astype(np.uint32)[:n]
    order = rng.permutation(n).astype(np.uint32) if with_order else None
    scales, las_off = _node_params(rng, len(counts))
    with swz.Context(0) as ctx:
        _pack_and_compare(ctx, S, counts, offsets, n, names, perm, order, scales, las_off)


@pytest.mark.gpu
@pytest.mark.parametrize("names", [MASKS[0], MASKS[3]])
def test_gpu_pack_tiles_of_one_point_nodes(source, names):
    """Every row a node of its own: 40 bytes of image per 34-byte record, more than one pass of a block's staging."""
    import schwarzwald_amd as swz
    S = source
    T = S["tile"]
    rng = np.random.default_rng(24)
    n = 2 * T + 3
    counts = np.ones(n, np.uint64)
    counts[T // 2:T // 2 + 9] = 2
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    n = int(counts.sum())
    perm = rng.permutation(S["src"]).astype(np.uint32)[:n]
    scales, las_off = _node_params(rng, len(counts))
    with swz.Context(0) as ctx:
        _pack_and_compare(ctx, S, counts, offsets, n, names, perm, None, scales, las_off)


@pytest.mark.gpu
@pytest.mark.parametrize("names", MASKS)
def test_gpu_pack_hard_quantisation_values_at_tile_edges(source, names):
    import torch
    import schwarzwald_amd as swz
    S = source
    T = S["tile"]
    n = 2 * T
    q = _hard_quotients()
    with swz.Context(0) as ctx:
        for scale in (0.5, 0.25):
            hard = _hard_xyz(scale)
            xyz = S["xyz"][:n].copy()
            for i, row in enumerate(hard):        # first and last rows of both tiles, in turn
                xyz[[0, T - 1, T, 2 * T - 1][i % 4] + (i // 4) * (1 if i % 4 in (0, 2) else -1)] = row
            d_xyz = torch.from_numpy(xyz).to("cuda:0")
            counts, offsets = np.array([T + 3, T - 3], np.uint64), np.array([0, T + 3], np.uint64)
            scales, las_off = np.array([scale, scale]), np.zeros((2, 3))
            _pack_and_compare(ctx, S, counts, offsets, n, names, np.arange(n, dtype=np.uint32), None, scales, las_off, xyz=xyz, d_xyz=d_xyz)
    assert len(q) <= 2 * T


@pytest.mark.gpu
def test_gpu_pack_refuses_before_anything_is_launched(source):
    import torch
    import schwarzwald_amd as swz
    S = source
    d = S["d"]
    n = S["src"]
    u = lambda *v: np.array(v, dtype=np.uint64)
    both = {"rgb": d["rgb"].data_ptr(), "gps_time": d["gps_time"].data_ptr()}
    good = dict(offset=u(0, 10), count=u(10, 5))
    sc, off = np.array([0.001, 0.001]), np.zeros((2, 3))
    bad_off = off.copy()
    bad_off[1, 2] = np.inf
    nan_off = off.copy()
    nan_off[0, 0] = np.nan
    cases = [
        ("offsets not ascending", dict(offset=u(10, 0), count=u(5, 10)), both, ("rgb",), n, sc, off),
        ("ranges overlap", dict(offset=u(0, 9), count=u(10, 5)), both, ("rgb",), n, sc, off),
        ("range passes n", dict(offset=u(0, n - 2), count=u(10, 3)), both, ("rgb",), n, sc, off),
        ("offset passes n", dict(offset=u(0, n + 1), count=u(10, 1)), both, ("rgb",), n, sc, off),
        ("count wraps around", dict(offset=u(0, 16), count=u(10, 2 ** 64 - 8)), both, ("rgb",), n, sc, off),
        ("mask names absent rgb", good, {"gps_time": d["gps_time"].data_ptr()}, ("rgb",), n, sc, off),
        ("mask names absent intensity", good, both, ("rgb", "intensity"), n, sc, off),
        ("unknown mask bit", good, both, 1 << 12, n, sc, off),
        ("n above the limit", good, both, ("rgb",), 2 ** 32 - 65535, sc, off),
        ("scale zero", good, both, ("rgb",), n, np.array([0.001, 0.0]), off),
        ("scale negative", good, both, ("rgb",), n, np.array([-0.001, 0.001]), off),
        ("scale infinite", good, both, ("rgb",), n, np.array([0.001, np.inf]), off),
        ("scale NaN", good, both, ("rgb",), n, np.array([np.nan, 0.001]), off),
        ("offset infinite", good, both, ("rgb",), n, sc, bad_off),
        ("offset NaN", good, both, ("rgb",), n, sc, nan_off),
    ]
    perm = torch.arange(n, dtype=torch.int32, device="cuda:0")
    with swz.Context(0) as ctx:
        buf = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        for name, nodes, attrs, mask, rows, scales, las_off in cases:
            with pytest.raises(swz.SwzError) as e:
                ctx.las_pack_device(perm.data_ptr(), None, rows, d["xyz"].data_ptr(), attrs, nodes, las_off, scales, buf.data_ptr(), 1 << 16,
                                    attrs=mask)
            assert e.value.code == ERR_BAD_ARG, name
        with pytest.raises(swz.SwzError) as e:   # an image buffer smaller than the layout: 15 records of 26 bytes
            ctx.las_pack_device(perm.data_ptr(), None, n, d["xyz"].data_ptr(), both, good, off, sc, buf.data_ptr(), 399, attrs=("rgb",))
        assert e.value.code == ERR_BAD_ARG
        # nothing to do: no nodes, n == 0, only empty nodes
        empty = dict(offset=np.empty(0, np.uint64), count=np.empty(0, np.uint64))
        ctx.las_pack_device(perm.data_ptr(), None, n, d["xyz"].data_ptr(), both, empty, np.empty((0, 3)), np.empty(0), buf.data_ptr(), 1 << 16,
                            attrs=("rgb",))
        ctx.las_pack_device(None, None, 0, None, both, empty, np.empty((0, 3)), np.empty(0), None, 0, attrs=("rgb",))
        ctx.las_pack_device(perm.data_ptr(), None, n, d["xyz"].data_ptr(), both, dict(offset=u(5, 9), count=u(0, 0)), off, sc, buf.data_ptr(),
                            1 << 16, attrs=("rgb",))
        torch.cuda.synchronize()
        assert np.all(buf.cpu().numpy() == 0xA5)


# ------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_gpu_entwine_output_holds_the_rows_the_oracle_assigns(tmp_path):
    import torch
    import schwarzwald_amd as swz
    rng = np.random.default_rng(31)
    n = 20_000
    xyz = rng.random((n, 3))
    cols = _columns(rng, n)
    names = ("rgb", "intensity", "gps_time")
    spacing = O.spacing_from_diagonal(*UNIT, 16)
    o = O.tile(xyz, *UNIT, O.GRID_CENTER, 500, spacing)
    assert o["status"] == 0
    want = _oracle_node_rows(o)
    assert len(want) == 73
    d_pack, d_host = tmp_path / "pack", tmp_path / "host"
    swz.ept_create_dirs(str(d_pack))
    swz.ept_create_dirs(str(d_host))

    dev = torch.device("cuda:0")
    with swz.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        d_xyz = torch.from_numpy(xyz).to(dev)
        d_attr = {a: torch.from_numpy(np.ascontiguousarray(cols[a]).view(np.uint8).reshape(-1)).to(dev) for a in names}
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        level = torch.empty(n, dtype=torch.int8, device=dev)
        ctx.tile_device(d_xyz.data_ptr(), n, *UNIT, swz.TileParams(sampler=swz.GRID_CENTER, max_points_per_node=500, spacing_at_root=spacing),
                        keys.data_ptr(), perm.data_ptr(), level.data_ptr())
        order = torch.empty(n, dtype=torch.int32, device=dev)
        nodes = ctx.build_node_lists_device(keys.data_ptr(), level.data_ptr(), n, order.data_ptr())
        boxes = [swz.node_bounds(int(l), int(k), *UNIT) for l, k in zip(nodes["level"], nodes["key"])]
        mn, mx = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
        scales = np.array([swz.las_scale_from_bounds(a, b) for a, b in zip(mn, mx)])
        total = swz.las_image_layout(nodes["count"], names)["total"]
        image = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
        ctx.las_pack_device(perm.data_ptr(), order.data_ptr(), n, d_xyz.data_ptr(), {a: t.data_ptr() for a, t in d_attr.items()}, nodes,
                            mn, scales, image.data_ptr(), total, attrs=names)
        ctx.las_persist_nodes(str(d_pack / "ept-data"), nodes, image.cpu().numpy(), names, mn, mx, scales, swz.LAS_NAMING_ENTWINE)
    swz.ept_hierarchy_write(str(d_pack), nodes)

    # the expectation: the oracle's rows of every node through the host writer, the hierarchy from their counts
    w_level, w_key = [], []
    for name, rows in want.items():
        lv, key = _key(name[1:])
        w_level.append(lv)
        w_key.append(key)
        b_min, b_max = swz.node_bounds(lv, key, *UNIT)
        swz.las_write_node_rows(str(d_host / "ept-data" / (swz.node_name_entwine(lv, key) + ".las")), xyz[rows],
                                {a: cols[a][rows] for a in names}, b_min, b_max, swz.las_scale_from_bounds(b_min, b_max))
    swz.ept_hierarchy_write(str(d_host), dict(level=w_level, key=w_key, count=[len(r) for r in want.values()]))
    got = sorted(os.listdir(d_pack / "ept-data"))
    assert got == sorted(os.listdir(d_host / "ept-data")) and len(got) == 73
    for f in got:
        assert (d_pack / "ept-data" / f).read_bytes() == (d_host / "ept-data" / f).read_bytes(), f
    hier = sorted(os.listdir(d_pack / "ept-hierarchy"))
    assert hier == sorted(os.listdir(d_host / "ept-hierarchy")) == ["0-0-0-0.json"]
    total_points = 0
    for f in hier:
        a, b = json.loads((d_pack / "ept-hierarchy" / f).read_text()), json.loads((d_host / "ept-hierarchy" / f).read_text())
        assert a == b
        total_points += sum(v for v in a.values() if v > 0)
    assert total_points == n
    # and one file read back: the root's points within half a step of the input
    r_xyz, r_attrs = swz.las_read_node(str(d_pack / "ept-data" / "0-0-0-0.las"))
    rows = want["r"]
    assert np.abs(r_xyz - xyz[rows]).max() <= 0.5 * 0.001 + 2 * np.spacing(1.0)
    assert np.array_equal(r_attrs["rgb"], cols["rgb"][rows]) and np.array_equal(r_attrs["gps_time"], cols["gps_time"][rows])
