"""The host side of reading a data set of LAS files (swz_las_scan_files, swz_input_batches): headers of LAS 1.2 - 1.4
written here with numpy, the data set's boxes against a numpy restatement of AABB::makeCubic / getCenter
(core/math/AABB.h:50-70, core/pointcloud/FileStats.cpp:30-37), the common attributes against las_file_has_attribute
(core/io/LASFile.cpp:415-445) worked out by hand, every refusal.  No GPU."""
import os

import numpy as np
import pytest

import schwarzwald_amd as swz
from las_input_util import HEADER_SIZE, LasTile, make_cubic, vlr, write_las
from test_las_decode import SIZES

ALWAYS = {"intensity", "classification", "edge_of_flight_line", "number_of_returns", "return_number", "point_source_id",
          "scan_direction_flag", "scan_angle_rank", "user_data"}
# UTM-sized offsets: the boxes are compared bit for bit, so the order of the operations matters there
UTM = [(412345.678, 5401234.321, 287.125), (413345.681, 5400234.117, 301.5), (411345.003, 5402234.9, 150.062)]


def _tiles(rng):
    specs = [dict(n=7, fmt=0, minor=2), dict(n=5, fmt=1, minor=2, extra=1, vlrs=[vlr("LASF_Projection", 34735, b"x" * 24)]),
             dict(n=3, fmt=2, minor=3), dict(n=9, fmt=3, minor=3, extra=1, vlrs=[vlr("abc", 1, b"y" * 7)]),
             dict(n=4, fmt=6, minor=4), dict(n=6, fmt=7, minor=4, extra=3), dict(n=2, fmt=8, minor=4, vlrs=[vlr("q", 2, b"")])]
    tiles = []
    for i, s in enumerate(specs):
        off = UTM[i % 3]
        tiles.append(LasTile(rng, s["n"], s["fmt"], extra=s.get("extra", 0), minor=s["minor"], scale=(0.001, 0.001, 0.01),
                             offset=off, lo=-5000 * (i + 1), hi=70000 * (i + 2), vlrs=s.get("vlrs", ())))
    return tiles


def test_scan_headers_of_every_version_and_format(tmp_path):
    rng = np.random.default_rng(1)
    tiles = _tiles(rng)
    paths = [t.write(tmp_path / ("t%d.las" % i)) for i, t in enumerate(tiles)]
    files, ds = swz.las_scan_files(paths)
    odd_offsets = 0
    for t, f in zip(tiles, files):
        assert f["status"] == swz.LAS_FILE_OK
        assert f["count"] == t.n
        assert f["point_format"] == t.fmt and f["record_bytes"] == SIZES[t.fmt] + t.extra
        assert f["offset_to_point_data"] == HEADER_SIZE[t.minor] + sum(len(v) for v in t.vlrs) == t.data_offset
        odd_offsets += f["offset_to_point_data"] & 1
        assert f["scale"] == t.scale and f["offset"] == t.offset and f["min"] == t.bmin and f["max"] == t.bmax
        want = set(ALWAYS)
        if t.fmt in (2, 3, 5, 7, 8, 10):
            want.add("rgb")
        if t.fmt in (1, 3):   # as las_file_has_attribute is written: the LAS 1.4 formats are not credited with GPS time
            want.add("gps_time")
        assert set(f["attrs"]) == want
    assert odd_offsets >= 3 and any(f["record_bytes"] & 1 for f in files)
    assert ds["total_points"] == sum(t.n for t in tiles) and ds["readable_files"] == len(tiles)
    tmin = np.min([t.bmin for t in tiles], axis=0)
    tmax = np.max([t.bmax for t in tiles], axis=0)
    cubic, origin, center = make_cubic(tmin, tmax)
    for got, want in ((ds["tight"], (tmin, tmax)), (ds["cubic"], cubic), (ds["origin"], origin)):
        for g, w in zip(got, want):
            assert g.tobytes() == np.asarray(w, np.float64).tobytes()
    assert ds["center"].tobytes() == center.tobytes()
    assert set(ds["attrs"]) == ALWAYS   # format 0 is among them


def test_extended_point_count(tmp_path):
    rng = np.random.default_rng(2)
    t = LasTile(rng, 11, 6)
    a = str(tmp_path / "a.las")
    # format 6: the legacy count says 3, the extended one the truth
    write_las(a, t.records, 6, t.scale, t.offset, t.bmin, t.bmax, minor=4, legacy_count=3)
    # LAS 1.4 with a legacy format: legacy count 0 -> the extended count; legacy count set -> the legacy count
    u = LasTile(rng, 11, 1, minor=4)
    b, c = str(tmp_path / "b.las"), str(tmp_path / "c.las")
    write_las(b, u.records, 1, u.scale, u.offset, u.bmin, u.bmax, minor=4, legacy_count=0)
    write_las(c, u.records, 1, u.scale, u.offset, u.bmin, u.bmax, minor=4, legacy_count=9, extended_count=11)
    files, ds = swz.las_scan_files([a, b, c])
    assert [f["count"] for f in files] == [11, 11, 9]
    assert ds["total_points"] == 31


@pytest.mark.parametrize("fmts,want", [((1, 2), set()), ((1, 3), {"gps_time"}), ((2, 3, 7), {"rgb"}), ((3, 3), {"rgb", "gps_time"}),
                                       ((3, 8), {"rgb"}), ((1, 6), set()), ((5, 10), {"rgb"}), ((0, 3), set())])
def test_common_attribute_mask(tmp_path, fmts, want):
    rng = np.random.default_rng(3)
    paths = [LasTile(rng, 2, f).write(tmp_path / ("f%d.las" % i)) for i, f in enumerate(fmts)]
    _, ds = swz.las_scan_files(paths)
    assert set(ds["attrs"]) == ALWAYS | want
    assert "normal" not in ds["attrs"]


def _good(tmp_path, **kw):
    t = LasTile(np.random.default_rng(4), 10, kw.pop("fmt", 1))
    p = str(tmp_path / "src.las")
    write_las(p, t.records, t.fmt, t.scale, t.offset, t.bmin, t.bmax, **kw)
    return open(p, "rb").read(), t


def test_refusals(tmp_path):
    # (the text of a refusal, which names the file, needs a context to be read back: tests/test_las_input_gpu.py)
    seen = {}

    def scan_error(path):
        L = swz.load_library()
        import ctypes as C
        arr = (C.c_char_p * 1)(os.fsencode(path))
        ds = swz.api._LasDataset()
        return L.swz_las_scan_files(None, arr, 1, 0, None, C.byref(ds))

    def refused(name, data, status):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        assert scan_error(p) == swz.api.ERR_BAD_ARG, name
        good = LasTile(np.random.default_rng(9), 3, 0).write(tmp_path / ("good_" + name))
        files, ds = swz.las_scan_files([good, p], skip_unreadable=True)
        assert files[1]["count"] == 0 and files[1]["status"] == status, (name, files[1]["status"])
        assert ds["total_points"] == 3 and ds["readable_files"] == 1
        seen[name] = status

    data, t = _good(tmp_path)
    rb = t.record_bytes
    refused("short.las", data[:200], swz.LAS_FILE_BAD_HEADER)
    refused("signature.las", b"LASX" + data[4:], swz.LAS_FILE_BAD_HEADER)
    bad = bytearray(data); bad[104] = 11
    refused("format11.las", bytes(bad), swz.LAS_FILE_BAD_HEADER)
    bad = bytearray(data); bad[105:107] = (rb - 1).to_bytes(2, "little")
    refused("record_short.las", bytes(bad), swz.LAS_FILE_BAD_HEADER)
    bad = bytearray(data); bad[96:100] = (len(data) + 1).to_bytes(4, "little")
    refused("data_offset.las", bytes(bad), swz.LAS_FILE_BAD_HEADER)
    refused("truncated.las", data[:-1], swz.LAS_FILE_BAD_HEADER)           # count x record length passes the end by one byte
    bad = bytearray(data); bad[104] |= 0x80
    refused("laz_bit.las", bytes(bad), swz.LAS_FILE_COMPRESSED)
    data_vlr, _ = _good(tmp_path, vlrs=[vlr("other", 7, b"zz"), vlr("laszip encoded", 22204, b"\0" * 34)])
    refused("laz_vlr.las", data_vlr, swz.LAS_FILE_COMPRESSED)
    data14, _ = _good(tmp_path, fmt=6, minor=4)
    bad = bytearray(data14); bad[94:96] = (227).to_bytes(2, "little")     # a 1.4 file whose header would end before its count
    refused("header14.las", bytes(bad), swz.LAS_FILE_BAD_HEADER)
    assert scan_error(str(tmp_path / "missing.las")) == swz.api.ERR_BAD_ARG
    files, _ = swz.las_scan_files([LasTile(np.random.default_rng(9), 3, 0).write(tmp_path / "g.las"), str(tmp_path / "missing.las")],
                                  skip_unreadable=True)
    assert files[1]["status"] == swz.LAS_FILE_UNREADABLE
    assert len(seen) == 9


def test_truncated_file_is_refused_without_a_read_outside_it(tmp_path):
    """A header that promises more than the file holds: the scan answers from the file's size, and a file cut inside its
    VLRs or right behind its header is read no further than it goes (a read past the end would fail the scan with another
    status, or fault under the page boundary of a mapping; pread returns short instead and the scan stops there)."""
    data, t = _good(tmp_path, vlrs=[vlr("a", 1, b"p" * 100), vlr("b", 2, b"q" * 100)])
    import ctypes as C
    L = swz.load_library()
    for cut in (227, 227 + 30, 227 + 54 + 100 + 10, len(data) - t.record_bytes):
        p = str(tmp_path / ("cut%d.las" % cut))
        with open(p, "wb") as f:
            f.write(data[:cut])
        ds = swz.api._LasDataset()
        info = (swz.api._LasFileInfo * 1)()
        assert L.swz_las_scan_files(None, (C.c_char_p * 1)(os.fsencode(p)), 1, 0, info, C.byref(ds)) == swz.api.ERR_BAD_ARG
        assert L.swz_las_scan_files(None, (C.c_char_p * 1)(os.fsencode(p)), 1, swz.LAS_SCAN_SKIP_UNREADABLE, info, C.byref(ds)) \
            == swz.api.ERR_BAD_ARG   # ... and with nothing else in the list there are no points to process
        assert info[0].status == swz.LAS_FILE_BAD_HEADER and info[0].point_count == 0


def test_no_points_is_refused(tmp_path):
    t = LasTile(np.random.default_rng(5), 0, 0)
    p = t.write(tmp_path / "empty.las")
    with pytest.raises(swz.SwzError):
        swz.las_scan_files([p])
    with pytest.raises(swz.SwzError):
        swz.las_scan_files([])
    # an empty file beside one with points is read, and its box counts (DatasetMetadata::add_file_metadata)
    u = LasTile(np.random.default_rng(5), 4, 0, lo=2 ** 21, hi=2 ** 22)
    files, ds = swz.las_scan_files([p, u.write(tmp_path / "u.las")])
    assert [f["count"] for f in files] == [0, 4] and ds["readable_files"] == 2
    assert ds["tight"][0].tolist() == t.bmin and ds["tight"][1].tolist() == u.bmax


def test_input_batches():
    assert swz.input_batches([10, 10, 10], 10).tolist() == [0, 10, 20, 30]           # exact multiples
    assert swz.input_batches([30], 10).tolist() == [0, 10, 20, 30]
    assert swz.input_batches([7, 0, 0, 9, 0, 8], 10).tolist() == [0, 10, 20, 24]    # empty files in the list, cuts mid-file
    assert swz.input_batches([7, 9, 8], 10, min_last=4).tolist() == [0, 10, 20, 24]  # a tail of min_last points stays
    assert swz.input_batches([7, 9, 8], 10, min_last=5).tolist() == [0, 10, 24]      # a shorter one is folded
    assert swz.input_batches([7, 9, 8], 100, min_last=24).tolist() == [0, 24]
    assert swz.input_batches([3], 10, min_last=0).tolist() == [0, 3]
    assert swz.input_batches([0, 0], 10).tolist() == [0]
    with pytest.raises(swz.SwzError):
        swz.input_batches([7, 9, 8], 100, min_last=25)                               # a data set below min_last
    with pytest.raises(swz.SwzError):
        swz.input_batches([7], 0)
    import ctypes as C
    L = swz.load_library()
    cnt = np.array([7, 9, 8], dtype=np.uint64)
    first = np.zeros(4, dtype=np.uint64)
    num = C.c_uint64()
    args = (3, cnt.ctypes.data_as(C.POINTER(C.c_uint64)), 10, 0)
    assert L.swz_input_batches(*args, 2, first.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(num)) == swz.api.ERR_BAD_ARG   # max_batches too small
    assert L.swz_input_batches(*args, 3, first.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(num)) == 0 and num.value == 3
    assert first.tolist() == [0, 10, 20, 24]
    assert L.swz_input_batches(*args, 0, None, C.byref(num)) == 0 and num.value == 3    # only the count
