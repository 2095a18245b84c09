"""LAS files written with numpy for the tests of the input side (swz_las_scan_files, swz_las_decode_segments_device,
swz_tiler_add_las_files): the public header block of LAS 1.2 / 1.3 / 1.4, variable length records, point records of
formats 0-10 with extra bytes.  TEST INFRASTRUCTURE ONLY."""
import struct

import numpy as np

import oracle_lib as O
from test_las_decode import SIZES, make_records

HEADER_SIZE = {2: 227, 3: 235, 4: 375}


def las_header(minor, fmt, record_bytes, count, scale, offset, bmin, bmax, data_offset, num_vlrs=0, legacy_count=None,
               extended_count=None):
    """The public header block of LAS 1.<minor>, little-endian."""
    size = HEADER_SIZE[minor]
    h = bytearray(size)
    h[0:4] = b"LASF"
    h[24], h[25] = 1, minor
    h[58:74] = b"numpy test files"
    struct.pack_into("<H", h, 94, size)
    struct.pack_into("<I", h, 96, data_offset)
    struct.pack_into("<I", h, 100, num_vlrs)
    h[104] = fmt
    struct.pack_into("<H", h, 105, record_bytes)
    if legacy_count is None:
        legacy_count = 0 if (minor >= 4 and fmt >= 6) else count
    struct.pack_into("<I", h, 107, legacy_count)
    struct.pack_into("<3d", h, 131, *scale)
    struct.pack_into("<3d", h, 155, *offset)
    struct.pack_into("<6d", h, 179, bmax[0], bmin[0], bmax[1], bmin[1], bmax[2], bmin[2])
    if minor >= 4:
        struct.pack_into("<Q", h, 247, count if extended_count is None else extended_count)
    return bytes(h)


def vlr(user_id, record_id, payload):
    return struct.pack("<H16sHH32s", 0, user_id.encode(), record_id, len(payload), b"test") + payload


def write_las(path, records, fmt, scale, offset, bmin, bmax, minor=2, vlrs=(), **header_args):
    """records: a structured array of make_records (or raw bytes with record_bytes in header_args).  Returns the offset to
    the point data."""
    if isinstance(records, np.ndarray):
        raw, rb, count = records.tobytes(), records.dtype.itemsize, len(records)
    else:
        raw, rb = bytes(records), header_args.pop("record_bytes")
        count = header_args.pop("count", len(raw) // rb)
    body = b"".join(vlrs)
    data_offset = header_args.pop("data_offset", HEADER_SIZE[minor] + len(body))
    head = las_header(minor, fmt, rb, count, scale, offset, bmin, bmax, data_offset, num_vlrs=len(vlrs), **header_args)
    with open(path, "wb") as f:
        f.write(head + body + raw)
    return data_offset


class LasTile:
    """One synthetic file: records whose integer coordinates lie in [lo, hi) of the file's own scale and offset, a header box
    that may be tighter than the records (clamp = True: some records are moved onto the box)."""

    def __init__(self, rng, n, fmt, extra=0, minor=None, scale=(1e-3, 1e-3, 1e-3), offset=(0.0, 0.0, 0.0), lo=0, hi=2 ** 20,
                 clamp=False, vlrs=()):
        self.n, self.fmt, self.extra = n, fmt, extra
        self.minor = minor if minor is not None else (4 if fmt >= 6 else 2)
        self.scale, self.offset, self.vlrs = list(scale), list(offset), list(vlrs)
        self.records = make_records(rng, n, fmt, extra)
        for ax in "XYZ":
            self.records[ax] = rng.integers(lo, hi, n)
        self.record_bytes = SIZES[fmt] + extra
        span_lo, span_hi = (lo + (hi - lo) // 8, hi - (hi - lo) // 8) if clamp else (lo, hi)
        self.bmin = [self.offset[k] + span_lo * self.scale[k] for k in range(3)]
        self.bmax = [self.offset[k] + span_hi * self.scale[k] for k in range(3)]

    def write(self, path):
        self.path = str(path)
        self.data_offset = write_las(self.path, self.records, self.fmt, self.scale, self.offset, self.bmin, self.bmax, minor=self.minor,
                                     vlrs=self.vlrs)
        return self.path

    def raw(self):
        return self.records.view(np.uint8).reshape(-1)

    def oracle(self, first=0, count=None):
        """(xyz, attrs) of the records [first, first + count) as the oracle decodes them"""
        count = self.n - first if count is None else count
        rec = self.raw()[first * self.record_bytes:(first + count) * self.record_bytes]
        if count == 0:
            return np.empty((0, 3)), {k: np.empty((0, O.ATTRIBUTES[k][2]) if O.ATTRIBUTES[k][2] > 1 else 0, O.ATTRIBUTES[k][1])
                                      for k in O.LAS_ATTRIBUTES}
        return O.las_decode(rec, count, self.scale, self.offset, self.bmin, self.bmax, self.fmt, self.record_bytes)

    def segment(self, first_row, byte_offset, first=0, count=None):
        return dict(first_row=first_row, count=self.n - first if count is None else count, byte_offset=byte_offset, scale=self.scale,
                    offset=self.offset, min=self.bmin, max=self.bmax, point_format=self.fmt, record_bytes=self.record_bytes)


def oracle_dataset(tiles):
    """(xyz, attrs) of all records of the tiles, file by file, as the oracle decodes them"""
    parts = [t.oracle() for t in tiles]
    xyz = np.concatenate([p[0] for p in parts])
    attrs = {k: np.concatenate([p[1][k] for p in parts]) for k in O.LAS_ATTRIBUTES}
    return xyz, attrs


def make_cubic(tmin, tmax):
    """AABB::makeCubic / getCenter (core/math/AABB.h:50-70) and total_bounds_cubic_at_origin (FileStats.cpp:30-37) restated:
    the same operations in the same order, on float64."""
    tmin, tmax = np.asarray(tmin, np.float64), np.asarray(tmax, np.float64)
    extent = tmax - tmin
    half = np.float64(max(extent[0], max(extent[1], extent[2]))) / np.float64(2)
    center = tmin + extent / np.float64(2)
    cmin, cmax = center - half, center + half
    ccenter = cmin + (cmax - cmin) / np.float64(2)
    return (cmin, cmax), (cmin - ccenter, cmax - ccenter), ccenter
