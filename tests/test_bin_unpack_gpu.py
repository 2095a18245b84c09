"""swz_bin_unpack_segments_device: BIN node files unpacked on the device, the inverse of swz_bin_pack_device.

The files are written with the host swz_bin_write_node and laid one behind the other at byte offsets of every residue mod 8,
with guard bytes between and around them; what the kernel writes must equal swz_bin_read_node of each file bit for bit
(positions and doubles compared as integers, NaN payloads and -0.0 planted).  Nothing expected comes from the pack kernel."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
GUARD, POISON = 0xEE, 0x5A
ALL = ("rgb", "normal", "intensity", "classification", "edge_of_flight_line", "gps_time", "number_of_returns", "return_number",
       "point_source_id", "scan_direction_flag", "scan_angle_rank", "user_data")
MASKS = [()] + [(a,) for a in ALL] + [("rgb", "intensity"), ALL]


def _attributes():
    from schwarzwald_amd.api import ATTRIBUTES
    return ATTRIBUTES


def _torch_dtype(dt):
    import torch
    return getattr(torch, np.dtype(dt).name)


def _bits(a):
    """an array as unsigned integers of its element size: the comparison is of bits, not of values"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _rows(rng, n, names):
    """n rows with awkward bit patterns: NaNs with payloads, -0.0, infinities, denormals"""
    xyz = rng.standard_normal((n, 3)) * 1e6
    special = np.array([0x7FF8000000000001, 0xFFF0000000000000, 0x8000000000000000, 0x7FF0DEADBEEF0001, 0x0000000000000001],
                       dtype=np.uint64).view(np.float64)
    pick = rng.random((n, 3)) < 0.2
    xyz[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    cols = {}
    for name in names:
        _, dt, width = _attributes()[name]
        raw = rng.integers(0, 256, n * width * np.dtype(dt).itemsize, dtype=np.uint8)   # every bit pattern, NaNs included
        arr = raw.view(dt)
        cols[name] = arr.reshape(n, width) if width > 1 else arr
    return xyz, cols


def _counts(T):
    return [1, 2, 3, 99, 100, T - 1, 1, 1, 1, 1, 1, T, T + 1, 2 * T + 1, 1, 1, 7]


class Image:
    """files written by bin_write_node, concatenated with guard bytes so that file i starts at residue (first + i) mod 8"""

    def __init__(self, tmp, rng, spec, first_residue=0, tight=False):
        import schwarzwald_amd as swz
        parts, self.segments, self.want = [], [], []
        at, row = 0, 0
        for i, (n, names) in enumerate(spec):
            xyz, cols = _rows(rng, n, names)
            path = os.path.join(tmp, "f%d.bin" % i)
            swz.bin_write_node(path, xyz, cols)
            body = np.fromfile(path, dtype=np.uint8)
            pad = 0 if (tight and i == 0) else 8 + ((first_residue + i) - at) % 8   # 8..15 guard bytes in front
            parts.append(np.full(pad, GUARD, np.uint8))
            at += pad
            self.segments.append(dict(first_row=row, count=n, byte_offset=at, attrs=names))
            parts.append(body)
            at += len(body)
            got_xyz, got_cols = swz.bin_read_node(path)                                   # the yardstick
            assert sorted(got_cols) == sorted(names) and len(got_xyz) == n
            self.want.append((got_xyz, got_cols, names))
            row += n
        if not tight:
            parts.append(np.full(13, GUARD, np.uint8))
        self.raw = np.concatenate(parts)
        self.rows = row

    def expected(self, columns):
        xyz = np.concatenate([w[0] for w in self.want])
        cols = {}
        for name in columns:
            _, dt, width = _attributes()[name]
            pieces = []
            for got_xyz, got_cols, names in self.want:
                n = len(got_xyz)
                pieces.append(got_cols[name] if name in names else np.zeros((n, width) if width > 1 else n, dtype=dt))  # the zero fill
            cols[name] = np.concatenate(pieces)
        return xyz, cols


def _outputs(n, columns, front=3, back=5, with_xyz=True):
    """output buffers of front + n + back rows filled with a sentinel; the call gets the pointer of row `front`"""
    import torch
    dev = torch.device("cuda:0")
    rows = front + n + back
    xyz = torch.zeros((rows, 3), dtype=torch.float64, device=dev)
    xyz.view(torch.uint8).fill_(POISON)
    cols = {}
    for name in columns:
        _, dt, width = _attributes()[name]
        cols[name] = torch.zeros((rows, width) if width > 1 else (rows,), dtype=_torch_dtype(dt), device=dev)
        cols[name].view(torch.uint8).fill_(POISON)
    ptrs = {k: v.data_ptr() + front * v.element_size() * (v.shape[1] if v.dim() > 1 else 1) for k, v in cols.items()}
    return xyz, cols, (xyz.data_ptr() + front * 24) if with_xyz else None, ptrs


def _check(xyz, cols, front, n, want_xyz, want_cols, xyz_written=True):
    got = xyz.cpu().numpy()
    if xyz_written:
        assert np.array_equal(_bits(got[front:front + n]), _bits(want_xyz))
        outside = np.concatenate([got[:front].reshape(-1), got[front + n:].reshape(-1)])
    else:
        outside = got.reshape(-1)
    assert (_bits(outside).view(np.uint8) == POISON).all()   # rows outside the segments keep the sentinel
    for k, v in cols.items():
        a = v.cpu().numpy()
        assert np.array_equal(_bits(a[front:front + n]), _bits(want_cols[k])), k
        outside = np.concatenate([a[:front].reshape(-1), a[front + n:].reshape(-1)])
        assert (_bits(outside).view(np.uint8) == POISON).all(), k


def _upload(raw, misalign=0):
    """the image on the device in a buffer allocated to the byte: raw begins `misalign` bytes into it and ends with it"""
    import torch
    dev = torch.device("cuda:0")
    d_buf = torch.empty(misalign + len(raw), dtype=torch.uint8, device=dev)
    d_buf[misalign:] = torch.from_numpy(raw).to(dev)
    return d_buf, d_buf.data_ptr() + misalign


@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    with swz.Context(0) as c:
        yield c


@pytest.mark.parametrize("mask_index", range(len(MASKS)))
def test_unpack_equals_bin_read_node(ctx, tmp_path, mask_index):
    import torch
    import schwarzwald_amd as swz
    names = MASKS[mask_index]
    T = swz.bin_unpack_tile()
    rng = np.random.default_rng(100 + mask_index)
    img = Image(str(tmp_path), rng, [(n, names) for n in _counts(T)], first_residue=mask_index)
    assert {s["byte_offset"] % 8 for s in img.segments} == set(range(8))
    assert any(s["count"] % 2 == 1 and s["count"] > 50 for s in img.segments)     # 3 n bytes of RGB with n odd: odd addresses behind
    want_xyz, want = img.expected(names)
    d_buf, d_raw = _upload(img.raw)
    xyz, cols, p_xyz, ptrs = _outputs(img.rows, names)
    ctx.bin_unpack_segments_device(d_raw, len(img.raw), img.segments, p_xyz, ptrs)
    torch.cuda.synchronize()
    _check(xyz, cols, 3, img.rows, want_xyz, want)


@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
def test_image_that_fills_its_buffer_to_the_byte(ctx, tmp_path, misalign):
    """the first file starts with the buffer's first byte and the last ends with its last: the two ends are read as bytes"""
    import torch
    import schwarzwald_amd as swz
    T = swz.bin_unpack_tile()
    rng = np.random.default_rng(7 + misalign)
    names = ("rgb", "intensity", "gps_time", "user_data")
    img = Image(str(tmp_path), rng, [(n, names) for n in (5, T + 1, 1, 1, 3)], first_residue=0, tight=True)
    assert img.segments[0]["byte_offset"] == 0 and img.segments[-1]["byte_offset"] + 12 + 3 * (24 + 14) == len(img.raw)
    want_xyz, want = img.expected(names)
    d_buf, d_raw = _upload(img.raw, misalign)
    xyz, cols, p_xyz, ptrs = _outputs(img.rows, names)
    ctx.bin_unpack_segments_device(d_raw, len(img.raw), img.segments, p_xyz, ptrs)
    torch.cuda.synchronize()
    _check(xyz, cols, 3, img.rows, want_xyz, want)


def _mixed_spec(T):
    few, some = ("intensity",), ("rgb", "intensity", "gps_time")
    return [(T - 1, ALL), (1, ()), (1, few), (1, some), (1, ALL), (2, ()), (T + 1, some), (3, few), (99, ("normal", "gps_time")),
            (2 * T + 1, ()), (100, ALL)]


def test_segments_with_different_masks_zero_fill(ctx, tmp_path):
    import torch
    import schwarzwald_amd as swz
    T = swz.bin_unpack_tile()
    img = Image(str(tmp_path), np.random.default_rng(5), _mixed_spec(T), first_residue=3)
    want_xyz, want = img.expected(ALL)
    assert any((want[a] == 0).all() for a in ALL) is False                        # every column is filled by some segment
    d_buf, d_raw = _upload(img.raw)
    xyz, cols, p_xyz, ptrs = _outputs(img.rows, ALL)
    ctx.bin_unpack_segments_device(d_raw, len(img.raw), img.segments, p_xyz, ptrs)
    torch.cuda.synchronize()
    _check(xyz, cols, 3, img.rows, want_xyz, want)


@pytest.mark.parametrize("columns,with_xyz", [((), True), (("gps_time", "rgb"), False), (("point_source_id",), True), (ALL, False)])
def test_null_outputs_and_column_subsets(ctx, tmp_path, columns, with_xyz):
    """columns absent from d_out are skipped (the arrays in front of and behind them still count), d_xyz_out may be NULL"""
    import torch
    import schwarzwald_amd as swz
    T = swz.bin_unpack_tile()
    img = Image(str(tmp_path), np.random.default_rng(11), _mixed_spec(T), first_residue=6)
    want_xyz, want = img.expected(columns)
    d_buf, d_raw = _upload(img.raw)
    xyz, cols, p_xyz, ptrs = _outputs(img.rows, columns, with_xyz=with_xyz)
    ctx.bin_unpack_segments_device(d_raw, len(img.raw), img.segments, p_xyz, ptrs)
    torch.cuda.synchronize()
    _check(xyz, cols, 3, img.rows, want_xyz, want, xyz_written=with_xyz)


def test_zero_segments_and_zero_rows_launch_nothing(ctx, tmp_path):
    import torch
    xyz, cols, p_xyz, ptrs = _outputs(4, ("rgb",), front=0, back=0)
    ctx.bin_unpack_segments_device(0, 0, [], p_xyz, ptrs)
    d_buf, d_raw = _upload(np.zeros(12, np.uint8))
    ctx.bin_unpack_segments_device(d_raw, 12, [dict(first_row=0, count=0, byte_offset=0, attrs=())], p_xyz, ptrs)
    torch.cuda.synchronize()
    _check(xyz, cols, 0, 0, np.empty((0, 3)), {"rgb": np.empty((0, 3), np.uint8)})


def test_refusals_launch_nothing(ctx, tmp_path):
    import torch
    import schwarzwald_amd as swz
    names = ("rgb", "intensity")
    img = Image(str(tmp_path), np.random.default_rng(3), [(10, names), (20, names)])
    d_buf, d_raw = _upload(img.raw)
    xyz, cols, p_xyz, ptrs = _outputs(img.rows, names)
    a, b = img.segments
    size_b = 12 + 20 * (24 + 5)
    cases = {
        "rows that do not start at 0": ([dict(a, first_row=1), dict(b, first_row=11)], len(img.raw), "contiguously"),
        "a gap between the rows": ([a, dict(b, first_row=11)], len(img.raw), "contiguously"),
        "rows that overlap": ([a, dict(b, first_row=9)], len(img.raw), "contiguously"),
        "an image that passes raw_bytes": ([a, b], b["byte_offset"] + size_b - 1, "passes raw_bytes"),
        "an offset behind raw_bytes": ([a, dict(b, byte_offset=len(img.raw) + 1)], len(img.raw), "passes raw_bytes"),
        "a mask bit that does not exist": ([a, dict(b, attrs=1 << 12)], len(img.raw), "does not exist"),
        "too many rows": ([dict(a, count=2 ** 32 - 65535)], len(img.raw), "2^32-65536"),
    }
    for what, (segments, raw_bytes, word) in cases.items():
        with pytest.raises(swz.SwzError) as e:
            ctx.bin_unpack_segments_device(d_raw, raw_bytes, segments, p_xyz, ptrs)
        assert e.value.code == ERR_BAD_ARG and word in str(e.value), (what, str(e.value))
    torch.cuda.synchronize()
    for t in [xyz] + list(cols.values()):
        assert (t.view(torch.uint8) == POISON).all()                              # nothing was launched
    # and the same arguments unharmed are taken
    ctx.bin_unpack_segments_device(d_raw, len(img.raw), img.segments, p_xyz, ptrs)
    torch.cuda.synchronize()
    _check(xyz, cols, 3, img.rows, *img.expected(names))
