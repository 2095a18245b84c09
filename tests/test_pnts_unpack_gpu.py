"""swz_pnts_unpack_segments_device: the arrays of .pnts files unpacked on the device, the inverse of swz_pnts_pack_device.

The raw image is laid out by hand here -- POSITION, RGB and INTENSITY of every segment in a chosen order, each at a chosen
residue mod 16 of its byte offset, guard bytes between them -- and the expectation is numpy on those bytes:
np.frombuffer(...).astype(np.float64) for the positions, plain copies for the columns.  Nothing expected comes from the
library's pack kernel or reader.  Positions are compared bit for bit wherever the stored float is not a NaN, and with isnan
where it is."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
GUARD, POISON = 0xEE, 0x5A
BOTH = ("rgb", "intensity")
ORDERS = list(itertools.permutations(("position", "rgb", "intensity")))
WIDTH = {"position": 12, "rgb": 3, "intensity": 2}
# +0, -0, the smallest denormal and its negative, the largest denormal, FLT_MIN, FLT_MAX, -FLT_MAX, +inf, -inf, a quiet and a
# signalling NaN, a NaN with the sign set
SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000,
                    0xFF800000, 0x7FC00001, 0x7F800001, 0xFFC12345], dtype=np.uint32)


class Image:
    """spec: one dict per segment -- count, attrs (the arrays besides POSITION), order (of the arrays in the image), residue
    (name -> the array's byte offset mod 16).  tight: no guard in front of the first array or behind the last one."""

    def __init__(self, rng, spec, tight=False):
        raw, self.segments, want_xyz, want = bytearray(), [], [], {"rgb": [], "intensity": []}
        row = 0
        for i, sp in enumerate(spec):
            n, attrs = sp["count"], sp.get("attrs", BOTH)
            seg = dict(first_row=row, count=n, attrs=attrs, position_offset=0, rgb_offset=0, intensity_offset=0)
            bits = rng.integers(0, 2 ** 32, 3 * n, dtype=np.uint32)                 # every pattern: NaNs and denormals included
            if i == 0:
                bits[:min(3 * n, len(SPECIAL))] = SPECIAL[:3 * n]
            data = {"position": bits.tobytes(), "rgb": rng.integers(0, 256, 3 * n, dtype=np.uint8).tobytes(),
                    "intensity": rng.integers(0, 65536, n, dtype=np.uint16).tobytes()}
            for name in sp.get("order", ORDERS[0]):
                if name != "position" and name not in attrs:
                    continue
                if not (tight and len(raw) == 0):
                    res = sp.get("residue", {}).get(name)
                    pad = 1 if res is None else 1 + (res - (len(raw) + 1)) % 16
                    raw += bytes([GUARD]) * pad
                seg[name + "_offset"] = len(raw)
                raw += data[name]
            # the yardstick: numpy on the bytes of the image
            f = np.frombuffer(bytes(raw[seg["position_offset"]:seg["position_offset"] + 12 * n]), dtype="<f4").reshape(n, 3)
            with np.errstate(invalid="ignore"):                                     # (a signalling NaN is quieted by the cast)
                want_xyz.append((f, f.astype(np.float64)))
            want["rgb"].append(np.frombuffer(bytes(raw[seg["rgb_offset"]:seg["rgb_offset"] + 3 * n]), dtype=np.uint8).reshape(n, 3)
                               if "rgb" in attrs else np.zeros((n, 3), np.uint8))
            want["intensity"].append(np.frombuffer(bytes(raw[seg["intensity_offset"]:seg["intensity_offset"] + 2 * n]), dtype="<u2")
                                     if "intensity" in attrs else np.zeros(n, np.uint16))
            self.segments.append(seg)
            row += n
        if not tight:
            raw += bytes([GUARD]) * 13
        self.raw = np.frombuffer(bytes(raw), dtype=np.uint8)
        self.rows = row
        self.floats = np.concatenate([w[0] for w in want_xyz]) if want_xyz else np.empty((0, 3), np.float32)
        self.xyz = np.concatenate([w[1] for w in want_xyz]) if want_xyz else np.empty((0, 3))
        none = {"rgb": np.empty((0, 3), np.uint8), "intensity": np.empty(0, np.uint16)}
        self.cols = {k: np.concatenate(v) if v else none[k] for k, v in want.items()}


def _outputs(n, columns, front, back=5, with_xyz=True):
    """output buffers of front + n + back rows filled with a sentinel; the call gets the pointer of row `front`"""
    import torch
    dev = torch.device("cuda:0")
    rows = front + n + back
    xyz = torch.zeros((rows, 3), dtype=torch.float64, device=dev)
    xyz.view(torch.uint8).fill_(POISON)
    cols = {}
    for name in columns:
        cols[name] = torch.zeros((rows, 3) if name == "rgb" else (rows,), dtype=torch.uint8 if name == "rgb" else torch.uint16, device=dev)
        cols[name].view(torch.uint8).fill_(POISON)
    ptrs = {k: v.data_ptr() + front * (3 if k == "rgb" else 2) for k, v in cols.items()}
    return xyz, cols, (xyz.data_ptr() + front * 24) if with_xyz else None, ptrs


def _check(img, xyz, cols, front, xyz_written=True):
    n = img.rows
    got = xyz.cpu().numpy()
    if xyz_written:
        g = got[front:front + n]
        nan = np.isnan(img.floats)
        assert np.array_equal(g.view(np.uint64)[~nan], img.xyz.view(np.uint64)[~nan])     # sign of zero, denormals, infinities
        assert np.isnan(g[nan]).all()
        outside = np.concatenate([got[:front].reshape(-1), got[front + n:].reshape(-1)])
    else:
        outside = got.reshape(-1)
    assert (outside.view(np.uint8) == POISON).all()                                       # the guard bands keep the sentinel
    for k, v in cols.items():
        a = v.cpu().numpy()
        assert np.array_equal(a[front:front + n], img.cols[k]), k
        outside = np.concatenate([a[:front].reshape(-1), a[front + n:].reshape(-1)])
        assert (np.ascontiguousarray(outside).view(np.uint8) == POISON).all(), k


def _upload(raw, misalign=0):
    """the image on the device in a buffer allocated to the byte: raw begins `misalign` bytes into it and ends with it"""
    import torch
    dev = torch.device("cuda:0")
    d_buf = torch.empty(misalign + len(raw), dtype=torch.uint8, device=dev)
    if len(raw):
        d_buf[misalign:] = torch.from_numpy(raw.copy()).to(dev)
    return d_buf, d_buf.data_ptr() + misalign


def _run(ctx, img, columns=BOTH, front=3, with_xyz=True, misalign=0):
    import torch
    d_buf, d_raw = _upload(img.raw, misalign)
    xyz, cols, p_xyz, ptrs = _outputs(img.rows, columns, front, with_xyz=with_xyz)
    ctx.pnts_unpack_segments_device(d_raw, len(img.raw), img.segments, p_xyz, ptrs)
    torch.cuda.synchronize()
    _check(img, xyz, cols, front, xyz_written=with_xyz)


@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    with swz.Context(0) as c:
        yield c


@pytest.mark.parametrize("front", [0, 3])        # the positions 16-byte aligned, and 8 bytes off
@pytest.mark.parametrize("count", ["1", "T-1", "T", "T+1"])
def test_one_segment(ctx, count, front):
    import schwarzwald_amd as swz
    T = swz.pnts_unpack_tile()
    n = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1}[count]
    _run(ctx, Image(np.random.default_rng(n), [dict(count=n, residue=dict(position=1, rgb=2, intensity=7))]), front=front)


@pytest.mark.parametrize("front", [0, 3])
def test_segments_inside_and_across_tiles(ctx, front):
    """three segments inside the first tile (an empty one between them), then one across the three tiles"""
    import schwarzwald_amd as swz
    T = swz.pnts_unpack_tile()
    spec = [dict(count=7), dict(count=0), dict(count=1, order=ORDERS[3]), dict(count=40, order=ORDERS[5]),
            dict(count=2 * T + 3, order=ORDERS[4], residue=dict(position=3, rgb=1, intensity=15))]
    img = Image(np.random.default_rng(2), spec)
    assert img.segments[-1]["first_row"] < T and img.rows > 2 * T
    _run(ctx, img, front=front)


def test_every_residue_and_every_order(ctx):
    """segment i: POSITION at residue i, RGB at i + 5, INTENSITY at i + 11 (mod 16), the arrays in order i mod 6"""
    spec = [dict(count=3 + 2 * i, order=ORDERS[i % 6], residue=dict(position=i, rgb=(i + 5) % 16, intensity=(i + 11) % 16))
            for i in range(16)]
    spec += [dict(count=9, order=o) for o in ORDERS]
    img = Image(np.random.default_rng(3), spec)
    for name in ("position", "rgb", "intensity"):
        assert {s[name + "_offset"] % 16 for s in img.segments[:16]} == set(range(16))
    _run(ctx, img)


@pytest.mark.parametrize("misalign", [0, 1, 3])
@pytest.mark.parametrize("last", ["position", "rgb", "intensity"])
def test_image_that_fills_its_buffer_to_the_byte(ctx, misalign, last):
    """the first array begins with the buffer's first byte and the last ends with its last: the two ends are read as bytes"""
    import schwarzwald_amd as swz
    T = swz.pnts_unpack_tile()
    order = [o for o in ORDERS if o[-1] == last][0]
    img = Image(np.random.default_rng(4 + misalign), [dict(count=5, order=ORDERS[2]), dict(count=T + 1), dict(count=3, order=order)],
                tight=True)
    first, end = img.segments[0], img.segments[-1]
    assert first[ORDERS[2][0] + "_offset"] == 0 and end[last + "_offset"] + WIDTH[last] * 3 == len(img.raw)
    _run(ctx, img, misalign=misalign)


def _mixed_spec(T):
    return [dict(count=T - 1), dict(count=1, attrs=()), dict(count=1, attrs=("rgb",)), dict(count=1, attrs=("intensity",)),
            dict(count=2, attrs=()), dict(count=T + 1, attrs=("intensity",), order=ORDERS[4]), dict(count=99, attrs=("rgb",)),
            dict(count=100, order=ORDERS[5])]


def test_absent_arrays_give_zeros(ctx):
    import schwarzwald_amd as swz
    img = Image(np.random.default_rng(5), _mixed_spec(swz.pnts_unpack_tile()))
    assert (img.cols["rgb"] == 0).all(axis=1).sum() > 200 and (img.cols["intensity"] != 0).any()
    _run(ctx, img)


@pytest.mark.parametrize("columns,with_xyz", [((), True), (("rgb",), False), (("intensity",), True), (BOTH, False)])
def test_null_outputs_and_column_subsets(ctx, columns, with_xyz):
    import schwarzwald_amd as swz
    _run(ctx, Image(np.random.default_rng(6), _mixed_spec(swz.pnts_unpack_tile())), columns=columns, with_xyz=with_xyz)


def test_zero_segments_and_zero_rows_launch_nothing(ctx):
    import torch
    empty = Image(np.random.default_rng(7), [])
    xyz, cols, p_xyz, ptrs = _outputs(0, BOTH, front=2)
    ctx.pnts_unpack_segments_device(0, 0, [], p_xyz, ptrs)
    d_buf, d_raw = _upload(np.zeros(12, np.uint8))
    ctx.pnts_unpack_segments_device(d_raw, 12, [dict(first_row=0, count=0, position_offset=0, attrs=BOTH)], p_xyz, ptrs)
    torch.cuda.synchronize()
    _check(empty, xyz, cols, 2)


def test_refusals_launch_nothing(ctx):
    import torch
    import schwarzwald_amd as swz
    img = Image(np.random.default_rng(8), [dict(count=10), dict(count=20)])
    d_buf, d_raw = _upload(img.raw)
    xyz, cols, p_xyz, ptrs = _outputs(img.rows, BOTH, front=3)
    a, b = img.segments
    size = len(img.raw)
    other = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    cases = {
        "rows that do not start at 0": ([dict(a, first_row=1), dict(b, first_row=11)], size, ptrs, "contiguously"),
        "a gap between the rows": ([a, dict(b, first_row=11)], size, ptrs, "contiguously"),
        "rows that overlap": ([a, dict(b, first_row=9)], size, ptrs, "contiguously"),
        "positions that pass raw_bytes": ([a, b], b["position_offset"] + 12 * 20 - 1, ptrs, "passes raw_bytes"),
        "colours that pass raw_bytes": ([a, dict(b, rgb_offset=size - 3 * 20 + 1)], size, ptrs, "passes raw_bytes"),
        "intensities that pass raw_bytes": ([a, dict(b, intensity_offset=size - 2 * 20 + 1)], size, ptrs, "passes raw_bytes"),
        "an offset behind raw_bytes": ([a, dict(b, position_offset=size + 1)], size, ptrs, "passes raw_bytes"),
        "a mask bit outside RGB | INTENSITY": ([a, dict(b, attrs=swz.PNTS_RGB | 8)], size, ptrs, "does not hold"),
        "reserved": ([a, dict(b, reserved=1)], size, ptrs, "reserved"),
        "a column the format lacks": ([a, b], size, dict(ptrs, classification=other.data_ptr()), "no other output column"),
        "too many rows": ([dict(a, count=2 ** 32 - 65535)], size, ptrs, "2^32-65536"),
    }
    for what, (segments, raw_bytes, d_attrs, word) in cases.items():
        with pytest.raises(swz.SwzError) as e:
            ctx.pnts_unpack_segments_device(d_raw, raw_bytes, segments, p_xyz, d_attrs)
        assert e.value.code == ERR_BAD_ARG and word in str(e.value), (what, str(e.value))
    torch.cuda.synchronize()
    for t in [xyz, other] + list(cols.values()):
        assert (t.view(torch.uint8) == (0 if t is other else POISON)).all()              # nothing was launched
    # an array the mask does not name may lie anywhere; and the same arguments unharmed are taken
    ctx.pnts_unpack_segments_device(d_raw, size, [a, dict(b, attrs=(), rgb_offset=2 ** 40, intensity_offset=2 ** 41)], None, None)
    ctx.pnts_unpack_segments_device(d_raw, size, img.segments, p_xyz, ptrs)
    torch.cuda.synchronize()
    _check(img, xyz, cols, 3)
