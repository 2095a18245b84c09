"""3D Tiles node files (core/io/PNTSWriter.cpp:109-264, 507-527; core/io/Cesium3DTilesPersistence.cpp:53-78).

The expected bytes are written out by hand here from the layout: a 28-byte header, the feature-table JSON padded with
spaces to a multiple of 8 (counted from the start of the JSON), then the binary -- POSITION 3 x f32 at 0, RGB 3 x u8 at
12 * count, INTENSITY u16 at the next multiple of 2, zeros up to a multiple of 8.  JSON is compared after json.loads: the
spelling of a number is no part of the format.

CPU part: the layout function, the two host writers (packed body / unpacked rows) against the hand-written bytes, the
reader on good, foreign and malformed files, the grey table of --calculate-rgb-from against the reference's expression
evaluated with the host's logf, and the numbers of the JSON.  GPU part: swz_pnts_pack_device against the hand-written
image of a synthetic node table (no tiling involved), its refusals, and tile -> node lists -> pack -> copy -> files
against the rows the oracle assigns to every node, single batch and a FAST tiler's export.
"""
import ctypes as C
import json
import math
import os
import struct

import numpy as np
import pytest

import oracle_lib as O

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
MASKS = [(), ("rgb",), ("intensity",), ("rgb", "intensity")]
ERR_BAD_ARG = 2


# ------------------------------------------------------------------------------------------ the layout, by hand
def _layout(count, names):
    """(rgb offset, intensity offset, body size) of a node of `count` points; an absent array has offset None."""
    if count == 0:
        return None, None, 0
    at = 12 * count
    rgb = inten = None
    if "rgb" in names:
        rgb = at
        at += 3 * count
    if "intensity" in names:
        at += at % 2
        inten = at
        at += 2 * count
    return rgb, inten, (at + 7) // 8 * 8


def _expected_body(xyz, rgb, intensity, names):
    n = len(xyz)
    o_rgb, o_int, size = _layout(n, names)
    body = bytearray(size)
    body[0:12 * n] = np.ascontiguousarray(xyz, dtype=np.float64).astype("<f4").tobytes()
    if o_rgb is not None:
        body[o_rgb:o_rgb + 3 * n] = np.ascontiguousarray(rgb, dtype=np.uint8).tobytes()
    if o_int is not None:
        body[o_int:o_int + 2 * n] = np.ascontiguousarray(intensity, dtype="<u2").tobytes()
    return bytes(body)


def _expected_json(n, names, rtc):
    o_rgb, o_int, _ = _layout(n, names)
    want = {"POINTS_LENGTH": n, "RTC_CENTER": list(rtc), "POSITION": {"byteOffset": 0}}
    if o_rgb is not None:
        want["RGB"] = {"byteOffset": o_rgb}
    if o_int is not None:
        want["INTENSITY"] = {"byteOffset": o_int}
    return want


def _split(data):
    """The test's own parser: (header fields, JSON text, binary)."""
    assert data[:4] == b"pnts"
    version, length, json_len, bin_len, bt_json, bt_bin = struct.unpack("<6I", data[4:28])
    assert version == 1 and bt_json == 0 and bt_bin == 0
    assert length == len(data) == 28 + json_len + bin_len
    assert json_len % 8 == 0 and bin_len % 8 == 0
    return json_len, data[28:28 + json_len].decode(), data[28 + json_len:]


def _parse(data):
    _, text, binary = _split(data)
    head = json.loads(text)
    n = head["POINTS_LENGTH"]
    out = {"xyz": np.frombuffer(binary, "<f4", 3 * n, head["POSITION"]["byteOffset"]).reshape(n, 3)}
    if "RGB" in head:
        out["rgb"] = np.frombuffer(binary, np.uint8, 3 * n, head["RGB"]["byteOffset"]).reshape(n, 3)
    if "INTENSITY" in head:
        out["intensity"] = np.frombuffer(binary, "<u2", n, head["INTENSITY"]["byteOffset"])
    return head, out


_GREY = {}


def _grey(mapping, intensity):
    """RGBFromIntensityAttribute (PNTSWriter.cpp:507-527) with the host's own logf and double log."""
    i = np.asarray(intensity, dtype=np.uint16)
    if mapping == 1:
        return (i >> 8).astype(np.uint8)
    if mapping in _GREY:
        return _GREY[mapping][i]
    libm = C.CDLL("libm.so.6")
    libm.logf.restype = C.c_float
    libm.logf.argtypes = [C.c_float]
    logs = np.array([libm.logf(float(np.float32(v) + np.float32(1))) for v in range(65536)], dtype=np.float32)
    numerator = (np.float32(255) * logs).astype(np.float32)          # 255 * std::log(float): a float product
    table = (numerator.astype(np.float64) / math.log(65535)).astype(np.uint8)   # divided in double, the cast truncates
    _GREY[mapping] = table
    return table[i]


def _hard_positions(rng, n):
    xyz = (rng.random((n, 3)) - 0.5) * 2000.0
    special = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24), -123456.789, 1e-39, -1e-45, 4.5e6 + 1e-9, 0.1]
    flat = xyz.reshape(-1)
    flat[:min(len(special), flat.size)] = special[:flat.size]
    return xyz


# ------------------------------------------------------------------------------------------ CPU: layout
def test_layout_of_counts_and_masks():
    import schwarzwald_amd as swz
    counts = [0, 1, 2, 3, 5, 7, 8, 4097]
    for names in MASKS:
        got = swz.pnts_layout(counts, names)
        at = 0
        for k, c in enumerate(counts):
            o_rgb, o_int, size = _layout(c, names)
            assert got["size"][k] == size and size % 8 == 0, (names, c)
            assert got["offset"][k] == at
            assert got["rgb_offset"][k] == (o_rgb or 0) and got["intensity_offset"][k] == (o_int or 0)
            at += size
        assert got["total"] == at
    # the smallest case that has everything: RGB at 12, intensity at 16 (15 rounded up), 24 bytes, 6 of them padding
    one = swz.pnts_layout([1], ("rgb", "intensity"))
    assert (one["rgb_offset"][0], one["intensity_offset"][0], one["size"][0]) == (12, 16, 24)
    both = swz.pnts_layout([2, 3], ("rgb", "intensity"))
    assert both["intensity_offset"][0] == 30 and both["intensity_offset"][1] == 46     # even: 15 c, odd: 15 c + 1
    assert swz.pnts_layout([], ())["total"] == 0
    with pytest.raises(swz.SwzError):
        swz.pnts_layout([1], 2)        # bit 1 is the normals: no .pnts array
    with pytest.raises(swz.SwzError):
        swz.pnts_layout([1 << 40], ())  # byteLength is a u32


# ------------------------------------------------------------------------------------------ CPU: the host writers
@pytest.mark.parametrize("names", MASKS)
@pytest.mark.parametrize("n", [1, 2, 5, 333])
def test_host_writers_against_the_hand_written_bytes(tmp_path, names, n):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(100 + n)
    xyz = _hard_positions(rng, n)
    rgb = rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8)
    inten = rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)
    rtc = [4.5e6 + 1e-9, -0.1, 123456789.125]
    body = _expected_body(xyz, rgb, inten, names)
    p_rows, p_body = str(tmp_path / "rows.pnts"), str(tmp_path / "body.pnts")
    swz.pnts_write_node_rows(p_rows, xyz, {"rgb": rgb, "intensity": inten}, write=names, rtc_center=rtc)
    swz.pnts_write_node(p_body, n, np.frombuffer(body, np.uint8), names, rtc_center=rtc)
    data = open(p_rows, "rb").read()
    assert data == open(p_body, "rb").read()
    json_len, text, binary = _split(data)
    stripped = text.rstrip(" ")
    assert len(text) - len(stripped) < 8 and " " not in stripped and "\n" not in stripped
    assert json.loads(text) == _expected_json(n, names, rtc)
    assert list(json.loads(text)) == ["POINTS_LENGTH", "RTC_CENTER", "POSITION"] + [k.upper() for k in names]
    assert binary == body
    # a float tie rounds to even, a value below the smallest normal float survives as a denormal
    if n >= 2:
        got = np.frombuffer(binary, "<f4", 6)
        assert got[0] == np.float32(1.0) and got[1] == np.float32(1 + 2.0 ** -22) and got[4] == np.float32(1e-39) != 0
    # the library's reader and the test's own parser return what was written
    head, arrays = _parse(data)
    r_xyz, r_attrs, r_rtc = swz.pnts_read_node(p_rows)
    assert r_rtc == rtc and head["RTC_CENTER"] == rtc
    assert np.array_equal(r_xyz, xyz.astype(np.float32).astype(np.float64)) and np.array_equal(arrays["xyz"], xyz.astype(np.float32))
    assert set(r_attrs) == set(names)
    for k, want in (("rgb", rgb), ("intensity", inten)):
        if k in names:
            assert np.array_equal(r_attrs[k], want) and np.array_equal(arrays[k], want)


def test_body_of_the_wrong_size_and_bad_masks_are_refused(tmp_path):
    import schwarzwald_amd as swz
    p = str(tmp_path / "x.pnts")
    with pytest.raises(swz.SwzError) as e:
        swz.pnts_write_node(p, 1, np.zeros(16, np.uint8), ("rgb", "intensity"))     # the body is 24 bytes
    assert e.value.code == ERR_BAD_ARG
    with pytest.raises(swz.SwzError):
        swz.pnts_write_node_rows(p, np.zeros((1, 3)), {}, write=("rgb",))           # no colour column
    with pytest.raises(swz.SwzError):
        swz.pnts_write_node_rows(p, np.zeros((1, 3)), {"rgb": np.zeros((1, 3), np.uint8)}, write=("rgb",), rgb_from=1)
    with pytest.raises(swz.SwzError):
        swz.pnts_write_node_rows(p, np.zeros((1, 3)), {}, write=("intensity",))
    assert not os.path.exists(p)


def test_empty_node_writes_no_file_and_unwritable_directory_is_an_error(tmp_path):
    import schwarzwald_amd as swz
    swz.pnts_write_node(str(tmp_path / "none.pnts"), 0, np.empty(0, np.uint8))
    swz.pnts_write_node_rows(str(tmp_path / "none2.pnts"), np.empty((0, 3)))
    assert list(tmp_path.iterdir()) == []
    gone = str(tmp_path / "does" / "not" / "exist" / "r.pnts")
    with pytest.raises(swz.SwzError):
        swz.pnts_write_node(gone, 1, np.zeros(16, np.uint8))
    with pytest.raises(swz.SwzError):
        swz.pnts_write_node_rows(gone, np.zeros((1, 3)))


@pytest.mark.parametrize("mapping", [1, 2])
def test_rgb_from_intensity_is_written_without_a_colour_column(tmp_path, mapping):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(7)
    n = 257
    xyz = rng.random((n, 3))
    inten = rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)
    inten[:4] = [0, 1, 65535, 255]
    grey = _grey(mapping, inten)
    p = str(tmp_path / "grey.pnts")
    swz.pnts_write_node_rows(p, xyz, {"intensity": inten}, write=("rgb", "intensity"), rgb_from=mapping)
    _, text, binary = _split(open(p, "rb").read())
    assert binary == _expected_body(xyz, np.repeat(grey[:, None], 3, axis=1), inten, ("rgb", "intensity"))
    assert json.loads(text) == _expected_json(n, ("rgb", "intensity"), [0.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------ CPU: the reader
def _file(json_text, binary, pad_to=8, length=None, magic=b"pnts", version=1):
    text = json_text.encode()
    text += b" " * (-len(text) % pad_to)
    total = 28 + len(text) + len(binary)
    return magic + struct.pack("<6I", version, total if length is None else length, len(text), len(binary), 0, 0) + text + binary


def test_reader_uses_the_offsets_of_a_foreign_file(tmp_path):
    """Arrays in another order, gaps between them, a JSON with whitespace, unknown members and a longer padding."""
    import schwarzwald_amd as swz
    rng = np.random.default_rng(8)
    n = 5
    xyz = rng.random((n, 3)).astype(np.float32)
    rgb = rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8)
    inten = rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)
    binary = bytearray(b"\xEE" * 120)
    binary[2:12] = inten.tobytes()         # INTENSITY at 2
    binary[13:28] = rgb.tobytes()          # RGB at 13
    binary[40:100] = xyz.tobytes()         # POSITION at 40
    text = ('{ "INTENSITY" : {"byteOffset": 2, "componentType": "UNSIGNED_SHORT"},\n "extras": {"a": [1, {"b": null}], "s": "q\\"}"},'
            ' "RGB": {"byteOffset":13}, "RTC_CENTER": [1.5, -2e3, 0.25], "POSITION": {"byteOffset": 40}, "POINTS_LENGTH": 5, "ok": true}')
    p = tmp_path / "foreign.pnts"
    p.write_bytes(_file(text, bytes(binary), pad_to=32))
    got_xyz, got_attrs, rtc = swz.pnts_read_node(str(p))
    assert np.array_equal(got_xyz, xyz.astype(np.float64)) and rtc == [1.5, -2000.0, 0.25]
    assert np.array_equal(got_attrs["rgb"], rgb) and np.array_equal(got_attrs["intensity"], inten)


def test_reader_refuses_malformed_files(tmp_path):
    import schwarzwald_amd as swz
    n = 3
    good_json = '{"POINTS_LENGTH":3,"RTC_CENTER":[0,0,0],"POSITION":{"byteOffset":0},"RGB":{"byteOffset":36}}'
    binary = bytes(48)
    good = _file(good_json, binary)
    cases = {
        "good": good,
        "short file": good[:20],
        "empty file": b"",
        "wrong magic": _file(good_json, binary, magic=b"b3dm"),
        "byteLength larger than the file": _file(good_json, binary, length=len(good) + 8),
        "file cut off": good[:-8],
        "trailing bytes": good + bytes(8),
        "json length passes the file": good[:12] + struct.pack("<I", 1 << 20) + good[16:],
        "binary length passes the file": good[:16] + struct.pack("<I", 1 << 30) + good[20:],
        "position passes the binary": _file(good_json.replace('"byteOffset":0', '"byteOffset":16'), binary),
        "rgb passes the binary": _file(good_json.replace("36", "40"), binary),
        "count too large for the binary": _file(good_json.replace('"POINTS_LENGTH":3', '"POINTS_LENGTH":4000000000'), binary),
        "negative offset": _file(good_json.replace("36", "-4"), binary),
        "huge offset": _file(good_json.replace("36", "1e300"), binary),
        "json cut off": _file(good_json[:-20], binary),
        "json not an object": _file("[1,2,3]", binary),
        "no POINTS_LENGTH": _file(good_json.replace("POINTS_LENGTH", "POINTS"), binary),
        "no POSITION": _file(good_json.replace("POSITION", "POS"), binary),
        "garbage json": _file("{" + "\xff" * 30, binary),
        "unterminated string": _file('{"POINTS_LENGTH', binary),
        "deep nesting": _file('{"a":' + "[" * 5000 + "]" * 5000 + "}", binary),
    }
    for name, data in cases.items():
        p = tmp_path / "case.pnts"
        p.write_bytes(data)
        if name == "good":
            assert swz.pnts_read_node(str(p))[0].shape == (n, 3)
            continue
        with pytest.raises(swz.SwzError) as e:
            swz.pnts_read_node(str(p))
        assert e.value.code == ERR_BAD_ARG, name
        L = swz.load_library()
        xyz = np.full((n, 3), 7.0)
        cols = swz.api._AttributeColumns()
        assert L.swz_pnts_read_node(None, str(p).encode(), xyz.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cols)) == ERR_BAD_ARG, name
        assert np.all(xyz == 7.0), name
    with pytest.raises(swz.SwzError):
        swz.pnts_read_node(str(tmp_path / "missing.pnts"))


# ------------------------------------------------------------------------------------------ CPU: grey table, numbers
@pytest.mark.parametrize("mapping", [1, 2])
def test_grey_table_equals_the_reference_expression_for_every_intensity(mapping):
    import schwarzwald_amd as swz
    want = _grey(mapping, np.arange(65536))
    got = np.array([swz.pnts_rgb_from_intensity(mapping, i) for i in range(65536)], dtype=np.uint8)
    assert np.array_equal(got, want)
    assert got[0] == 0 and got[65535] == 255 and np.all(np.diff(got.astype(int)) >= 0)
    assert swz.pnts_rgb_from_intensity(0, 40000) == 0


def test_json_numbers_parse_back_bit_equal(tmp_path):
    import schwarzwald_amd as swz
    values = [0.1, 1 / 3, -0.0, 5e-324, 1e21, 123456789.125, float(2 ** 53 + 2), 4.5e6 + 1e-9, 1.7976931348623157e308]
    for i in range(0, len(values), 3):
        rtc = values[i:i + 3]
        p = str(tmp_path / "n.pnts")
        swz.pnts_write_node_rows(p, np.zeros((1, 3)), rtc_center=rtc)
        _, text, _ = _split(open(p, "rb").read())
        raw = text[text.index("[") + 1:text.index("]")].split(",")
        assert [struct.pack("<d", float(s)) for s in raw] == [struct.pack("<d", v) for v in rtc], raw
        assert [struct.pack("<d", v) for v in json.loads(text)["RTC_CENTER"]] == [struct.pack("<d", v) for v in rtc]
        assert all(len(s) <= len(repr(v)) for s, v in zip(raw, rtc)), raw       # never longer than Python's shortest form
    with pytest.raises(swz.SwzError):
        swz.pnts_write_node_rows(str(tmp_path / "nan.pnts"), np.zeros((1, 3)), rtc_center=[0.0, float("nan"), 0.0])


# ------------------------------------------------------------------------------------------ GPU: the pack kernel
def _synthetic_table():
    rng = np.random.default_rng(9)
    counts = np.array([0, 1, 5000, 3, 0, 777, 2, 1, 1, 255, 256, 257] + list(rng.integers(1, 400, 60)), dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    return counts, offsets


def _expected_image(counts, offsets, rows_xyz, rows_rgb, rows_int, names):
    parts = []
    for c, o in zip(counts, offsets):
        s = slice(int(o), int(o + c))
        parts.append(_expected_body(rows_xyz[s], rows_rgb[s], rows_int[s], names) if c else b"")
    return b"".join(parts)


@pytest.fixture(scope="module")
def packed_inputs():
    import torch
    counts, offsets = _synthetic_table()
    n = int(counts.sum())
    # empty nodes, several nodes inside one wavefront, a node over many blocks of 256 rows
    rng = np.random.default_rng(10)
    src = n + n // 2
    xyz = _hard_positions(rng, src)
    rgb = rng.integers(0, 255, (src, 3), endpoint=True).astype(np.uint8)
    inten = rng.integers(0, 65535, src, endpoint=True).astype(np.uint16)
    perm = rng.permutation(src).astype(np.uint32)[:n]
    order = rng.permutation(n).astype(np.uint32)
    dev = torch.device("cuda:0")
    d = dict(xyz=torch.from_numpy(xyz).to(dev), rgb=torch.from_numpy(rgb).to(dev), intensity=torch.from_numpy(inten.view(np.int16)).to(dev),
             perm=torch.from_numpy(perm.view(np.int32)).to(dev), order=torch.from_numpy(order.view(np.int32)).to(dev))
    torch.cuda.synchronize()
    return dict(counts=counts, offsets=offsets, n=n, xyz=xyz, rgb=rgb, intensity=inten, perm=perm, order=order, d=d)


GUARD = 4096


@pytest.mark.gpu
@pytest.mark.parametrize("with_order", [True, False])
def test_gpu_pack_writes_the_hand_written_image(packed_inputs, with_order):
    import torch
    import schwarzwald_amd as swz
    P = packed_inputs
    d = P["d"]
    rows = P["perm"][P["order"]] if with_order else P["perm"]
    nodes = dict(offset=P["offsets"], count=P["counts"])
    with swz.Context(0) as ctx:
        for names in MASKS:
            lay = swz.pnts_layout(P["counts"], names)
            total = lay["total"]
            for mapping in (0, 1, 2):
                rgb_rows = P["rgb"][rows] if mapping == 0 else np.repeat(_grey(mapping, P["intensity"][rows])[:, None], 3, axis=1)
                want = _expected_image(P["counts"], P["offsets"], P["xyz"][rows], rgb_rows, P["intensity"][rows], names)
                assert len(want) == total
                buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                # with a mapping the colour column is not needed: leave it out
                attrs = {"intensity": d["intensity"].data_ptr()}
                if mapping == 0:
                    attrs["rgb"] = d["rgb"].data_ptr()
                ctx.pnts_pack_device(d["perm"].data_ptr(), d["order"].data_ptr() if with_order else None, P["n"], d["xyz"].data_ptr(),
                                     attrs, nodes, buf.data_ptr() + GUARD, total, attrs=names, rgb_from=mapping)
                got = buf.cpu().numpy()
                assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + total:] == 0xA5), (names, mapping)
                image = got[GUARD:GUARD + total].tobytes()
                if image != want:
                    bad = np.flatnonzero(np.frombuffer(image, np.uint8) != np.frombuffer(want, np.uint8))
                    k = int(np.searchsorted(lay["offset"], bad[0], side="right") - 1)
                    pytest.fail("mask %s mapping %d: %d bytes differ, first at %d = node %d (count %d) + %d"
                                % (names, mapping, len(bad), bad[0], k, P["counts"][k], bad[0] - lay["offset"][k]))


@pytest.mark.gpu
def test_gpu_pack_handles_gaps_a_short_table_and_nothing_to_do(packed_inputs):
    """Rows that belong to no node (in front of the first, between two and behind the last) are skipped, node boundaries at
    and next to a block edge; no nodes and n == 0 launch nothing."""
    import torch
    import schwarzwald_amd as swz
    P = packed_inputs
    d = P["d"]
    # [250, 256) ends on a block edge, [256, 511) starts on it and ends one row before the next, [511, 513) straddles that one
    counts = np.array([3, 0, 6, 255, 2, 187, 1], dtype=np.uint64)
    offsets = np.array([2, 5, 250, 256, 511, 513, 701], dtype=np.uint64)
    names = ("rgb", "intensity")
    rows = P["perm"]
    total = swz.pnts_layout(counts, names)["total"]
    want = _expected_image(counts, offsets, P["xyz"][rows], P["rgb"][rows], P["intensity"][rows], names)
    with swz.Context(0) as ctx:
        buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        attrs = {"rgb": d["rgb"].data_ptr(), "intensity": d["intensity"].data_ptr()}
        ctx.pnts_pack_device(d["perm"].data_ptr(), None, P["n"], d["xyz"].data_ptr(), attrs, dict(offset=offsets, count=counts),
                             buf.data_ptr() + GUARD, total, attrs=names)
        got = buf.cpu().numpy()
        assert got[GUARD:GUARD + total].tobytes() == want
        assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + total:] == 0xA5)
        buf.fill_(0xA5)
        torch.cuda.synchronize()
        empty = dict(offset=np.empty(0, np.uint64), count=np.empty(0, np.uint64))
        ctx.pnts_pack_device(d["perm"].data_ptr(), None, P["n"], d["xyz"].data_ptr(), attrs, empty, buf.data_ptr() + GUARD, total, attrs=names)
        ctx.pnts_pack_device(None, None, 0, None, attrs, empty, None, 0, attrs=names)
        ctx.pnts_pack_device(d["perm"].data_ptr(), None, P["n"], d["xyz"].data_ptr(), attrs,
                             dict(offset=np.array([5, 9], np.uint64), count=np.zeros(2, np.uint64)), buf.data_ptr() + GUARD, total, attrs=names)
        assert np.all(buf.cpu().numpy() == 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("names", [MASKS[0], MASKS[3]])
def test_gpu_pack_tiles_of_one_point_nodes(packed_inputs, names):
    """Every row a node of its own: a block lists as many nodes as it has rows, the whole window of its table; the nine
    two-point nodes shift the node boundaries against the block edges from the middle of the first block on."""
    import torch
    import schwarzwald_amd as swz
    P = packed_inputs
    d = P["d"]
    T = 256  # rows per block of the pack kernel
    counts = np.ones(2 * T + 3, np.uint64)
    counts[T // 2:T // 2 + 9] = 2
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    n = int(counts.sum())
    rows = P["perm"][:n]
    total = swz.pnts_layout(counts, names)["total"]
    want = _expected_image(counts, offsets, P["xyz"][rows], P["rgb"][rows], P["intensity"][rows], names)
    assert len(want) == total
    with swz.Context(0) as ctx:
        buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        attrs = {"rgb": d["rgb"].data_ptr(), "intensity": d["intensity"].data_ptr()}
        ctx.pnts_pack_device(d["perm"].data_ptr(), None, n, d["xyz"].data_ptr(), attrs, dict(offset=offsets, count=counts),
                             buf.data_ptr() + GUARD, total, attrs=names)
        got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + total:] == 0xA5)
    assert got[GUARD:GUARD + total].tobytes() == want


@pytest.mark.gpu
def test_gpu_pack_refuses_bad_tables_before_anything_is_launched(packed_inputs):
    import torch
    import schwarzwald_amd as swz
    P = packed_inputs
    d = P["d"]
    n = P["n"]
    u = lambda *v: np.array(v, dtype=np.uint64)
    both = {"rgb": d["rgb"].data_ptr(), "intensity": d["intensity"].data_ptr()}
    good = dict(offset=u(0, 10), count=u(10, 5))
    cases = [
        ("offsets not ascending", dict(offset=u(10, 0), count=u(5, 10)), both, ("rgb",), 0, n),
        ("ranges overlap", dict(offset=u(0, 9), count=u(10, 5)), both, ("rgb",), 0, n),
        ("range passes n", dict(offset=u(0, n - 2), count=u(10, 3)), both, ("rgb",), 0, n),
        ("offset passes n", dict(offset=u(0, n + 1), count=u(10, 1)), both, ("rgb",), 0, n),
        ("count wraps around", dict(offset=u(0, 16), count=u(10, 2 ** 64 - 8)), both, ("rgb",), 0, n),
        ("mask names absent rgb", good, {"intensity": d["intensity"].data_ptr()}, ("rgb",), 0, n),
        ("mask names absent intensity", good, {"rgb": d["rgb"].data_ptr()}, ("intensity",), 0, n),
        ("mapping without intensity", good, {"rgb": d["rgb"].data_ptr()}, ("rgb",), 2, n),
        ("unknown mapping", good, both, ("rgb",), 3, n),
        ("unknown mask bit", good, both, 8, 0, n),
        ("n above the limit", good, both, ("rgb",), 0, 2 ** 32 - 65535),
    ]
    with swz.Context(0) as ctx:
        buf = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        for name, nodes, attrs, mask, mapping, rows in cases:
            with pytest.raises(swz.SwzError) as e:
                ctx.pnts_pack_device(d["perm"].data_ptr(), None, rows, d["xyz"].data_ptr(), attrs, nodes, buf.data_ptr(), 1 << 16,
                                     attrs=mask, rgb_from=mapping)
            assert e.value.code == ERR_BAD_ARG, name
        with pytest.raises(swz.SwzError) as e:   # an image buffer smaller than the layout
            ctx.pnts_pack_device(d["perm"].data_ptr(), None, n, d["xyz"].data_ptr(), both, good, buf.data_ptr(), 100, attrs=("rgb",))
        assert e.value.code == ERR_BAD_ARG
        torch.cuda.synchronize()
        assert np.all(buf.cpu().numpy() == 0xA5)


# ------------------------------------------------------------------------------------------ GPU: end to end
def _oracle_node_rows(tile):
    """oracle tile result -> {node name: rows of the input, in file order}"""
    keys, perm, level = tile["keys"], tile["perm"], tile["level"]
    order = np.lexsort((np.arange(len(keys)), level))
    out = {}
    i = 0
    while i < len(order):
        p = order[i]
        L = int(level[p])
        shift = 63 if L < 0 else 3 * (20 - L)
        prefix = int(keys[p]) >> shift
        j = i
        while j < len(order) and level[order[j]] == L and (int(keys[order[j]]) >> shift) == prefix:
            j += 1
        name = "r" + "".join(str((int(keys[p]) >> (3 * (20 - l))) & 7) for l in range(L + 1))
        out[name] = perm[order[i:j]]
        i = j
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", [O.GRID_CENTER, O.MIN_DISTANCE])
def test_gpu_node_files_hold_the_rows_the_oracle_assigns(tmp_path, sampler):
    import torch
    import schwarzwald_amd as swz
    rng = np.random.default_rng(31)
    n = 20_000
    xyz = rng.random((n, 3))
    rgb = rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8)
    inten = rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)
    # a spacing of diagonal / 16 makes the root and its eight children overflow: 1 + 8 + 64 nodes, the fullest tree that
    # 20 000 points at 500 per node fill (a finer spacing leaves almost every point in the root)
    spacing = O.spacing_from_diagonal(*UNIT, 16)
    o = O.tile(xyz, *UNIT, sampler, 500, spacing)
    assert o["status"] == 0
    want = _oracle_node_rows(o)
    assert len(want) == 73 and sum(len(v) % 2 for v in want.values()) > 20
    names = ("rgb", "intensity")
    rtc = [4.5e6, -1.25e5, 300.0]
    d_pack, d_host = tmp_path / "pack", tmp_path / "host"
    d_pack.mkdir()
    d_host.mkdir()

    dev = torch.device("cuda:0")
    with swz.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        d_xyz = torch.from_numpy(xyz).to(dev)
        d_attr = {"rgb": torch.from_numpy(rgb).to(dev), "intensity": torch.from_numpy(inten.view(np.int16)).to(dev)}
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        level = torch.empty(n, dtype=torch.int8, device=dev)
        ctx.tile_device(d_xyz.data_ptr(), n, *UNIT, swz.TileParams(sampler=sampler, max_points_per_node=500, spacing_at_root=spacing),
                        keys.data_ptr(), perm.data_ptr(), level.data_ptr())
        order = torch.empty(n, dtype=torch.int32, device=dev)
        nodes = ctx.build_node_lists_device(keys.data_ptr(), level.data_ptr(), n, order.data_ptr())
        ptrs = {k: v.data_ptr() for k, v in d_attr.items()}
        total = swz.pnts_layout(nodes["count"], names)["total"]
        image = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
        ctx.pnts_pack_device(perm.data_ptr(), order.data_ptr(), n, d_xyz.data_ptr(), ptrs, nodes, image.data_ptr(), total, attrs=names)
        ctx.pnts_persist_nodes(str(d_pack), nodes, image.cpu().numpy(), names, rtc_center=rtc)
        # the host path: gathered double rows, converted on the host
        out_xyz = torch.empty_like(d_xyz)
        out_attr = {k: torch.empty_like(v) for k, v in d_attr.items()}
        ctx.gather_payload_device(perm.data_ptr(), order.data_ptr(), n, d_xyz.data_ptr(), ptrs, out_xyz.data_ptr(),
                                  {k: v.data_ptr() for k, v in out_attr.items()})
        torch.cuda.synchronize()
        h_xyz = out_xyz.cpu().numpy()
        h_rgb, h_int = out_attr["rgb"].cpu().numpy(), out_attr["intensity"].cpu().numpy().view(np.uint16)
    for k in range(len(nodes["count"])):
        s = slice(int(nodes["offset"][k]), int(nodes["offset"][k] + nodes["count"][k]))
        name = swz.node_name(int(nodes["level"][k]), int(nodes["key"][k]))
        swz.pnts_write_node_rows(str(d_host / (name + ".pnts")), h_xyz[s], {"rgb": h_rgb[s], "intensity": h_int[s]}, rtc_center=rtc)
    tiles = swz.tileset_build(nodes["level"], nodes["key"], *UNIT, spacing, rtc)
    swz.tileset_write(tiles, str(d_pack))

    got = sorted(f for f in os.listdir(d_pack) if f.endswith(".pnts"))
    assert got == sorted(f + ".pnts" for f in want)
    for f in got:
        data = (d_pack / f).read_bytes()
        assert data == (d_host / f).read_bytes(), f
        head, arrays = _parse(data)
        rows = want[f[:-5]]
        assert head["POINTS_LENGTH"] == len(rows) and head["RTC_CENTER"] == rtc
        assert np.array_equal(arrays["xyz"], xyz[rows].astype(np.float32)), f
        assert np.array_equal(arrays["rgb"], rgb[rows]) and np.array_equal(arrays["intensity"], inten[rows]), f
    jsons = sorted(f for f in os.listdir(d_pack) if f.endswith(".json"))
    assert jsons == sorted(swz.node_name(t["level"], t["key"]) + ".json" for t in tiles if t["is_tileset_root"])
    assert "r.json" in jsons and json.loads((d_pack / "r.json").read_text())["root"]["content"]["uri"] == "r.pnts"


@pytest.mark.gpu
def test_gpu_fast_tiler_export_packed_straight_from_the_pools(tmp_path):
    """A FAST tiler fed three batches: its export ids are the perm (no order), the pools the source; reconstructed nodes
    store copies, so there are more stored rows than points."""
    import torch
    import schwarzwald_amd as swz
    rng = np.random.default_rng(32)
    n = 2_000       # about 6 000 node files, most of them of one point: hundreds of nodes inside one block
    xyz = rng.random((n, 3))
    rgb = rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8)
    inten = rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)
    spacing = O.spacing_from_diagonal(*UNIT, 32)
    t = O.Tiler(*UNIT, O.GRID_CENTER, 200, spacing, strategy=O.FAST, fast_concurrency=2)
    for part in np.array_split(xyz, 3):
        assert t.add_batch(part) == 0
    assert t.finalize() == 0
    ex = t.export()
    t.close()
    names = ("rgb", "intensity")
    params = swz.TileParams(sampler=swz.GRID_CENTER, max_points_per_node=200, spacing_at_root=spacing, strategy=swz.FAST, fast_concurrency=2)
    with swz.Context(0) as ctx:
        with swz.Tiler(ctx, *UNIT, params) as tl:
            for px, pr, pi in zip(np.array_split(xyz, 3), np.array_split(rgb, 3), np.array_split(inten, 3)):
                tl.add_batch(px, {"rgb": pr, "intensity": pi})
            tl.finalize()
            ns = int(tl.info()["num_stored"])
            assert ns > n
            table = tl.node_table()
            d_ids = torch.empty(ns, dtype=torch.int32, device="cuda:0")
            tl.export_device(None, d_ids.data_ptr(), None)
            pool_xyz, pool_attrs = tl.pools_device()
            total = swz.pnts_layout(table["count"], names)["total"]
            image = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            ctx.pnts_pack_device(d_ids.data_ptr(), None, ns, pool_xyz, pool_attrs, table, image.data_ptr(), total, attrs=names)
            ctx.pnts_persist_nodes(str(tmp_path), table, image.cpu().numpy(), names)
    assert np.array_equal(table["key"], ex["key"]) and np.array_equal(table["count"], ex["count"])
    assert len(os.listdir(tmp_path)) == len(ex["level"])
    for j in range(len(ex["level"])):
        ids = ex["ids"][int(ex["offset"][j]):int(ex["offset"][j] + ex["count"][j])]
        head, arrays = _parse((tmp_path / (swz.node_name(int(ex["level"][j]), int(ex["key"][j])) + ".pnts")).read_bytes())
        assert np.array_equal(arrays["xyz"], xyz[ids].astype(np.float32))
        assert np.array_equal(arrays["rgb"], rgb[ids]) and np.array_equal(arrays["intensity"], inten[ids])
