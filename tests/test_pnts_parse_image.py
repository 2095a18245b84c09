"""swz_pnts_parse_image: where the arrays of a .pnts file image are (host only, no GPU).

Files of the library's own writer must parse to what swz_pnts_layout says; hand-made images (another array order, unknown
members, a batch table, a JSON whose length is no multiple of 8) must parse to offsets that find the right bytes; every
refusal is checked on an image cut to its last valid byte minus one, so a parser that reads past the image would be caught by
the allocator's guard or give a different answer."""
import ctypes as C
import struct

import numpy as np
import pytest

ERR_BAD_ARG = 2


def _file(json_text, binary, pad_to=8, length=None, magic=b"pnts", version=1, batch_json=b"", batch_binary=b""):
    text = json_text.encode()
    text += b" " * (-len(text) % pad_to)
    total = 28 + len(text) + len(binary) + len(batch_json) + len(batch_binary)
    head = magic + struct.pack("<6I", version, total if length is None else length, len(text), len(binary), len(batch_json), len(batch_binary))
    return head + text + binary + batch_json + batch_binary


def _parse_exact(data):
    """the image in an allocation of exactly its size"""
    import schwarzwald_amd as swz
    return swz.pnts_parse_image(np.frombuffer(bytes(data), dtype=np.uint8).copy())


@pytest.mark.parametrize("attrs", [(), ("rgb",), ("intensity",), ("rgb", "intensity")])
@pytest.mark.parametrize("n", [1, 2, 7, 100])
def test_written_files_parse_to_the_layout(tmp_path, attrs, n):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(n)
    xyz = rng.random((n, 3)) * 100
    cols = {"rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
            "intensity": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)}
    path = str(tmp_path / "r.pnts")
    swz.pnts_write_node_rows(path, xyz, cols, write=list(attrs), rtc_center=(10.5, -3.25, 1e6))
    data = open(path, "rb").read()
    got = _parse_exact(data)
    lay = swz.pnts_layout([n], attrs)
    json_bytes, binary_bytes = struct.unpack_from("<2I", data, 12)
    base = 28 + json_bytes
    assert binary_bytes == lay["size"][0] == lay["total"]
    assert got["count"] == n and got["attrs"] == list(attrs) and got["rtc_center"] == [10.5, -3.25, 1e6]
    assert got["position_offset"] == base
    assert got["rgb_offset"] == (base + int(lay["rgb_offset"][0]) if "rgb" in attrs else 0)
    assert got["intensity_offset"] == (base + int(lay["intensity_offset"][0]) if "intensity" in attrs else 0)
    # and the bytes there are the rows
    assert np.array_equal(np.frombuffer(data, "<f4", 3 * n, got["position_offset"]).reshape(n, 3), xyz.astype(np.float32))
    if "rgb" in attrs:
        assert np.array_equal(np.frombuffer(data, np.uint8, 3 * n, got["rgb_offset"]).reshape(n, 3), cols["rgb"])
    if "intensity" in attrs:
        assert np.array_equal(np.frombuffer(data[got["intensity_offset"]:got["intensity_offset"] + 2 * n], "<u2"), cols["intensity"])
    # the readers agree
    rx, rc, rtc = swz.pnts_read_node(path)
    assert np.array_equal(rx, xyz.astype(np.float32).astype(np.float64)) and sorted(rc) == sorted(attrs)


def _foreign(n=5):
    rng = np.random.default_rng(8)
    xyz = rng.random((n, 3)).astype(np.float32)
    rgb = rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8)
    inten = rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)
    binary = bytearray(b"\xEE" * 123)
    binary[3:13] = inten.tobytes()         # INTENSITY at 3: an odd address
    binary[14:29] = rgb.tobytes()          # RGB at 14
    binary[41:101] = xyz.tobytes()         # POSITION at 41
    return xyz, rgb, inten, bytes(binary)


@pytest.mark.parametrize("pad_to", [1, 8, 32])
def test_foreign_images(pad_to):
    """INTENSITY, RGB, POSITION in that order with gaps, an unknown member with nested values, a batch table, and (pad_to 1) a
    JSON of 8 k + 3 bytes, so that the binary begins at an odd offset of the file"""
    xyz, rgb, inten, binary = _foreign()
    text = ('{ "INTENSITY" : {"byteOffset": 3, "componentType": "UNSIGNED_SHORT"},\n "extras": {"a": [1, {"b": null}], "s": "q\\"}"},'
            ' "RGB": {"byteOffset":14}, "RTC_CENTER": [1.5, -2e3, 0.25], "POSITION": {"byteOffset": 41}, "POINTS_LENGTH": 5, "ok": true,'
            ' "NORMAL": {"byteOffset": 7}}')
    if pad_to == 1:
        text += " " * ((3 - len(text)) % 8)
        assert len(text) % 8 == 3
    batch_json = b'{"id":{"byteOffset":0,"componentType":"UNSIGNED_INT","type":"SCALAR"}} '
    data = _file(text, binary, pad_to=pad_to, batch_json=batch_json, batch_binary=bytes(range(20)))
    got = _parse_exact(data)
    assert got["count"] == 5 and got["attrs"] == ["rgb", "intensity"] and got["rtc_center"] == [1.5, -2000.0, 0.25]
    assert np.array_equal(np.frombuffer(data[got["position_offset"]:][:60], "<f4").reshape(5, 3), xyz)
    assert np.array_equal(np.frombuffer(data[got["rgb_offset"]:][:15], np.uint8).reshape(5, 3), rgb)
    assert np.array_equal(np.frombuffer(data[got["intensity_offset"]:][:10], "<u2"), inten)
    base = 28 + struct.unpack_from("<I", data, 12)[0]
    assert (got["position_offset"], got["rgb_offset"], got["intensity_offset"]) == (base + 41, base + 14, base + 3)


def test_refusals_on_images_cut_to_the_byte(tmp_path):
    """every refusal, the image ending one byte in front of the last byte that would make it valid (or at the last byte the
    check looks at); the outputs are not touched"""
    import schwarzwald_amd as swz
    L = swz.load_library()
    good_json = '{"POINTS_LENGTH":3,"RTC_CENTER":[0,0,0],"POSITION":{"byteOffset":0},"RGB":{"byteOffset":36},"INTENSITY":{"byteOffset":46}}'
    binary = bytes(56)
    good = _file(good_json, binary)
    assert _parse_exact(good)["count"] == 3
    quant = good_json.replace('"POSITION"', '"POSITION_QUANTIZED"')
    cases = {
        "empty image": (b"", "shorter"),
        "short image": (good[:27], "shorter"),
        "good but one byte short": (good[:-1], "add up"),
        "wrong magic": (_file(good_json, binary, magic=b"b3dm"), "magic"),
        "unknown version": (_file(good_json, binary, version=2), "version"),
        "byteLength larger than the image": (_file(good_json, binary, length=len(good) + 1), "add up"),
        "trailing byte": (good + b"\0", "add up"),
        "json length passes the image": (good[:12] + struct.pack("<I", 1 << 20) + good[16:], "add up"),
        "binary length passes the image": (good[:16] + struct.pack("<I", 1 << 30) + good[20:], "add up"),
        "batch table that passes the image": (good[:20] + struct.pack("<I", 1) + good[24:], "add up"),
        "position passes the binary by one": (_file(good_json.replace('"byteOffset":0', '"byteOffset":21'), binary), "passes the end"),
        "rgb passes the binary by one": (_file(good_json.replace("36", "48"), binary), "passes the end"),
        "intensity passes the binary by one": (_file(good_json.replace("46", "51"), binary), "passes the end"),
        "binary one byte too small": (_file(good_json.replace("46", "50"), binary[:-1]), "passes the end"),
        "count too large for the binary": (_file(good_json.replace('"POINTS_LENGTH":3', '"POINTS_LENGTH":4000000000'), binary), "passes the end"),
        "negative offset": (_file(good_json.replace("36", "-4"), binary), "passes the end"),
        "json cut off": (_file(good_json[:-20], binary), "feature-table JSON"),
        "json not an object": (_file("[1,2,3]", binary), "feature-table JSON"),
        "no POINTS_LENGTH": (_file(good_json.replace("POINTS_LENGTH", "POINTS"), binary), "feature-table JSON"),
        "unterminated string": (_file('{"POINTS_LENGTH', binary), "feature-table JSON"),
        "deep nesting": (_file('{"a":' + "[" * 5000 + "]" * 5000 + "}", binary), "feature-table JSON"),
        "POSITION_QUANTIZED only": (_file(quant, binary), "POSITION"),
    }
    for name, (data, word) in cases.items():
        buf = np.frombuffer(bytes(data), dtype=np.uint8).copy() if data else np.zeros(1, np.uint8)
        outs = [C.c_uint64(77), C.c_uint32(77), (C.c_double * 3)(7, 7, 7), C.c_uint64(77), C.c_uint64(77), C.c_uint64(77)]
        st = L.swz_pnts_parse_image(None, C.c_void_p(buf.ctypes.data), len(data), C.byref(outs[0]), C.byref(outs[1]), outs[2],
                                    C.byref(outs[3]), C.byref(outs[4]), C.byref(outs[5]))
        assert st == ERR_BAD_ARG, name
        assert [o.value for o in outs[:2] + outs[3:]] == [77] * 5 and list(outs[2]) == [7, 7, 7], name
        with pytest.raises(swz.SwzError):
            swz.pnts_parse_image(bytes(data))
        # the text: the scan of a directory that holds the file reports the same check's words (a context needs a GPU)
        if len(data) >= 1:
            d = tmp_path / ("case%d" % len(list(tmp_path.iterdir())))
            d.mkdir()
            (d / "r.pnts").write_bytes(data)
            with pytest.raises(swz.SwzError) as e:
                swz.dataset_scan(str(d))
            assert word in str(e.value) and "r.pnts" in str(e.value), (name, str(e.value))
    # the binary that is just large enough is taken
    assert _parse_exact(_file(good_json.replace("46", "50"), binary))["intensity_offset"] == 28 + len(good) - 28 - 56 + 50
