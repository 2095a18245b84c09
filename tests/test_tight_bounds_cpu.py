"""The host parts of SWZ_OUT_TIGHT_BOUNDS (no GPU): swz_tileset_build_boxes -- the tileset tree with the boxes of the points
instead of the octree cubes, united bottom-up --, swz_tileset_write's half-axes for the entries it marks, the text it
writes for every other entry, which must stay what it was, swz_las_stored_box, and the refusals of the flags."""
import json
import math
import os

import numpy as np
import pytest

import schwarzwald_amd as swz
from schwarzwald_amd import api

ROOT_BOX = ((-8.0, 0.0, 16.0), (24.0, 32.0, 48.0))
SPACING = 0.75
OFFSET = (432100.25, -5412345.5, 310.125)
INF = float("inf")


def _key(octants):
    key = 0
    for level, o in enumerate(octants):
        key |= o << ((20 - level) * 3)
    return key


# three levels below the root; r30 is in no table: an ancestor without a file.  r312 holds no point.
TABLE = {"r": (), "r3": (3,), "r31": (3, 1), "r301": (3, 0, 1), "r306": (3, 0, 6), "r312": (3, 1, 2), "r5": (5,)}
BOXES = {"r": ((1.0, 2.0, 20.0), (3.0, 30.0, 21.0)),  # (the boxes need not lie inside the cubes: the union is what is tested)
         "r3": ((-1.5, 17.0, 30.0), (0.25, 18.0, 30.0)),  # flat in z
         "r31": ((4.0, 20.0, 40.0), (5.0, 21.0, 41.0)),
         "r301": ((-7.0, 16.5, 33.0), (-6.0, 16.75, 35.0)),
         "r306": ((-3.0, 19.0, 32.5), (-2.0, 19.5, 32.75)),
         "r312": ((INF, INF, INF), (-INF, -INF, -INF)),
         "r5": ((10.0, 1.0, 47.0), (23.0, 1.0, 47.5))}
NAMES = sorted(TABLE, key=lambda n: (len(n), n))


def _table():
    levels = np.array([len(TABLE[n]) - 1 for n in NAMES], dtype=np.int8)
    keys = np.array([_key(TABLE[n]) for n in NAMES], dtype=np.uint64)
    lo = np.array([BOXES[n][0] for n in NAMES], dtype=np.float64)
    hi = np.array([BOXES[n][1] for n in NAMES], dtype=np.float64)
    return levels, keys, lo, hi


def _union(names, offset):
    lo = [min(BOXES[n][0][a] for n in names) + offset[a] for a in range(3)]
    hi = [max(BOXES[n][1][a] for n in names) + offset[a] for a in range(3)]
    return lo, hi


@pytest.mark.parametrize("offset", [None, OFFSET])
def test_boxes_are_united_bottom_up_and_shifted(offset):
    levels, keys, lo, hi = _table()
    tiles = swz.tileset_build(levels, keys, *ROOT_BOX, SPACING, offset, node_boxes=(lo, hi))
    cubes = swz.tileset_build(levels, keys, *ROOT_BOX, SPACING, offset)
    by_name = {swz.node_name(t["level"], t["key"]): t for t in tiles}
    assert set(by_name) == set(TABLE) | {"r30"} and len(tiles) == len(cubes)
    off = offset or (0.0, 0.0, 0.0)
    for name, t in by_name.items():
        if name == "r312":
            continue
        below = [n for n in TABLE if n.startswith(name) and n != "r312"]  # itself (if it has a file) and all descendants
        want = _union(below, off)
        assert t["tight"] and (t["bounds_min"], t["bounds_max"]) == want, name
    # the ancestor without a file is exactly the union of its children
    assert not by_name["r30"]["has_content"]
    assert (by_name["r30"]["bounds_min"], by_name["r30"]["bounds_max"]) == _union(["r301", "r306"], off)
    # a node without a point and without descendants keeps its cube and is not marked
    cube = {swz.node_name(t["level"], t["key"]): t for t in cubes}["r312"]
    assert not by_name["r312"]["tight"]
    assert (by_name["r312"]["bounds_min"], by_name["r312"]["bounds_max"]) == (cube["bounds_min"], cube["bounds_max"])
    # everything but the boxes is swz_tileset_build's, and a parent encloses its children
    for t, c in zip(tiles, cubes):
        for field in ("level", "key", "has_content", "is_tileset_root", "num_children", "parent", "first_child", "geometric_error"):
            assert t[field] == c[field]
        if t["parent"] >= 0 and t["tight"]:
            p = tiles[t["parent"]]
            assert all(p["bounds_min"][a] <= t["bounds_min"][a] and t["bounds_max"][a] <= p["bounds_max"][a] for a in range(3))


def _tiles_of(doc, out):
    out.append(doc)
    for child in doc.get("children", []):
        _tiles_of(child, out)
    return out


def test_marked_entries_are_written_with_half_axes(tmp_path):
    levels, keys, lo, hi = _table()
    tiles = swz.tileset_build(levels, keys, *ROOT_BOX, SPACING, OFFSET, node_boxes=(lo, hi))
    swz.tileset_write(tiles, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["r.json", "r301.json", "r306.json", "r312.json"]
    seen = {}
    for f in os.listdir(tmp_path):
        for tile in _tiles_of(json.loads((tmp_path / f).read_text())["root"], []):
            name = tile["content"]["uri"].rsplit(".", 1)[0]
            seen.setdefault(name, []).append(tile["boundingVolume"]["box"])
    by_name = {swz.node_name(t["level"], t["key"]): t for t in tiles}
    assert set(seen) == set(by_name)
    for name, boxes in seen.items():
        t = by_name[name]
        for box in boxes:
            assert [box[k] for k in range(3, 12) if (k - 3) % 4] == [0.0] * 6
            for a in range(3):
                mn, mx = t["bounds_min"][a], t["bounds_max"][a]
                centre, axis = box[a], box[3 + 4 * a]
                assert centre == mn + (mx - mn) / 2
                if not t["tight"]:
                    assert axis == mx - mn  # the cube, the FULL extent: as the reference writes it
                    continue
                # the half extent, at most a few ulps of the centre wider, and centre -/+ half encloses the bounds
                assert centre - axis <= mn and mx <= centre + axis
                assert (mx - mn) / 2 <= axis <= (mx - mn) / 2 + 4 * math.ulp(max(abs(centre), axis))


def test_unmarked_entries_are_written_as_before(tmp_path):
    """flag 0 must not change a byte: the files of the unchanged tileset_build path, and of a boxes tree whose marks are
    taken off and whose bounds are put back, are the text this library has always written (pinned against a formula)."""
    levels, keys, lo, hi = _table()
    cubes = swz.tileset_build(levels, keys, *ROOT_BOX, SPACING, OFFSET)
    assert all("tight" not in t for t in cubes)
    plain, again = tmp_path / "plain", tmp_path / "again"
    plain.mkdir(), again.mkdir()
    swz.tileset_write(cubes, str(plain))
    boxed = swz.tileset_build(levels, keys, *ROOT_BOX, SPACING, OFFSET, node_boxes=(lo, hi))
    for t, c in zip(boxed, cubes):
        t["tight"], t["bounds_min"], t["bounds_max"] = False, c["bounds_min"], c["bounds_max"]
    swz.tileset_write(boxed, str(again))
    assert sorted(os.listdir(plain)) == sorted(os.listdir(again)) == ["r.json", "r301.json", "r306.json", "r312.json"]
    for f in os.listdir(plain):
        assert (plain / f).read_bytes() == (again / f).read_bytes()
    root = json.loads((plain / "r.json").read_text())["root"]
    e = [ROOT_BOX[1][a] - ROOT_BOX[0][a] for a in range(3)]
    assert root["boundingVolume"]["box"] == [ROOT_BOX[0][a] + OFFSET[a] + e[a] / 2 for a in range(3)] + [e[0], 0, 0, 0, e[1], 0, 0, 0, e[2]]


def test_bad_boxes_are_refused():
    levels, keys, lo, hi = _table()
    with pytest.raises(ValueError):
        swz.tileset_build(levels, keys, *ROOT_BOX, SPACING, node_boxes=(lo[:-1], hi))


def test_las_stored_box_is_the_quantised_box():
    offset, scale = (10.0, -3.0, 0.5), 0.001
    lo, hi = (10.12345, -2.99951, 0.5), (11.9996, -2.0, 0.50049)
    got = swz.las_stored_box(lo, hi, offset, scale)
    q = lambda v, o: o + float(int((v - o) / scale + 0.5)) * scale  # noqa: E731  (I32_QUANTIZE of a non-negative quotient)
    assert got == ([q(lo[a], offset[a]) for a in range(3)], [q(hi[a], offset[a]) for a in range(3)])
    assert got[0][2] == 0.5 and got[1][2] == 0.5  # both corners of a thin axis may land on one record value
    with pytest.raises(ValueError):
        swz.las_stored_box(lo, hi, offset, 0.0)


def test_flags_are_refused_by_name():
    for fmt in ("BIN", "BINZ"):
        with pytest.raises(swz.SwzError, match="OUT_TIGHT_BOUNDS") as e:
            api.output_flags_check(fmt, swz.OUT_TIGHT_BOUNDS)
        assert e.value.code == 2
    for fmt in swz.OUTPUT_FORMATS:
        for flags in (2, 0x80000000, swz.OUT_TIGHT_BOUNDS | 4):
            with pytest.raises(swz.SwzError, match="unknown flag bit") as e:
                api.output_flags_check(fmt, flags)
            assert e.value.code == 2
        api.output_flags_check(fmt, 0)
    for fmt in ("3DTILES", "LAS", "ENTWINE_LAS"):
        api.output_flags_check(fmt, swz.OUT_TIGHT_BOUNDS)


def test_the_flags_took_the_padding_of_the_params():
    import ctypes as C
    p = api._OutputParams
    assert C.sizeof(p) == 56
    assert [getattr(p, f).offset for f in ("format", "attribute_mask", "rgb_mapping", "flags", "global_offset", "chunk_points", "ept")] \
        == [0, 4, 8, 12, 16, 40, 48]
