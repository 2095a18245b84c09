"""Oriented tile volumes (host only): swz_tileset_oriented_boxes against the recipe of the reference's
boundingBoxFromAABB(aabb, transform) (core/pointcloud/Tileset.cpp:52-92) written in numpy over srs_transform, and
swz_tileset_write_oriented against the boxes it was given and against swz_tileset_write for everything else.  No tolerance:
the library and the recipe run the same host map on the same doubles."""
import json
import os

import numpy as np
import pytest

import srs_ref as R

UTM32N = R.utm_definition(32, False)
UTM19S = R.utm_definition(19, True)
ROOTS = {UTM32N: ([499000.0, 5400000.0, 200.0], [500024.0, 5401024.0, 1224.0]),
         UTM19S: ([300000.25, 6000000.5, -10.0], [300900.25, 6000900.5, 890.0])}


def _table():
    """the root, three octants, two children of one of them and one grandchild: levels -1 .. 2"""
    level = np.array([-1, 0, 0, 0, 1, 1, 2], dtype=np.int8)
    key = np.array([0, 1 << 60, 6 << 60, 7 << 60, (6 << 60) | (0 << 57), (6 << 60) | (5 << 57), (6 << 60) | (5 << 57) | (3 << 54)],
                   dtype=np.uint64)
    return level, key


def _tiles(definition, **kw):
    import schwarzwald_amd as swz
    level, key = _table()
    lo, hi = ROOTS[definition]
    return swz.tileset_build(level, key, lo, hi, 8.0, **kw)


def _recipe(srs, tiles):
    import schwarzwald_amd as swz
    out = np.empty((len(tiles), 12))
    for i, t in enumerate(tiles):
        mn, mx = np.array(t["bounds_min"]), np.array(t["bounds_max"])
        c = mn + (mx - mn) / 2
        pts = np.array([c, [mx[0], c[1], c[2]], [c[0], mx[1], c[2]], [c[0], c[1], mx[2]]])
        if srs is not None:
            pts = swz.srs_transform(srs, pts)
        out[i] = np.concatenate([pts[0], pts[1] - pts[0], pts[2] - pts[0], pts[3] - pts[0]])
    return out


@pytest.mark.parametrize("definition", [UTM32N, UTM19S])
def test_oriented_boxes_are_the_four_point_recipe(definition):
    import schwarzwald_amd as swz
    tiles = _tiles(definition)
    assert len(tiles) == 7 and max(t["level"] for t in tiles) == 2
    got = swz.tileset_oriented_boxes(definition, tiles)
    want = _recipe(definition, tiles)
    assert got.shape == (7, 12) and (got == want).all()
    assert (got == swz.tileset_oriented_boxes(swz.Srs(definition), tiles)).all()
    # on the globe, and tilted: no axis of the box is an axis of ECEF
    assert (np.abs(np.linalg.norm(got[:, :3], axis=1) - 6.37e6) < 3e4).all() and (got[:, 3:] != 0).all()
    if definition == UTM19S:
        assert (got[:, 1] < 0).all() and (got[:, 2] < 0).all()
    # the axes have the lengths of the half extents to a part in a thousand (k_0, the height above the ellipsoid)
    half = np.array([(np.array(t["bounds_max"]) - np.array(t["bounds_min"])) / 2 for t in tiles])
    length = np.linalg.norm(got[:, 3:].reshape(-1, 3, 3), axis=2)
    assert np.abs(length / half - 1).max() < 2e-3


def test_without_a_projection_centre_and_half_extents():
    import schwarzwald_amd as swz
    tiles = _tiles(UTM19S)
    got = swz.tileset_oriented_boxes(None, tiles)
    for row, t in zip(got, tiles):
        mn, mx = np.array(t["bounds_min"]), np.array(t["bounds_max"])
        c = mn + (mx - mn) / 2
        assert (row[:3] == c).all()
        assert (row[3:].reshape(3, 3) == np.diag(mx - c)).all()
    assert (got == _recipe(None, tiles)).all()


def test_refusals():
    import schwarzwald_amd as swz
    tiles = _tiles(UTM32N)
    with pytest.raises(swz.SwzError):
        swz.tileset_oriented_boxes("+proj=merc +datum=WGS84", tiles)
    with pytest.raises(ValueError):
        swz.tileset_write_oriented(tiles, np.zeros((len(tiles), 11)), "unused")
    bad = swz.tileset_oriented_boxes(UTM32N, tiles)
    bad[3, 7] = np.inf
    with pytest.raises(swz.SwzError):
        swz.tileset_write_oriented(tiles, bad, "unused")


def _walk(tile, out):
    out[tile["content"]["uri"]] = tile
    for child in tile.get("children", []):
        _walk(child, out)


def _read(directory):
    """file name -> (the parsed JSON, its tiles by content.uri)"""
    files = {}
    for f in sorted(os.listdir(directory)):
        assert f.endswith(".json")
        doc = json.load(open(os.path.join(directory, f)))
        tiles = {}
        _walk(doc["root"], tiles)
        files[f] = (doc, tiles)
    return files


def _without_boxes(node):
    if isinstance(node, dict):
        return {k: _without_boxes(v) for k, v in node.items() if k != "boundingVolume"}
    if isinstance(node, list):
        return [_without_boxes(v) for v in node]
    return node


@pytest.mark.parametrize("tight", [False, True])
def test_write_oriented(tmp_path, tight):
    import schwarzwald_amd as swz
    level, key = _table()
    lo, hi = ROOTS[UTM32N]
    kw = {}
    if tight:   # boxes of "points" well inside the cubes; the node r1 holds none
        plain = swz.tileset_build(level, key, lo, hi, 8.0)
        by_node = {(t["level"], t["key"]): t for t in plain}
        mn = np.array([np.array(by_node[(int(l), int(k))]["bounds_min"]) + 1.5 for l, k in zip(level, key)])
        mx = np.array([np.array(by_node[(int(l), int(k))]["bounds_max"]) - 2.25 for l, k in zip(level, key)])
        mn[1], mx[1] = np.inf, -np.inf
        kw = dict(node_boxes=(mn, mx))
    tiles = swz.tileset_build(level, key, lo, hi, 8.0, **kw)
    obb = swz.tileset_oriented_boxes(UTM32N, swz.tileset_build(level, key, lo, hi, 8.0))
    if tight:
        assert [bool(t["tight"]) for t in tiles] == [True, False, True, True, True, True, True]
    a, b = tmp_path / "oriented", tmp_path / "plain"
    a.mkdir()
    b.mkdir()
    swz.tileset_write_oriented(tiles, obb, str(a))
    swz.tileset_write(tiles, str(b))
    got, plain = _read(str(a)), _read(str(b))
    assert sorted(got) == sorted(plain) == ["r.json", "r653.json"]
    seen = 0
    for f in got:
        assert _without_boxes(got[f][0]) == _without_boxes(plain[f][0])     # geometricError, uris, children, asset
        for uri, tile in got[f][1].items():
            i = next(j for j, t in enumerate(tiles) if swz.node_name(t["level"], t["key"]) == uri.rsplit(".", 1)[0])
            box = tile["boundingVolume"]["box"]
            if tiles[i].get("tight"):
                assert box == plain[f][1][uri]["boundingVolume"]["box"] and box[4] == box[5] == box[6] == 0
            else:
                assert box == [float(repr(float(v))) for v in obb[i]]
            seen += 1
    assert seen == 8    # the seven entries, the file root r653 twice
