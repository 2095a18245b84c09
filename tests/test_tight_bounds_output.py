"""swz_tiler_write_output with SWZ_OUT_TIGHT_BOUNDS: about 6 000 points on a thin, tilted sheet inside the unit root box, tiled
in two batches with a small max_points_per_node, so that the tree has at least three levels and every octree cube is mostly
empty.  Every format that holds a box is written with and without the flag: the point data must not change by a byte, the
metadata must change in the boxes only, and the boxes must be those of the points -- enclosing (checked against every point
of a tile and of all its descendants, read back from the files), nested, and TIGHT: every face of a leaf's box is touched by
a stored point, which no cube of this sheet does.

Tolerances.  That every point lies inside is exact and inclusive.  A tileset box is [centre, half-axes]: a face is centre -/+
half evaluated in double, two roundings away from the extreme point (the centre's and the face's), and swz_tileset_write may
widen a half-axis by a few ulps so that the face encloses; so "touched" allows 4 ulp of the larger of |centre| and half, and
so does "a child's face lies inside its parent's" -- the two faces are rounded apart when they share the extreme point.  The
LAS header, the Entwine bounds and Tiler.node_boxes are compared with ==."""
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
GLOBAL_OFFSET = (1000.5, -20.25, 3.0)
ERR_BAD_ARG = 2
COLUMNS = ("rgb", "intensity")


def _sheet():
    rng = np.random.default_rng(31337)
    n = 6000
    xy = rng.random((n, 2))
    z = 0.25 + 0.45 * xy[:, 0] + 0.2 * xy[:, 1] + 0.004 * (rng.random(n) - 0.5)  # tilted, 0.4 % of the box thick
    xyz = np.column_stack([xy, z])
    cols = {"rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
            "intensity": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)}
    return xyz, cols


def _listing(top):
    out = {}
    for base, _, files in os.walk(top):
        for f in files:
            out[os.path.relpath(os.path.join(base, f), top)] = os.path.join(base, f)
    return out


def _read(path):
    with open(path, "rb") as f:
        return f.read()


EPT = dict(bounds=UNIT, conforming_bounds=UNIT, points=6000, attrs=COLUMNS, span=128, srs=dict(authority="EPSG", horizontal="25832"),
           version="1.0.0")


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """the tiler, and every format written without the flag, with it, and with it in the smallest chunks"""
    import torch
    import schwarzwald_amd as swz
    top = tmp_path_factory.mktemp("tight")
    xyz, cols = _sheet()
    with swz.Context(0) as ctx:
        params = swz.TileParams(sampler=swz.SAMPLERS["RANDOM_GRID"], max_points_per_node=48,
                                spacing_at_root=swz.spacing_from_diagonal(*UNIT, 12), strategy=swz.ACCURATE)
        t = swz.Tiler(ctx, UNIT[0], UNIT[1], params)
        half = len(xyz) // 2
        t.add_batch(xyz[:half], {a: c[:half] for a, c in cols.items()})
        t.add_batch(xyz[half:], {a: c[half:] for a, c in cols.items()})  # the second batch reaches the files of the first
        t.finalize()
        info, nodes = t.info(), t.node_table()
        assert info["num_batches"] == 2 and int(nodes["level"].max()) >= 2 and len(nodes["count"]) >= 50
        dirs = {}
        for fmt in ("3DTILES", "LAS", "ENTWINE_LAS"):
            for leg, tight in (("plain", False), ("tight", True)):
                dirs[fmt, leg] = str(top / (fmt + "_" + leg))
                t.write_output(dirs[fmt, leg], fmt, attrs=COLUMNS, global_offset=GLOBAL_OFFSET, tight_bounds=tight,
                               ept=EPT if fmt == "ENTWINE_LAS" else None)
        boxes = t.node_boxes()
        # the pools and the export ids, for the boxes the long way
        d_ids = torch.empty(int(info["num_stored"]), dtype=torch.int32, device="cuda:0")
        t.export_device(None, d_ids.data_ptr(), None)
        torch.cuda.synchronize()
        ids = d_ids.cpu().numpy().view(np.uint32)
        pool_ptr, _ = t.pools_device()
        pool = ctx.copy_to_host(pool_ptr, int(info["num_points"]) * 24).view(np.float64).reshape(-1, 3)
        # the smallest chunks the call cuts (a chunk is never smaller than the largest node): many chunks, two images in turn
        ctx.set_option("SWZ_OUTPUT_CHUNK_POINTS", "1")
        assert len(swz.output_chunks(nodes["count"], 1)) - 1 >= len(nodes["count"]) // 4
        for fmt in ("3DTILES", "ENTWINE_LAS"):
            dirs[fmt, "chunks"] = str(top / (fmt + "_chunks"))
            t.write_output(dirs[fmt, "chunks"], fmt, attrs=COLUMNS, global_offset=GLOBAL_OFFSET, tight_bounds=True,
                           ept=EPT if fmt == "ENTWINE_LAS" else None)
        boxes_chunks = t.node_boxes()
        # the refusals through the call itself, and the tiler takes another write afterwards
        refusals = []
        for fmt, kw in (("BIN", dict(tight_bounds=True)), ("BINZ", dict(tight_bounds=True)), ("LAS", dict(flags=2)),
                        ("3DTILES", dict(tight_bounds=True, flags=8))):
            with pytest.raises(swz.SwzError) as e:
                t.write_output(str(top / "refused"), fmt, attrs=COLUMNS, **kw)
            refusals.append((fmt, kw, e.value.code, str(e.value)))
        assert not os.path.exists(str(top / "refused"))
        dirs["LAS", "again"] = str(top / "LAS_again")
        t.write_output(dirs["LAS", "again"], "LAS", attrs=COLUMNS, tight_bounds=True)
        t.close()
    return dict(dirs=dirs, nodes=nodes, boxes=boxes, boxes_chunks=boxes_chunks, ids=ids, pool=pool, refusals=refusals)


def test_node_boxes_are_min_max_over_the_pools(written):
    W = written
    nodes, ids, pool = W["nodes"], W["ids"], W["pool"]
    lo, hi = W["boxes"]
    assert lo.shape == hi.shape == (len(nodes["count"]), 3)
    for k in range(len(nodes["count"])):
        o, c = int(nodes["offset"][k]), int(nodes["count"][k])
        assert c > 0
        rows = pool[ids[o:o + c]]
        assert (lo[k] == rows.min(axis=0)).all() and (hi[k] == rows.max(axis=0)).all(), k
    assert (W["boxes_chunks"][0] == lo).all() and (W["boxes_chunks"][1] == hi).all()


def _strip(doc):
    if isinstance(doc, dict):
        return {k: _strip(v) for k, v in doc.items() if k != "boundingVolume"}
    if isinstance(doc, list):
        return [_strip(v) for v in doc]
    return doc


def test_3dtiles_point_files_do_not_change_and_the_json_only_in_the_boxes(written):
    plain, tight = _listing(written["dirs"]["3DTILES", "plain"]), _listing(written["dirs"]["3DTILES", "tight"])
    assert sorted(plain) == sorted(tight)
    pnts = [f for f in plain if f.endswith(".pnts")]
    assert len(pnts) == len(written["nodes"]["count"]) and len(plain) > len(pnts)
    changed = 0
    for f in sorted(plain):
        a, b = _read(plain[f]), _read(tight[f])
        if f.endswith(".pnts"):
            assert a == b, f
            continue
        assert f.endswith(".json")
        da, db = json.loads(a), json.loads(b)
        assert _strip(da) == _strip(db), f
        changed += da != db
    assert changed == len(plain) - len(pnts)  # every tileset file holds a box of this sheet, and every such box shrank


def _tileset(directory):
    """name -> box, name -> names of its children, from every tileset file of the directory"""
    boxes, children = {}, {}

    def walk(tile):
        name = tile["content"]["uri"].rsplit(".", 1)[0]
        box = tile["boundingVolume"]["box"]
        assert boxes.setdefault(name, box) == box, name  # the entry at the bottom of a file is the root of the next
        if "children" in tile:
            children[name] = [walk(ch) for ch in tile["children"]]
        return name

    for f in os.listdir(directory):
        if f.endswith(".json"):
            walk(json.loads(_read(os.path.join(directory, f)))["root"])
    return boxes, children


@pytest.mark.parametrize("leg", ["tight", "chunks"])
def test_3dtiles_boxes_enclose_nest_and_touch(written, leg):
    import schwarzwald_amd as swz
    directory = written["dirs"]["3DTILES", leg]
    nodes = written["nodes"]
    files = {swz.node_name(int(lv), int(key)) for lv, key in zip(nodes["level"], nodes["key"])}
    points = {}
    for name in files:
        xyz, _, rtc = swz.pnts_read_node(os.path.join(directory, name + ".pnts"))
        assert rtc == list(GLOBAL_OFFSET)
        points[name] = xyz + np.array(GLOBAL_OFFSET)  # the boxes are translated by the offset, the positions are not
    boxes, children = _tileset(directory)
    assert files <= set(boxes) and max(len(n) for n in boxes) >= 4
    leaves = 0
    for name, box in boxes.items():
        assert [box[k] for k in range(3, 12) if (k - 3) % 4] == [0.0] * 6
        centre, half = np.array(box[:3]), np.array([box[3], box[7], box[11]])
        lo, hi = centre - half, centre + half
        below = np.concatenate([points[f] for f in files if f.startswith(name)])  # its own points and all its descendants'
        assert len(below) and (lo <= below).all() and (below <= hi).all(), name
        tol = np.array([4 * math.ulp(max(abs(centre[a]), half[a])) for a in range(3)])
        for child in children.get(name, []):
            c, h = np.array(boxes[child][:3]), np.array([boxes[child][3], boxes[child][7], boxes[child][11]])
            assert (lo - tol <= c - h).all() and (c + h <= hi + tol).all(), (name, child)
        if name in files and not any(f != name and f.startswith(name) for f in boxes):
            leaves += 1
            own = points[name]
            for a in range(3):
                assert own[:, a].min() - lo[a] <= tol[a] and hi[a] - own[:, a].max() <= tol[a], (name, a)
    assert leaves >= 20
    # a cube fails tightness: the same check on the unflagged tileset finds loose faces on every leaf
    loose, _ = _tileset(written["dirs"]["3DTILES", "plain"])
    name = max(files, key=len)
    own = points[name]
    assert any(own[:, a].min() - (loose[name][a] - loose[name][3 + 4 * a] / 2) > 1e-4 for a in range(3))


def test_chunked_output_is_the_same_directory(written):
    for fmt in ("3DTILES", "ENTWINE_LAS"):
        a, b = _listing(written["dirs"][fmt, "tight"]), _listing(written["dirs"][fmt, "chunks"])
        assert sorted(a) == sorted(b)
        for f in a:
            assert _read(a[f]) == _read(b[f]), (fmt, f)


@pytest.mark.parametrize("fmt", ["LAS", "ENTWINE_LAS"])
def test_las_files_change_in_the_48_bytes_of_the_extent_only(written, fmt):
    import schwarzwald_amd as swz
    plain, tight = _listing(written["dirs"][fmt, "plain"]), _listing(written["dirs"][fmt, "tight"])
    assert sorted(plain) == sorted(tight)
    las = [f for f in plain if f.endswith(".las")]
    assert len(las) == len(written["nodes"]["count"])
    lo_all, hi_all = np.full(3, np.inf), np.full(3, -np.inf)
    for f in sorted(plain):
        a, b = _read(plain[f]), _read(tight[f])
        if not f.endswith(".las"):
            if os.path.basename(f) != "ept.json":
                assert a == b, f
            continue
        assert a[:179] == b[:179] and a[227:] == b[227:] and a[179:227] != b[179:227], f
        head, (xyz, _) = swz.las_read_header(tight[f]), swz.las_read_node(tight[f])
        assert head["min"] == list(xyz.min(axis=0)) and head["max"] == list(xyz.max(axis=0)), f
        assert head["offset"] == swz.las_read_header(plain[f])["offset"]
        lo_all, hi_all = np.minimum(lo_all, head["min"]), np.maximum(hi_all, head["max"])
    if fmt == "ENTWINE_LAS":
        was, now = json.loads(_read(plain["ept.json"])), json.loads(_read(tight["ept.json"]))
        assert now["bounds"] == was["bounds"] == UNIT[0] + UNIT[1]
        assert was["boundsConforming"] == UNIT[0] + UNIT[1]
        assert now["boundsConforming"] == list(lo_all) + list(hi_all)
        assert {k: v for k, v in now.items() if k != "boundsConforming"} == {k: v for k, v in was.items() if k != "boundsConforming"}


def test_flags_are_refused_by_the_call_and_the_tiler_goes_on(written):
    for fmt, kw, code, text in written["refusals"]:
        assert code == ERR_BAD_ARG and "swz_tiler_write_output" in text, (fmt, kw, text)
        assert ("OUT_TIGHT_BOUNDS" if fmt in ("BIN", "BINZ") else "unknown flag bit") in text, (fmt, kw, text)
    a, b = _listing(written["dirs"]["LAS", "tight"]), _listing(written["dirs"]["LAS", "again"])
    assert sorted(a) == sorted(b) and all(_read(a[f]) == _read(b[f]) for f in a)
