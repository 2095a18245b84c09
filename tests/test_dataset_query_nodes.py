"""swz_dataset_query_nodes (host only): which nodes of a written data set a box query reads, against a brute force over the
scanned table; the refusals by their words; the structs of the query against include/swz_gpu.h."""
import ctypes as C
import os

import numpy as np
import pytest

import schwarzwald_amd as swz
from schwarzwald_amd import api

ROOT = ([0.0, -2.0, 10.0], [4.0, 2.0, 14.0])
SIDE = 4.0
CELL = SIDE * 2.0 ** -21  # one key cell: the least a node box must be widened by
ERR_BAD_ARG = 2


def _key(digits):
    k = 0
    for l, d in enumerate(digits):
        k |= d << (3 * (20 - l))
    return k


# (octant digits, points): four levels, in no particular order
NODES = [((3, 1), 5), ((), 7), ((0,), 3), ((3,), 4), ((0, 7, 2), 1), ((3, 1, 0), 2), ((7,), 6), ((7, 7), 8), ((5, 2, 6), 3), ((4,), 2)]


def _write(directory, nodes=NODES, props=True):
    os.makedirs(directory, exist_ok=True)
    rng = np.random.default_rng(3)
    for digits, n in nodes:
        level, key = len(digits) - 1, _key(digits)
        lo, hi = swz.node_bounds(level, key, *ROOT)
        xyz = np.asarray(lo) + rng.random((n, 3)) * (np.asarray(hi) - np.asarray(lo))
        swz.bin_write_node(os.path.join(directory, swz.node_name(level, key) + ".bin"), xyz, dict(intensity=np.arange(n, dtype=np.uint16)))
    if props:
        swz.properties_json_write(directory, ROOT[0], ROOT[1], 0.5, sum(n for _, n in nodes))
    return directory


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return _write(str(tmp_path_factory.mktemp("query_nodes") / "bin"))


def _table(max_depth=None):
    return sorted((len(d) - 1, _key(d), n) for d, n in NODES if max_depth is None or len(d) <= max_depth)


def _meets(lo, hi, box, room=0.0):
    return all(lo[a] - room <= box[1][a] and box[0][a] <= hi[a] + room for a in range(3))


BOXES = [ROOT, ([9.0, 9.0, 9.0], [9.5, 9.5, 9.5]), ([0.0, -2.0, 10.0], [2.0, 0.0, 12.0]), ([2.0, 0.0, 12.0], [2.0, 0.0, 12.0]),
         ([3.1, 1.1, 10.1], [3.2, 1.2, 10.2]), ([0.0, -2.0, 13.99], [4.0, 2.0, 13.995]), ([2.0 + 3 * CELL, -2.0, 10.0], [4.0, 2.0, 14.0]),
         ([-1.0, -3.0, 9.0], [0.0 - 3 * CELL, 3.0, 15.0]), ([1.0, -1.5, 10.5], [1.0 + CELL, -1.5 + CELL, 10.5 + CELL])]


@pytest.mark.parametrize("max_depth", [None, 0, 1, 2])
@pytest.mark.parametrize("box", range(len(BOXES)))
def test_against_brute_force(data, box, max_depth):
    q = BOXES[box]
    got = swz.dataset_query_nodes(data, q[0], q[1], max_depth)
    kept = list(zip(got["level"].tolist(), got["key"].tolist(), got["count"].tolist()))
    table = _table(max_depth)
    assert kept == [row for row in table if row in kept]          # the scanned table's order, nothing invented
    assert got["points_bound"] == sum(r[2] for r in kept)
    for level, key, n in table:
        lo, hi = swz.node_bounds(level, key, *ROOT)
        if (level, key, n) not in kept:
            assert not _meets(lo, hi, q, CELL), "a dropped node's widened box meets the query box"
        if _meets(lo, hi, q):
            assert (level, key, n) in kept, "a node whose box meets the query box was dropped"


def test_whole_root_is_the_scan_and_far_is_empty(data):
    scan = swz.dataset_scan(data)
    got = swz.dataset_query_nodes(data, *ROOT)
    for k in ("level", "key", "count"):
        assert np.array_equal(got[k], scan["nodes"][k])
    assert got["points_bound"] == scan["points"] == sum(n for _, n in NODES)
    far = swz.dataset_query_nodes(data, [100.0, 100.0, 100.0], [101.0, 101.0, 101.0])
    assert len(far["level"]) == 0 and far["points_bound"] == 0
    shallow = swz.dataset_query_nodes(data, *ROOT, max_depth=1)
    assert shallow["level"].tolist() == [-1, 0, 0, 0, 0] and shallow["points_bound"] == 7 + 3 + 4 + 2 + 6


def test_one_key_cell_outside_a_node_still_reads_it(data):
    # a box that begins one key cell behind the node r3 on an axis, inside it on the others, keeps it; a distant one does not
    lo, hi = swz.node_bounds(0, _key((3,)), *ROOT)
    a = [hi[k] < ROOT[1][k] for k in range(3)].index(True)
    for gap, kept in ((CELL, True), (0.5, False)):
        q = ([lo[k] + 0.5 for k in range(3)], [hi[k] - 0.5 for k in range(3)])
        q[0][a], q[1][a] = hi[a] + gap, ROOT[1][a]
        got = swz.dataset_query_nodes(data, q[0], q[1])
        assert ((0, _key((3,))) in zip(got["level"].tolist(), got["key"].tolist())) == kept


def _refused(directory, *words, **kwargs):
    box = kwargs.pop("box", ROOT)
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_nodes(directory, box[0], box[1], **kwargs)
    assert e.value.code == ERR_BAD_ARG
    for w in ("swz_dataset_query_nodes",) + words:
        assert w in str(e.value), str(e.value)


def test_refusals(data, tmp_path):
    _refused(data, "box_min > box_max", box=([1.0, 0.0, 11.0], [0.5, 1.0, 12.0]))
    _refused(data, "not finite", box=([0.0, 0.0, float("nan")], [1.0, 1.0, 12.0]))
    _refused(data, "not finite", box=([0.0, 0.0, 10.0], [float("inf"), 1.0, 12.0]))
    _refused(data, "an unknown bit in source_flags", source_flags=2)
    _refused(data, "reserved must be 0", reserved=1)
    _refused(_write(str(tmp_path / "noroot"), props=False), "no root box")
    laz = _write(str(tmp_path / "laz"))
    open(os.path.join(laz, "r1.laz"), "wb").close()
    _refused(laz, "LAZ is not read")
    cloud = str(tmp_path / "cloud")
    os.makedirs(cloud)
    open(os.path.join(cloud, "cloud.js"), "w").close()
    _refused(cloud, "a cloud.js data set is not read")
    _refused(str(tmp_path / "missing"), "cannot read the directory")
    # .pnts sources: the flag, and one RTC_CENTER for all files
    pnts = str(tmp_path / "pnts")
    os.makedirs(pnts)
    xyz = np.array([[0.5, 0.5, 10.5], [1.0, 1.0, 11.0]])
    swz.pnts_write_node_rows(os.path.join(pnts, "r.pnts"), xyz, {}, rtc_center=(0.0, 0.0, 0.0))
    swz.pnts_write_node_rows(os.path.join(pnts, "r0.pnts"), xyz, {}, rtc_center=(0.0, 0.0, 0.0))
    swz.properties_json_write(pnts, ROOT[0], ROOT[1], 0.5, 4)
    _refused(pnts, "a 3DTILES source is converted only with SWZ_CONVERT_LOSSY_SOURCE in source_flags")
    assert swz.dataset_query_nodes(pnts, *ROOT, lossy_source=True)["points_bound"] == 4
    swz.pnts_write_node_rows(os.path.join(pnts, "r0.pnts"), xyz, {}, rtc_center=(1.0, 0.0, 0.0))
    _refused(pnts, "the RTC_CENTER differs from the files before it", "r0.pnts", lossy_source=True)


def test_pnts_boxes_are_relative_to_the_rtc_center(tmp_path):
    pnts = str(tmp_path / "pnts")
    os.makedirs(pnts)
    rtc = (1000.0, -500.0, 10.0)
    xyz = np.array([[0.5, -1.5, 10.5], [1.0, -1.0, 11.0]])
    for name in ("r", "r0", "r7"):
        swz.pnts_write_node_rows(os.path.join(pnts, name + ".pnts"), xyz, {}, rtc_center=rtc)
    swz.properties_json_write(pnts, ROOT[0], ROOT[1], 0.5, 6)
    # the stored positions are relative to RTC_CENTER, and so is the box of a query
    lo, hi = swz.node_bounds(0, _key((7,)), *ROOT)
    q = ([lo[a] - rtc[a] + 0.25 for a in range(3)], [hi[a] - rtc[a] - 0.25 for a in range(3)])
    got = swz.dataset_query_nodes(pnts, q[0], q[1], lossy_source=True)
    assert list(zip(got["level"].tolist(), got["key"].tolist())) == [(-1, 0), (0, _key((7,)))]
    assert len(swz.dataset_query_nodes(pnts, lo, hi, lossy_source=True)["level"]) == 0


def test_struct_layout():
    p, s = api._QueryParams, api._QueryStats
    assert C.sizeof(p) == 72
    assert [getattr(p, f).offset for f in ("box_min", "box_max", "max_depth", "attribute_mask", "source_flags", "reserved", "chunk_points")] \
        == [0, 24, 48, 52, 56, 60, 64]
    assert C.sizeof(s) == 88
    assert [getattr(s, f).offset for f in ("nodes_scanned", "nodes_read", "points_read", "points_out", "bytes_read", "chunks", "read_ms",
                                           "unpack_ms", "select_ms", "copy_ms", "wall_ms")] == list(range(0, 88, 8))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swz_gpu.h")).read()
    at = header.index("} swz_query_params;")
    body = header[header.rindex("typedef struct {", 0, at):at]
    order = [f for f in ("box_min", "box_max", "max_depth", "attribute_mask", "source_flags", "reserved", "chunk_points")]
    assert sorted(order, key=body.index) == order
    at = header.index("} swz_query_stats;")
    body = header[header.rindex("typedef struct {", 0, at):at]
    names = [f for f, _ in s._fields_]
    assert sorted(names, key=body.index) == names
