"""swz_dataset_query_region_nodes (host only): which nodes of a written data set a query by planes or by polygon reads.

Safety: a node any of whose lattice points passes the region's formula (tests/region_ref.py) is kept.  Effect: nodes inside the
region's bounding box, but a node side clear of the region, are dropped.  The refusals by their words."""
import itertools
import os

import numpy as np
import pytest

import region_ref as R
import schwarzwald_amd as swz

ROOT = ([0.0, -2.0, 10.0], [4.0, 2.0, 14.0])
SIDE = 4.0
CELL = SIDE * 2.0 ** -21
ERR_BAD_ARG = 2


def _key(digits):
    k = 0
    for l, d in enumerate(digits):
        k |= d << (3 * (20 - l))
    return k


def _cells():
    """(depth, ix, iy, iz) -> octant digits, read off swz.node_bounds"""
    out = {}
    for depth in range(4):
        for digits in itertools.product(range(8), repeat=depth):
            lo, _ = swz.node_bounds(depth - 1, _key(digits), *ROOT)
            cell = tuple(int(round((lo[a] - ROOT[0][a]) / (SIDE / 2 ** depth))) for a in range(3))
            out[(depth,) + cell] = digits
    return out


CELLS = _cells()
# the root, the 8 octants, the 64 nodes below them and the lower layer (iz == 0) of the 512 below those
NODES = [d for (depth, ix, iy, iz), d in sorted(CELLS.items()) if depth < 3 or iz == 0]


def _xy(unit):
    """a shape of the unit square in the root's x-y"""
    return np.asarray(unit) * SIDE + np.array([ROOT[0][0], ROOT[0][1]])


PLANE_DIAGONAL = [[1.0, 1.0, 0.0, -2.0]]                                  # x + y >= 2: the corner towards (0, -2) is cut off
REGIONS = {"diagonal": ("planes", PLANE_DIAGONAL),
           "wedge": ("planes", [[1.0, 1.0, 0.0, -2.0], [-1.0, 0.5, 0.0, 2.5], [0.0, 0.0, 1.0, -11.0], [0.3, -0.2, -1.0, 12.5]]),
           "square": ("polygon", _xy(R.SQUARE)), "L": ("polygon", _xy(R.L_SHAPE)), "U": ("polygon", _xy(R.U_SHAPE)),
           "bow_tie": ("polygon", np.array([[0.0, -2.0], [4.0, 2.0], [4.0, -2.0], [0.0, 2.0]])),
           "circle": ("polygon", _xy(R.circle(64, radius=0.3)))}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    directory = str(tmp_path_factory.mktemp("query_region_nodes") / "bin")
    os.makedirs(directory)
    for digits in NODES:
        lo, hi = swz.node_bounds(len(digits) - 1, _key(digits), *ROOT)
        xyz = (np.asarray(lo) + np.asarray(hi))[None, :] / 2
        swz.bin_write_node(os.path.join(directory, swz.node_name(len(digits) - 1, _key(digits)) + ".bin"), xyz, {})
    swz.properties_json_write(directory, ROOT[0], ROOT[1], 0.5, len(NODES))
    return directory


def _bbox(region):
    if region[0] == "polygon":
        v = np.asarray(region[1])
        return ([v[:, 0].min(), v[:, 1].min(), ROOT[0][2]], [v[:, 0].max(), v[:, 1].max(), ROOT[1][2]])
    return ROOT


def _kept(got):
    return set(zip(got["level"].tolist(), got["key"].tolist()))


def _lattice(lo, hi, per_axis=(9, 9, 3)):
    axes = [np.linspace(lo[a], hi[a], per_axis[a]) for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


@pytest.mark.parametrize("max_depth", [None, 0, 1, 2])
@pytest.mark.parametrize("name", list(REGIONS))
def test_a_node_that_holds_a_row_of_the_region_is_kept(data, name, max_depth):
    region = REGIONS[name]
    box = _bbox(region)
    got = swz.dataset_query_region_nodes(data, box[0], box[1], R.as_region(swz, region), max_depth)
    kept = _kept(got)
    table = [d for d in NODES if max_depth is None or len(d) <= max_depth]
    by_box = _kept(swz.dataset_query_nodes(data, box[0], box[1], max_depth))
    assert kept <= by_box <= {(len(d) - 1, _key(d)) for d in table}
    assert got["points_bound"] == len(kept) and len(got["level"]) == len(kept)
    holding = 0
    for d in table:
        lo, hi = swz.node_bounds(len(d) - 1, _key(d), *ROOT)
        if R.region_mask(_lattice(lo, hi), box, region).any():
            holding += 1
            assert (len(d) - 1, _key(d)) in kept, "a node that holds a row of the region was dropped"
    assert holding >= 1
    if max_depth is None and name not in ("square", "U"):   # (the square is its own bounding box; every node of the U's notch touches an edge)
        assert len(kept) < len(by_box), "the region drops nothing the box keeps"


def _node(depth, ix, iy, iz=0):
    d = CELLS[(depth, ix, iy, iz)]
    return (len(d) - 1, _key(d))


def test_nodes_clear_of_the_region_inside_its_bounding_box_are_dropped(data):
    # inside the L's notch (x in (2, 3), y in (0, 1)): the node [2.5, 3] x [0.5, 1] is half a unit clear of both edges
    L = REGIONS["L"]
    kept = _kept(swz.dataset_query_region_nodes(data, *_bbox(L), swz.Region.polygon(L[1])))
    assert _node(3, 5, 5) in _kept(swz.dataset_query_nodes(data, *_bbox(L)))
    assert _node(3, 5, 5) not in kept and _node(3, 4, 4) in kept and _node(3, 3, 3) in kept
    # and without a box: the polygon's x-y bounds, the root's z
    assert _kept(swz.dataset_query_region_nodes(data, None, None, swz.Region.polygon(L[1]))) == kept
    # beyond the diagonal plane: the node [0, 1] x [-2, -1] has x + y <= 0 < 2
    kept = _kept(swz.dataset_query_region_nodes(data, *ROOT, swz.Region.planes(PLANE_DIAGONAL)))
    for iz in range(4):
        assert _node(2, 0, 0, iz) not in kept and _node(2, 3, 3, iz) in kept
    assert _node(3, 0, 0) not in kept and _node(3, 3, 4) in kept          # [1.5, 2] x [0, 0.5] touches x + y = 2
    assert (-1, 0) in kept
    # inside the bow-tie's outer wedges: [1.5, 2] x [1, 1.5] lies above both diagonals, half a unit clear
    bow = REGIONS["bow_tie"]
    kept = _kept(swz.dataset_query_region_nodes(data, *ROOT, swz.Region.polygon(bow[1])))
    assert _node(3, 3, 6) not in kept and _node(3, 4, 1) not in kept     # above and below the crossing
    assert _node(3, 1, 4) in kept and _node(3, 6, 3) in kept             # left and right of it
    assert _node(3, 3, 4) in kept                                         # a diagonal runs through its corner


def test_one_key_cell_outside_a_plane_still_reads_the_node(data):
    level, key = _node(1, 0, 0, 0)                                        # x in [0, 2]
    for gap, kept in ((CELL, True), (0.5, False)):
        got = swz.dataset_query_region_nodes(data, *ROOT, swz.Region.planes([[1.0, 0.0, 0.0, -(2.0 + gap)]]))
        assert ((level, key) in _kept(got)) == kept
    # the same through a polygon: its left edge one key cell, then half a unit, behind the node
    for gap, kept in ((CELL, True), (0.5, False)):
        x = 2.0 + gap
        got = swz.dataset_query_region_nodes(data, *ROOT, swz.Region.polygon([[x, -2.0], [4.0, -2.0], [4.0, 2.0], [x, 2.0]]))
        assert ((level, key) in _kept(got)) == kept


def test_pnts_nodes_are_culled_relative_to_the_rtc_center(tmp_path):
    pnts = str(tmp_path / "pnts")
    os.makedirs(pnts)
    rtc = np.array([1000.0, -500.0, 10.0])
    xyz = np.array([[0.5, -1.5, 10.5], [1.0, -1.0, 11.0]])
    names = {"r": (), "r0": CELLS[(1, 0, 0, 0)], "r7": CELLS[(1, 1, 1, 1)]}
    for digits in names.values():
        swz.pnts_write_node_rows(os.path.join(pnts, swz.node_name(len(digits) - 1, _key(digits)) + ".pnts"), xyz, {}, rtc_center=tuple(rtc))
    swz.properties_json_write(pnts, ROOT[0], ROOT[1], 0.5, 6)
    far = (0, _key(names["r7"]))
    lo, hi = swz.node_bounds(*far, *ROOT)
    box = ((np.asarray(ROOT[0]) - rtc).tolist(), (np.asarray(ROOT[1]) - rtc).tolist())
    # a triangle well inside the far octant, given relative to RTC_CENTER as the stored positions are
    tri = np.array([[lo[0] + 0.5, lo[1] + 0.5], [hi[0] - 0.5, lo[1] + 0.5], [lo[0] + 1.0, hi[1] - 0.5]]) - rtc[:2]
    got = swz.dataset_query_region_nodes(pnts, box[0], box[1], swz.Region.polygon(tri), lossy_source=True)
    assert _kept(got) == {(-1, 0), far}
    plane = [[1.0, 0.0, 0.0, -(lo[0] + 0.5 - rtc[0])]]                     # x >= the octant's face + 0.5, relative
    assert _kept(swz.dataset_query_region_nodes(pnts, box[0], box[1], swz.Region.planes(plane), lossy_source=True)) == {(-1, 0), far}
    # the same outline in absolute coordinates is nowhere near the stored positions
    absolute = swz.dataset_query_region_nodes(pnts, box[0], box[1], swz.Region.polygon(tri + rtc[:2]), lossy_source=True)
    assert len(absolute["level"]) == 0


def _refused(directory, region, *words, **kwargs):
    box = kwargs.pop("box", ROOT)
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_region_nodes(directory, box[0], box[1], region, **kwargs)
    assert e.value.code == ERR_BAD_ARG
    for w in ("swz_dataset_query_region_nodes",) + words:
        assert w in str(e.value), str(e.value)


def test_refusals(data, tmp_path):
    plane, tri = [[1.0, 0.0, 0.0, 0.0]], [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]
    missing = str(tmp_path / "missing")                                   # a refused region reads no file: the directory is not missed
    for directory in (data, missing):
        _refused(directory, swz.Region(7, plane), "an unknown kind of region")
        _refused(directory, swz.Region(swz.REGION_POLYGON, tri, reserved=2), "the region's reserved must be 0")
        _refused(directory, swz.Region(swz.REGION_PLANES, plane, count=0), "a region of planes holds 1 to 16 of them")
        _refused(directory, swz.Region.planes(np.tile(plane, (17, 1))), "a region of planes holds 1 to 16 of them")
        _refused(directory, swz.Region.polygon(tri[:2]), "a polygon region holds 3 to 1024 vertices")
        _refused(directory, swz.Region.polygon(R.circle(1025)), "a polygon region holds 3 to 1024 vertices")
        _refused(directory, swz.Region(swz.REGION_PLANES, None, count=2), "a region with NULL values")
        _refused(directory, swz.Region.planes([[1.0, float("nan"), 0.0, 0.0]]), "a coefficient of a plane is not finite")
        _refused(directory, swz.Region.polygon(tri[:2] + [[0.0, float("inf")]]), "a vertex of the polygon is not finite")
        _refused(directory, swz.Region.planes([[0.0, 0.0, 0.0, 1.0]]), "a plane with a = b = c = 0")
        _refused(directory, swz.Region(swz.REGION_BOX, None, count=3), "a box region with a count that is not 0")
    # what the box query refuses, in its words
    _refused(data, swz.Region.polygon(tri), "box_min > box_max", box=([1.0, 0.0, 11.0], [0.5, 1.0, 12.0]))
    _refused(data, swz.Region.planes(plane), "not finite", box=([0.0, 0.0, float("nan")], [1.0, 1.0, 12.0]))
    _refused(data, swz.Region.planes(plane), "an unknown bit in source_flags", source_flags=2)
    _refused(data, swz.Region.planes(plane), "reserved must be 0", reserved=1)
    _refused(missing, swz.Region.planes(plane), "cannot read the directory")
    with pytest.raises(ValueError):
        swz.dataset_query_region_nodes(data, None, None, swz.Region.planes(plane))   # planes need the box


def test_box_region_and_none_are_the_box_query(data):
    box = ([0.5, -1.5, 10.0], [2.5, 0.25, 12.0])
    want = swz.dataset_query_nodes(data, *box)
    for region in (None, swz.Region.box()):
        got = swz.dataset_query_region_nodes(data, box[0], box[1], region)
        assert all(np.array_equal(got[k], want[k]) for k in ("level", "key", "count")) and got["points_bound"] == want["points_bound"]
