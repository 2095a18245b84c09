"""FAST (TilingAlgorithmV3) at every start level S = 3 .. 6, on clouds built to vote for one.

estimate_start_level_host (swz_session.hip) answers 6 for every cloud with fewer than 100 000 points per range, so uniform test
clouds run the level bookkeeping of FAST at S = 6 only: tiling from node level S - 1, session_fast_reconstruct's loop over the
levels S - 1 .. 0 with child_bit 0 for the first rebuilt level and 1 << (lv + 1) for the others, the multi-batch tiler that keeps
the S of its first batch, and a shard that stops the reconstruction at level 1.

sibling_cloud puts all points into two cells with d octant digits that differ in one digit.  With 100 000 points in each and
fast_concurrency = 2 every depth above the differing digit sees one range (score 0), the depth of the differing digit sees two
ranges of which two are large (score 2 / 2 = 1): S = max(that depth, 3).  One point fewer in a cell, or one thread more, and no
depth reaches the score: S = 6.

The tests without the gpu mark check, on the oracle alone, that every cloud really is its hard case -- the start level, a tree
with two levels below the start nodes, a start node that hands points down -- so that no choice of spacing can hide a failure
of the device code."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import test_shard_seams as seams
from test_multibatch import _compare as compare_node_files
from test_shard_seams import cloud_files, driver  # noqa: F401  (module fixtures: the single-process group driver and its clouds)

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
SAMPLERS = [O.RANDOM_GRID, O.GRID_CENTER, O.MIN_DISTANCE, O.JITTERED]  # those of test_tile_fast_matches_oracle
LARGE = 100000  # a range counts as large from this many points on
AXES = {"x": 4, "y": 2, "z": 1}  # the bit an axis sets in an octant digit


def cell_box(digits):
    """(lower corner, side) of the unit box's cell with these octant digits, root's child first."""
    lo, side = np.zeros(3), 1.0
    for g in digits:
        side *= 0.5
        lo += side * np.array([(g >> 2) & 1, (g >> 1) & 1, g & 1], dtype=np.float64)
    return lo, side


def sibling_path(path, axis, digit):
    """path with the bit of axis flipped in its digit-th digit (1 = the root's children)."""
    other = list(path)
    other[digit - 1] ^= AXES[axis]
    return other


def sibling_cloud(d, na, nb, seed, path=None, axis="x", digit=None):
    """na points uniform in the cell `path` (d octant digits; default: the cell at the origin), nb in the cell that differs from
    it along `axis` in digit number `digit` (1-based; default d: the two are children of one node), each cell shrunk by 1 % per
    face so that no point sits on a cell's face; rows in random order."""
    rng = np.random.default_rng(seed)
    path = [0] * d if path is None else list(path)
    assert len(path) == d
    digit = d if digit is None else digit
    parts = []
    for digits, n in ((path, na), (sibling_path(path, axis, digit), nb)):
        lo, side = cell_box(digits)
        parts.append(lo + side * (0.01 + 0.98 * rng.random((n, 3))))
    xyz = np.vstack(parts)
    return xyz[rng.permutation(xyz.shape[0])]


def prefix_of(digits):
    v = 0
    for g in digits:
        v = (v << 3) | g
    return v


DEEP_PATH = [5, 2, 7, 1, 6, 3]
# name -> (path of the first cell, axis, how many digits above the last one the two cells differ)
LAYOUTS = {
    "x pair at the origin": (lambda d: [0] * d, "x", 0),
    "z pair deep inside": (lambda d: DEEP_PATH[:d], "z", 0),
    "y pair of cousins": (lambda d: DEEP_PATH[::-1][:d], "y", 1),  # the parents differ: the vote is one level higher
}
# spacing = diagonal / SPACING_DIV, max_points_per_node: a start node of 100 000 points keeps some 8 000 and hands the rest
# to children that sample again, whose children take all (checked on the oracle below)
SPACING_DIV, MAX_POINTS = 32, 2000
# the clouds that vote 6: a start node is a 64th or an 8th of a cell (some 1 560 or 12 500 points)
THRESHOLD_DIV, THRESHOLD_MAX_POINTS = 32, 50
THRESHOLD_PAIRS = [(LARGE, LARGE - 1, 2), (LARGE, LARGE, 3)]


def layout_cloud_args(d, layout):
    path, axis, up = LAYOUTS[layout]
    return dict(path=path(d), axis=axis, digit=d - up)


def expected_start_level(d, layout):
    return max(d - LAYOUTS[layout][2], 3)


@functools.lru_cache(maxsize=None)
def layout_cloud(d, layout, na=LARGE, nb=LARGE):
    xyz = sibling_cloud(d, na, nb, 10 * d + len(layout), **layout_cloud_args(d, layout))
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def oracle_tile(cloud, sampler, concurrency=2, div=SPACING_DIV, max_points=MAX_POINTS):
    """The oracle's FAST tiling of a cloud (the arguments of one of the cached cloud functions), computed once."""
    xyz = cloud[0](*cloud[1:])
    o = O.tile(xyz, *UNIT, sampler, max_points, O.spacing_from_diagonal(*UNIT, div), strategy=O.FAST, fast_concurrency=concurrency)
    for a in (o["keys"], o["perm"], o["level"], o["dup"]):
        a.setflags(write=False)
    return o


def assert_two_levels_below_a_sampling_start_node(o, S):
    """The spacing condition, on the oracle's output alone: levels S and S + 1 exist (two below the start nodes at S - 1), and a
    start node keeps some of its points and hands others down."""
    assert o["status"] == 0
    level, keys = o["level"], o["keys"]
    assert int(level.min()) == S - 1 and int(level.max()) >= S + 1
    node = keys >> np.uint64(63 - 3 * S)
    handed_down = np.unique(node[level > S - 1])
    kept = np.unique(node[level == S - 1])
    assert np.intersect1d(kept, handed_down).size >= 1


def assert_fast_result(g, o, S):
    """ctx.tile's result is the oracle's, and the level bookkeeping is that of start level S by number."""
    assert g.stats["fast_start_levels"] == S
    assert o["stats"]["fast_start_levels"] == S
    assert np.array_equal(g.keys, o["keys"]) and np.array_equal(g.perm, o["perm"])
    assert np.array_equal(g.level, o["level"])
    assert np.array_equal(g.dup, o["dup"])
    assert g.stats["num_nodes"] == o["stats"]["num_nodes"]
    assert_fast_bookkeeping(g.level, g.dup, S)


def assert_fast_bookkeeping(level, dup, S):
    assert int(level.min()) == S - 1                      # tiling starts at node level S - 1
    assert int(dup.max()) < (1 << S)                      # the rebuilt levels are S - 2 .. -1: bits S - 1 .. 0
    assert int((dup == (1 << S) - 1).sum()) >= 1          # a point the root took was taken by every level on the way up
    for bit in range(S - 1):                              # a node samples from what its children took
        assert not np.any(((dup >> bit) & 1) & ~((dup >> (bit + 1)) & 1))
    assert np.all(level[dup != 0] == S - 1)               # and the first rebuilt level from the start nodes' own points


# ------------------------------------------------------------------------------------------ CPU: the clouds are their hard cases
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("d", [3, 4, 5, 6])
def test_sibling_cloud_fills_two_cells_that_differ_in_one_digit(d, layout):
    args = layout_cloud_args(d, layout)
    xyz = layout_cloud(d, layout)
    assert xyz.shape[0] <= 200000
    keys, clamped = O.index_points(xyz, *UNIT)
    assert np.array_equal(clamped, xyz)
    cells, counts = np.unique(keys >> np.uint64(63 - 3 * d), return_counts=True)
    a, b = prefix_of(args["path"]), prefix_of(sibling_path(args["path"], args["axis"], args["digit"]))
    assert sorted(cells.tolist()) == sorted([a, b]) and counts.tolist() == [LARGE, LARGE]
    shift = 3 * (d - args["digit"])
    assert (a ^ b) == AXES[args["axis"]] << shift         # one digit, one axis
    lo, side = cell_box(args["path"])
    inside = xyz[(keys >> np.uint64(63 - 3 * d)) == np.uint64(a)]
    assert inside.shape[0] == LARGE and np.all(inside > lo) and np.all(inside < lo + side)  # off every face


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("d", [3, 4, 5, 6])
def test_oracle_votes_the_engineered_level_and_samples_below_it(d, layout, sampler):
    S = expected_start_level(d, layout)
    o = oracle_tile((layout_cloud, d, layout), sampler)
    assert o["stats"]["fast_start_levels"] == S
    assert_two_levels_below_a_sampling_start_node(o, S)
    assert_fast_bookkeeping(o["level"], o["dup"], S)


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("na,nb,concurrency", THRESHOLD_PAIRS)
@pytest.mark.parametrize("d", [4, 5])
def test_oracle_votes_six_one_point_or_one_thread_off(d, na, nb, concurrency, sampler):
    o = oracle_tile((layout_cloud, d, "x pair at the origin", na, nb), sampler, concurrency, THRESHOLD_DIV, THRESHOLD_MAX_POINTS)
    assert o["stats"]["fast_start_levels"] == 6
    assert_two_levels_below_a_sampling_start_node(o, 6)


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def _params(sampler, concurrency=2, div=SPACING_DIV, max_points=MAX_POINTS, flags=0):
    import schwarzwald_amd as swz
    return swz.TileParams(sampler=sampler, max_points_per_node=max_points, spacing_at_root=O.spacing_from_diagonal(*UNIT, div),
                          strategy=swz.FAST, fast_concurrency=concurrency, flags=flags)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("d", [3, 4, 5, 6])
def test_tile_fast_matches_oracle_at_every_start_level(ctx, d, layout, sampler):
    """Reconstruction loops of 3, 4, 5 and 6 levels, dup masks of exactly S bits."""
    S = expected_start_level(d, layout)
    o = oracle_tile((layout_cloud, d, layout), sampler)
    g = ctx.tile(layout_cloud(d, layout), *UNIT, _params(sampler))
    print("d = %d, %s, %s: S = %d on the GPU, %d on the oracle" % (d, layout, O.SAMPLER_NAMES[sampler], g.stats["fast_start_levels"],
                                                                    o["stats"]["fast_start_levels"]))
    assert_fast_result(g, o, S)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 4, 5, 6])
def test_tile_fast_property_mode_at_every_start_level(ctx, d):
    """SWZ_FLAG_MIN_DISTANCE_PROPERTY has no counterpart in the oracle (the set it takes is its own): keys, order and start level
    are the oracle's, and the level bookkeeping must be that of S = d all the same."""
    import schwarzwald_amd as swz
    layout = "z pair deep inside"
    o = oracle_tile((layout_cloud, d, layout), O.MIN_DISTANCE)
    g = ctx.tile(layout_cloud(d, layout), *UNIT, _params(O.MIN_DISTANCE, flags=swz.FLAG_MIN_DISTANCE_PROPERTY))
    assert g.stats["fast_start_levels"] == d == o["stats"]["fast_start_levels"]
    assert np.array_equal(g.keys, o["keys"]) and np.array_equal(g.perm, o["perm"])
    assert int(g.level.max()) >= d + 1
    assert_fast_bookkeeping(g.level, g.dup, d)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("na,nb,concurrency", THRESHOLD_PAIRS)
@pytest.mark.parametrize("d", [4, 5])
def test_tile_fast_threshold_pair_on_the_device_path(ctx, d, na, nb, concurrency, sampler):
    """prefix_bounds_kernel feeds the estimate here: 99 999 points in a cell are not a large range, and two large ranges are
    not enough for three threads."""
    cloud = (layout_cloud, d, "x pair at the origin", na, nb)
    o = oracle_tile(cloud, sampler, concurrency, THRESHOLD_DIV, THRESHOLD_MAX_POINTS)
    g = ctx.tile(cloud[0](*cloud[1:]), *UNIT, _params(sampler, concurrency, THRESHOLD_DIV, THRESHOLD_MAX_POINTS))
    assert_fast_result(g, o, 6)


@functools.lru_cache(maxsize=None)
def corner_cloud(d, corner):
    """A sibling cloud whose first cell touches a corner of the bounds -- it holds bin 0 or bin 2^18 - 1 of the 8^6 prefix
    histogram --, with rows exactly on that corner's coordinates: 20 on the corner, 20 with x alone, 20 with y and z."""
    g = 0 if corner == "origin" else 7
    value = 0.0 if corner == "origin" else 1.0
    xyz = sibling_cloud(d, LARGE, LARGE, 60 + d + g, path=[g] * d, axis="x")
    lo, side = cell_box([g] * d)
    rows = np.flatnonzero(np.all((xyz > lo) & (xyz < lo + side), axis=1))
    assert rows.size == LARGE
    xyz[rows[:20]] = value
    xyz[rows[20:40], 0] = value
    xyz[rows[40:60], 1:] = value
    xyz.setflags(write=False)
    return xyz


@pytest.mark.parametrize("corner", ["origin", "far"])
@pytest.mark.parametrize("d", [5, 6])
def test_corner_clouds_fill_the_first_and_the_last_bin(d, corner):
    """Rows on bounds.min and bounds.max keep to the corner cells (the key clamps to the last cell), so that the corner cell
    holds exactly 100 000 points: one fewer in the first or the last range of the histogram and d = 5 votes 6."""
    xyz = corner_cloud(d, corner)
    keys, clamped = O.index_points(xyz, *UNIT)
    assert np.array_equal(clamped, xyz)
    edge = UNIT[0] if corner == "origin" else UNIT[1]
    assert int(np.all(xyz == edge, axis=1).sum()) == 20 and int(np.any(xyz == edge[0], axis=1).sum()) == 60
    bins = (keys >> np.uint64(45)).astype(np.int64)
    corner_bin = 0 if corner == "origin" else (1 << 18) - 1
    assert int(bins.min() if corner == "origin" else bins.max()) == corner_bin
    assert int((bins == corner_bin).sum()) >= 20
    cells, counts = np.unique(bins >> (3 * (6 - d)), return_counts=True)
    corner_cell = corner_bin >> (3 * (6 - d))
    assert cells.tolist() == sorted([corner_cell, corner_cell ^ 4]) and counts.tolist() == [LARGE, LARGE]
    for sampler in (O.RANDOM_GRID, O.MIN_DISTANCE):
        o = oracle_tile((corner_cloud, d, corner), sampler)
        assert o["stats"]["fast_start_levels"] == d
        assert_two_levels_below_a_sampling_start_node(o, d)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", [O.RANDOM_GRID, O.MIN_DISTANCE])
@pytest.mark.parametrize("corner", ["origin", "far"])
@pytest.mark.parametrize("d", [5, 6])
def test_tile_fast_keys_at_the_edges_of_the_bins(ctx, d, corner, sampler):
    """The first and the last entry of prefix_bounds_kernel's starts and its end sentinel decide the count of the corner cell."""
    o = oracle_tile((corner_cloud, d, corner), sampler)
    g = ctx.tile(corner_cloud(d, corner), *UNIT, _params(sampler))
    assert_fast_result(g, o, d)
    assert np.array_equal(g.xyz_clamped.view(np.uint64), o["xyz_clamped"].view(np.uint64))


# ------------------------------------------------------------------------------------------ the multi-batch tiler keeps its first S
MB_PATH = [5, 2, 7, 1, 6]


@functools.lru_cache(maxsize=None)
def tiler_batches(first):
    """Three batches: a d = 4 cloud, 3 000 uniform points, a d = 5 cloud inside the first one's cell (its points meet files that
    exist); first = 5: the d = 5 cloud comes first."""
    a = sibling_cloud(4, LARGE, LARGE, 41, path=MB_PATH[:4], axis="x")
    b = np.random.default_rng(42).random((3000, 3))
    c = sibling_cloud(5, LARGE, LARGE, 43, path=MB_PATH, axis="x")
    batches = (a, b, c) if first == 4 else (c, b, a)
    for x in batches:
        x.setflags(write=False)
    return batches


def batch_votes(first):
    return (4, 6, 5) if first == 4 else (5, 6, 4)


@functools.lru_cache(maxsize=None)
def oracle_tiler_files(first, sampler):
    """(export, counts, S after every batch) of the multi-batch oracle on tiler_batches(first)."""
    t = O.Tiler(*UNIT, sampler, MAX_POINTS, O.spacing_from_diagonal(*UNIT, SPACING_DIV), strategy=O.FAST, fast_concurrency=2)
    seen = []
    for part in tiler_batches(first):
        assert t.add_batch(part) == 0
        seen.append(t.stats()["fast_start_levels"])
    assert t.finalize() == 0
    ex, c = t.export(), t.counts()
    t.close()
    return ex, c, tuple(seen)


@pytest.mark.parametrize("first", [4, 5])
def test_oracle_tiler_keeps_the_vote_of_its_first_batch(first):
    for part, vote in zip(tiler_batches(first), batch_votes(first)):
        alone = O.tile(part, *UNIT, O.RANDOM_GRID, MAX_POINTS, O.spacing_from_diagonal(*UNIT, SPACING_DIV), strategy=O.FAST,
                       fast_concurrency=2)
        assert alone["status"] == 0 and alone["stats"]["fast_start_levels"] == vote
    ex, c, seen = oracle_tiler_files(first, O.RANDOM_GRID)
    assert seen == (first, first, first)
    assert int(ex["level"].min()) == -1 and int(ex["level"].max()) >= first + 1
    assert c["unsorted_cached_nodes"] == 0


def _gpu_tiler_files(ctx, first, sampler, staged):
    """test_multibatch._gpu_files on batches of unequal sizes, with the tiler's info read after every batch."""
    import schwarzwald_amd as swz
    import torch
    seen = []
    with swz.Tiler(ctx, UNIT[0], UNIT[1], _params(sampler)) as t:
        parts = tiler_batches(first)
        if staged:
            pinned = []
            for p in parts:
                a = swz.pinned_empty(p.shape, np.float64)
                a[...] = p
                pinned.append(a)
            t.stage_batch(pinned[0])
            for i in range(len(parts)):
                if i + 1 < len(parts):
                    t.stage_batch(pinned[i + 1])
                seen.append((t.tile_staged()["fast_start_levels"], t.info()["fast_start_levels"]))
        else:
            for p in parts:
                d = torch.from_numpy(np.array(p)).cuda()  # (a copy: the cached batches are read-only)
                torch.cuda.synchronize()
                seen.append((t.add_batch_device(d.data_ptr(), p.shape[0])["fast_start_levels"], t.info()["fast_start_levels"]))
        t.finalize()
        info = t.info()
        table = t.node_table()
        ns = int(info["num_stored"])
        d_ids = torch.empty(max(ns, 1), dtype=torch.int32, device="cuda")
        d_lvl = torch.empty(max(ns, 1), dtype=torch.int8, device="cuda")
        t.export_device(None, d_ids.data_ptr(), d_lvl.data_ptr())
        ids = d_ids.cpu().numpy().view(np.uint32)[:ns]
        lvl = d_lvl.cpu().numpy()[:ns]
    return dict(table=table, ids=ids, level=lvl, info=info), seen


@pytest.mark.gpu
@pytest.mark.parametrize("staged", [False, True], ids=["device", "staged"])
@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("first", [4, 5])
def test_tiler_keeps_the_start_level_of_its_first_batch(ctx, first, sampler, staged):
    """fast_start in swz_tiler.hip is voted once: a later batch that alone would vote 6, 5 or 4 is split at the first batch's
    level, and finalize rebuilds the levels first - 1 .. 0.  The node files are the multi-batch oracle's, node for node, id for
    id, in file order."""
    ex, c, oracle_seen = oracle_tiler_files(first, sampler)
    assert oracle_seen == (first, first, first)
    g, seen = _gpu_tiler_files(ctx, first, sampler, staged)
    assert seen == [(first, first)] * 3
    assert g["info"]["fast_start_levels"] == first and g["info"]["num_batches"] == 3
    assert g["info"]["rekey_inversions"] == 0 and c["unsorted_cached_nodes"] == 0
    compare_node_files(g, ex, c)


# ------------------------------------------------------------------------------------------ shards
@pytest.mark.gpu
def test_shard_set_start_level_accepts_one_to_six_once(ctx):
    import schwarzwald_amd as swz
    fixed = "swz_tiler_shard_set_start_level: the start level is fixed by the first batch"
    for S in range(1, 7):
        with swz.Tiler(ctx, UNIT[0], UNIT[1], _params(O.RANDOM_GRID)) as t:
            assert t.info()["fast_start_levels"] == -1
            for bad in (0, 7, -1):
                with pytest.raises(swz.SwzError) as e:
                    t.shard_set_start_level(bad)
                assert e.value.code == swz.api.ERR_BAD_ARG and "FAST tilers, levels 1..6" in str(e.value)
            assert t.info()["fast_start_levels"] == -1   # a refused level fixes nothing
            t.shard_set_start_level(S)
            assert t.info()["fast_start_levels"] == S
            t.shard_set_start_level(S)                   # every batch of a sharded data set says it again
            for other in [v for v in range(1, 7) if v != S]:
                with pytest.raises(swz.SwzError) as e:
                    t.shard_set_start_level(other)
                assert e.value.code == swz.api.ERR_BAD_ARG and fixed in str(e.value)
            assert t.info()["fast_start_levels"] == S
    accurate = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=MAX_POINTS, spacing_at_root=0.05)
    with swz.Tiler(ctx, UNIT[0], UNIT[1], accurate) as t:
        with pytest.raises(swz.SwzError) as e:
            t.shard_set_start_level(4)
        assert e.value.code == swz.api.ERR_BAD_ARG and "FAST tilers" in str(e.value)


def _sharded_family(name):
    """test_shard_seams.family for the clouds of this file ("fast-start-<d>"), its own families otherwise."""
    if name.startswith("fast-start-"):
        d = int(name.rsplit("-", 1)[1])
        return layout_cloud(d, "z pair deep inside"), UNIT, [(O.spacing_from_diagonal(*UNIT, SPACING_DIV), MAX_POINTS)]
    return _seams_family(name)


_seams_family = seams.family


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", [O.MIN_DISTANCE, O.RANDOM_GRID])
@pytest.mark.parametrize("d,shards", [(4, 2), (5, 4)])
def test_sharded_fast_matches_oracle_at_start_levels_four_and_five(driver, cloud_files, tmp_path, monkeypatch, d, shards, sampler):
    """swz_group_tile on one device (the driver of test_shard_seams.py, unchanged: only its table of clouds gains an entry): the
    shards' summed histograms vote S = d, every shard rebuilds its levels d - 1 .. 1, shard 0 the root.  The cloud lies in one
    octant of the root, so one shard holds every point and the root is rebuilt on a shard that holds none."""
    monkeypatch.setattr(seams, "family", _sharded_family)
    name = "fast-start-%d" % d
    xyz, bounds, cases = seams.family(name)
    sp, mppn = cases[0]
    o = oracle_tile((layout_cloud, d, "z pair deep inside"), sampler)
    assert o["stats"]["fast_start_levels"] == d
    want_key, want_level, want_dup = seams._by_index(o)
    what = "%s, %s, FAST 2, %d shards" % (name, O.SAMPLER_NAMES[sampler], shards)
    run = seams._run(driver, cloud_files, tmp_path, name, sp, mppn, shards, what, sampler=sampler, strategy=O.FAST, concurrency=2)
    assert int((run["points"] > 0).sum()) == 1 and int(run["points"].max()) == xyz.shape[0]
    seams._compare(name, what, shards, run["rows"], want_key, want_level, want_dup)
    assert_fast_bookkeeping(run["rows"]["level"], run["rows"]["dup"], d)
