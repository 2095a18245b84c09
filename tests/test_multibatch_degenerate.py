"""The multi-batch tiler (swz_tiler.hip) on batches shaped the way real runs are fed and np.array_split of a random cloud never
is: empty batches, batches of a handful of points, the same batch again, thousands of records at one position, clouds that lie
outside the bounds, nodes exactly at max_points_per_node, batches in Morton order.  Every family goes through the four samplers x
{ACCURATE, FAST with 2 and with 8 indexing threads} x {add_batch_device, stage_batch / tile_staged} and must give the files of the
multi-batch oracle (oracle/oracle.cpp MBTiler) node for node, id for id, in file order; where the oracle REFUSES a batch (FAST: a
batch of fewer than fast_concurrency points, the empty one included -- parallel::scatter throws, util/threading/Parallel.h:181-186;
any batch after finalize) the library must refuse the same batch, stay as it was, and go on with the data set.

The CPU tests at the top prove each family's premise with the oracle alone (it really is the case its name says); the GPU tests
hold the library against the oracle.  The documented case in which the two may differ (re-keyed cached points out of order:
rekey_inversions / unsorted_cached_nodes > 0) is out of scope: every family asserts that it does not occur."""
import collections
import functools

import numpy as np
import pytest

import oracle_lib as O

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ODD = ([-512.25, 1000.5, -3.125], [-512.25 + 777.7, 1000.5 + 777.7, -3.125 + 777.7])
SAMPLERS = [O.RANDOM_GRID, O.GRID_CENTER, O.MIN_DISTANCE, O.JITTERED]
SAMPLER_NAMES = {O.RANDOM_GRID: "RANDOM_GRID", O.GRID_CENTER: "GRID_CENTER", O.MIN_DISTANCE: "MIN_DISTANCE", O.JITTERED: "JITTERED"}
# (strategy, fast_concurrency); the concurrency of an ACCURATE tiler is not looked at
MODES = {"ACCURATE": (O.ACCURATE, 2), "FAST2": (O.FAST, 2), "FAST8": (O.FAST, 8)}
PATHS = ["device", "staged"]
ORC_ERR_BAD_ARG = -5
FAST_START = 6   # estimate_start_node_level (TilingAlgorithms.cpp:1473-1535) with fewer than 100 000 points per octant

Leg = collections.namedtuple("Leg", "sampler strategy conc bounds")


def _world(bounds, u):
    lo, hi = np.array(bounds[0]), np.array(bounds[1])
    return np.ascontiguousarray(lo + np.asarray(u, dtype=np.float64).reshape(-1, 3) * (hi - lo))


def _cloud(seed, n):
    return np.random.default_rng(seed).random((n, 3))


def _min_batch(leg):
    """the smallest batch the leg's strategy accepts"""
    return leg.conc if leg.strategy == O.FAST else 1


# ------------------------------------------------------------------------------------------------ the oracle, batch by batch
def _oracle_run(bounds, batches, sampler, max_points, spacing, strategy, conc, max_depth=100, after_finalize=None):
    """Feeds every batch, whatever the answer: returns (status per batch, export, counts, status of a batch after finalize)."""
    t = O.Tiler(bounds[0], bounds[1], sampler, max_points, spacing, max_depth=max_depth, strategy=strategy, fast_concurrency=conc)
    sts = [t.add_batch(b) for b in batches]
    assert t.finalize() == 0
    late = t.add_batch(after_finalize) if after_finalize is not None else None
    ex, c = t.export(), t.counts()
    t.close()
    return sts, ex, c, late


def _first_rerooted_level(sampler, bounds, spacing):
    """The first node level whose grid needs more than the 21 key levels (tile_node re-roots there, TilingAlgorithms.cpp:444-483):
    the files below it are keyed by the re-rooted index, which is no prefix of the points' root keys any more."""
    if sampler == O.MIN_DISTANCE:
        return 20
    for lv in range(-1, 21):
        if O.lib().orc_required_morton_index_depth(sampler, lv, O._vec3(bounds[0]), O._vec3(bounds[1]), O.C.c_float(spacing)) >= 21:
            return lv
    return 20


def _files(ex):
    return {(int(l), int(k)): ex["ids"][int(o):int(o + c)] for l, k, o, c in zip(ex["level"], ex["key"], ex["offset"], ex["count"])}


# ------------------------------------------------------------------------------------------------ families
# make(leg) -> list of batches in world coordinates.  d / max_points: spacing = diagonal / d.  Most families use the pair
# of tests/test_multibatch.py's small cases (32, 300); "real node sizes" is BASELINE's pair (250, 20 000).
def _split_at(xyz, cuts):
    return [xyz[a:b] for a, b in zip([0] + list(cuts), list(cuts) + [len(xyz)])]


def _f_empty(where):
    def make(leg):
        a = _world(leg.bounds, _cloud(1, 9000))
        e = a[:0]
        return {"first": [e, a[:4000], a[4000:]], "middle": [a[:4000], e, a[4000:]], "last": [a[:4000], a[4000:], e],
                "two in a row": [a[:3000], e, e, a[3000:6000], e, a[6000:]], "only": [e, e, e]}[where]
    return make


def _f_one_point_per_batch(leg):
    a = _world(leg.bounds, _cloud(2, 320))      # crosses max_points = 300 at batch 301: the root turns from take-all to sampled
    return [a[i:i + 1] for i in range(len(a))]


SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]   # encode block, run-pass tile, sort tile of swz_sort.hip +- 1


def _f_sizes(leg):
    a = _world(leg.bounds, _cloud(3, sum(SIZES)))
    return _split_at(a, np.cumsum(SIZES)[:-1])


def _f_around_concurrency(leg):
    c = leg.conc
    a = _world(leg.bounds, _cloud(4, 8000 + 3 * c))
    return _split_at(a, [4000, 4000 + c - 1, 4000 + 2 * c - 1, 4000 + 3 * c])


def _f_same_batch(n):
    def make(leg):
        a = _world(leg.bounds, _cloud(5, n))
        return [a, a.copy(), a.copy()]
    return make


STACK = 600


def _f_stack(split, inside_cloud):
    def make(leg):
        p = _world(leg.bounds, np.tile([[0.3, 0.3, 0.3]], (STACK, 1)))
        parts = [p] if not split else [p[:200], p[200:400], p[400:]]
        if inside_cloud:
            bg = _world(leg.bounds, _cloud(6, 3000 * len(parts)))
            rng = np.random.default_rng(60)
            parts = [np.vstack([q, bg[3000 * i:3000 * (i + 1)]])[rng.permutation(len(q) + 3000)] for i, q in enumerate(parts)]
        return parts
    return make


def _f_outside(leg):
    a = _world(leg.bounds, 3.0 * _cloud(7, 12000) - 1.0)   # three times as wide as the bounds, around them
    return _split_at(a, [5000, 9000])


# a box inside ONE cell of the FAST start level (level-6 cells are 1/64 wide; 48/64 = 0.75) and away from its faces
BOX_LO, BOX_W = 0.752, 0.008


def _box_points(seed, n):
    return BOX_LO + BOX_W * _cloud(seed, n)


def _outside_box_cell(u):
    cell = np.floor(u * 64.0)
    return u[~np.all(cell == 48.0, axis=1)]


def _f_threshold(first, more):
    """ACCURATE: the ROOT receives `first` points in batch 1 and `more` in batch 2.  FAST: the same for a start node (node level
    5): the points of the box are all that its cell ever receives, the rest of the batches (which the strategy needs to be
    accepted) lies in other cells."""
    def make(leg):
        if leg.strategy == O.ACCURATE:
            a = _world(leg.bounds, _cloud(8, first + more))
            return [a[:first], a[first:]] if more else [a]
        bg = _outside_box_cell(_cloud(9, 4000))
        box = _box_points(10, first + more)
        b1 = np.vstack([bg[:2000], box[:first]])
        b2 = np.vstack([bg[2000:2000 + leg.conc - more], box[first:]])
        return [_world(leg.bounds, b1), _world(leg.bounds, b2)]
    return make


def _f_into_deepest_leaf(leg):
    """The last batch is the smallest one the strategy accepts, every point of it a copy of a point that the deepest node of the
    tree built so far holds (found with the oracle: it depends on the sampler)."""
    a = _world(leg.bounds, np.vstack([_cloud(11, 6000), 0.6 + 0.01 * _cloud(12, 2000)]))
    first = _split_at(a, [4000])
    sp = O.spacing_from_diagonal(*leg.bounds, 32)
    _, ex, _, _ = _oracle_run(leg.bounds, first, leg.sampler, 300, sp, leg.strategy, leg.conc)
    deepest = len(ex["level"]) - 1 - int(np.argmax(ex["level"][::-1] == ex["level"].max()))
    pid = int(ex["ids"][int(ex["offset"][deepest])])
    return first + [np.tile(ex["xyz"][pid], (_min_batch(leg), 1))]


def _f_one_octant_later(leg):
    a = _world(leg.bounds, _cloud(13, 8000))
    b = _world(leg.bounds, 0.125 + 0.125 * _cloud(14, 3000))    # one level-2 octant: [1/8, 1/4)^3
    return _split_at(a, [4000]) + [b]


def _morton_sorted(leg, seed, n):
    a = _world(leg.bounds, _cloud(seed, n))
    keys, _ = O.index_points(a, *leg.bounds)
    return a[np.argsort(keys, kind="stable")]


def _f_morton(reverse):
    def make(leg):
        a = _morton_sorted(leg, 15, 9000)
        return np.array_split(a[::-1].copy() if reverse else a, 6)
    return make


INTERLEAVED_CELLS, INTERLEAVED_BATCHES = 200, 40


def _f_interleaved(leg):
    """200 cells of the FAST start level (level 6), 40 points in each; batch j is the j-th point of every cell."""
    rng = np.random.default_rng(16)
    cells = rng.choice(64 ** 3, INTERLEAVED_CELLS, replace=False)
    origin = np.column_stack([cells % 64, (cells // 64) % 64, cells // 4096]) / 64.0
    return [_world(leg.bounds, origin + (0.1 + 0.8 * rng.random((INTERLEAVED_CELLS, 3))) / 64.0) for _ in range(INTERLEAVED_BATCHES)]


Family = collections.namedtuple("Family", "make d max_points")
FAMILIES = {
    "1 empty first": Family(_f_empty("first"), 32, 300),
    "1 empty middle": Family(_f_empty("middle"), 32, 300),
    "1 empty last": Family(_f_empty("last"), 32, 300),
    "1 empty two in a row": Family(_f_empty("two in a row"), 32, 300),
    "1 empty only": Family(_f_empty("only"), 32, 300),
    "2 one point per batch": Family(_f_one_point_per_batch, 32, 300),
    "2 sizes at tile edges": Family(_f_sizes, 32, 300),
    "2 sizes around fast_concurrency": Family(_f_around_concurrency, 32, 300),
    "3 same batch three times": Family(_f_same_batch(6000), 32, 300),
    "3 same batch three times, real node sizes": Family(_f_same_batch(8000), 250, 20000),
    "4 stack in one batch": Family(_f_stack(False, False), 32, 50),
    "4 stack over three batches": Family(_f_stack(True, False), 32, 50),
    "4 stack in one batch inside a cloud": Family(_f_stack(False, True), 32, 50),
    "4 stack over three batches inside a cloud": Family(_f_stack(True, True), 32, 50),
    "5 outside the bounds": Family(_f_outside, 32, 300),
    "6 max_points then one more": Family(_f_threshold(300, 1), 32, 300),
    "6 one less than max_points then one more": Family(_f_threshold(299, 1), 32, 300),
    "6 exactly max_points at first sight": Family(_f_threshold(300, 0), 32, 300),
    "6 max_points plus one at first sight": Family(_f_threshold(301, 0), 32, 300),
    "6 last batch into the deepest leaf": Family(_f_into_deepest_leaf, 32, 300),
    "6 one level-2 octant after the whole cube": Family(_f_one_octant_later, 32, 300),
    "7 morton order": Family(_f_morton(False), 32, 300),
    "7 reverse morton order": Family(_f_morton(True), 32, 300),
    "7 interleaved over the start nodes": Family(_f_interleaved, 32, 300),
}
FAMILY_NAMES = list(FAMILIES)


def _leg(family, sampler, mode):
    strategy, conc = MODES[mode]
    # both bounds for every family, sampler and mode: the key path (cubic) and the position path of MIN_DISTANCE are both reached
    odd = (FAMILY_NAMES.index(family) + SAMPLERS.index(sampler) + list(MODES).index(mode)) % 2
    return Leg(sampler, strategy, conc, ODD if odd else UNIT)


@functools.lru_cache(maxsize=None)
def _case(family, sampler, mode):
    """(leg, batches, spacing, oracle's status per batch, export, counts, status after finalize) -- shared by the CPU premise
    tests and by both GPU paths of the leg."""
    fam = FAMILIES[family]
    leg = _leg(family, sampler, mode)
    batches = [np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 3) for b in fam.make(leg)]
    sp = O.spacing_from_diagonal(*leg.bounds, fam.d)
    late = _world(leg.bounds, _cloud(99, 64))
    sts, ex, c, late_st = _oracle_run(leg.bounds, batches, sampler, fam.max_points, sp, leg.strategy, leg.conc, after_finalize=late)
    return leg, batches, sp, sts, ex, c, late_st, late


def _expected_refusals(leg, batches):
    """What the issue of the refusal rule says, independent of the oracle's code: FAST refuses n < fast_concurrency."""
    return [ORC_ERR_BAD_ARG if (leg.strategy == O.FAST and len(b) < leg.conc) else 0 for b in batches]


ALL_LEGS = [(f, s, m) for f in FAMILY_NAMES for s in SAMPLERS for m in MODES]


def _leg_id(v):
    return SAMPLER_NAMES.get(v, v) if isinstance(v, int) else v


# ------------------------------------------------------------------------------------------------ CPU: the premises
@pytest.mark.parametrize("family,sampler,mode", ALL_LEGS, ids=_leg_id)
def test_oracle_premises_every_family(family, sampler, mode):
    """The oracle refuses exactly the batches the rule names and every batch after finalize; no cached node was out of order;
    every accepted point is stored (ACCURATE: exactly once; FAST: once below the start level, plus copies above), inside its node
    (checked down to the first re-rooted level)."""
    leg, batches, sp, sts, ex, c, late_st, _ = _case(family, sampler, mode)
    assert sts == _expected_refusals(leg, batches)
    assert late_st == ORC_ERR_BAD_ARG
    assert c["unsorted_cached_nodes"] == 0
    accepted = [b for b, st in zip(batches, sts) if st == 0]
    n = sum(len(b) for b in accepted)
    assert c["num_points"] == n and len(ex["xyz"]) == n
    if n == 0:
        assert c["num_nodes"] == 0 and c["num_stored"] == 0 and len(ex["ids"]) == 0
        return
    xyz = np.vstack(accepted)
    lo, hi = np.array(leg.bounds[0]), np.array(leg.bounds[1])
    assert np.array_equal(ex["xyz"], np.clip(xyz, lo, hi))      # ids count the ACCEPTED points in input order
    keys, _ = O.index_points(xyz, *leg.bounds)
    per_entry_level = np.repeat(ex["level"].astype(np.int64), ex["count"].astype(np.int64))
    if leg.strategy == O.ACCURATE:
        assert c["num_stored"] == n and np.array_equal(np.sort(ex["ids"]), np.arange(n, dtype=np.uint32))
    else:
        own = ex["ids"][per_entry_level >= FAST_START - 1]      # reconstructed ancestors hold copies
        assert np.array_equal(np.sort(own), np.arange(n, dtype=np.uint32))
        assert int(ex["ids"].max()) < n
    per_entry_key = np.repeat(ex["key"], ex["count"].astype(np.int64))
    check = (per_entry_level >= 0) & (per_entry_level <= _first_rerooted_level(sampler, leg.bounds, sp))
    sh = ((20 - per_entry_level[check]) * 3).astype(np.uint64)
    assert np.array_equal(keys[ex["ids"][check]] >> sh, per_entry_key[check] >> sh)


@pytest.mark.parametrize("sampler", SAMPLERS, ids=_leg_id)
@pytest.mark.parametrize("where", ["first", "middle", "last", "two in a row"])
def test_oracle_premise_empty_batches_change_no_file(sampler, where):
    """ACCURATE: the files with empty batches are the files without them."""
    leg, batches, sp, sts, ex, c, _, _ = _case("1 empty " + where, sampler, "ACCURATE")
    assert sts == [0] * len(batches) and any(len(b) == 0 for b in batches)
    _, ex2, c2, _ = _oracle_run(leg.bounds, [b for b in batches if len(b)], sampler, 300, sp, O.ACCURATE, 2)
    assert c2 == c
    for col in ("level", "key", "offset", "count", "ids"):
        assert np.array_equal(ex[col], ex2[col]), col


def test_oracle_premise_batch_sizes():
    leg = _leg("2 sizes at tile edges", O.RANDOM_GRID, "ACCURATE")
    assert [len(b) for b in _f_sizes(leg)] == SIZES
    assert len(_f_one_point_per_batch(leg)) > 300 and all(len(b) == 1 for b in _f_one_point_per_batch(leg))
    for mode, (strategy, conc) in MODES.items():
        leg = _leg("2 sizes around fast_concurrency", O.RANDOM_GRID, mode)
        assert [len(b) for b in _f_around_concurrency(leg)] == [4000, conc - 1, conc, conc + 1, 4000]


@pytest.mark.parametrize("family", [f for f in FAMILY_NAMES if f.startswith("3 ")])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=_leg_id)
def test_oracle_premise_same_batch_ties_with_the_cache_everywhere(family, sampler):
    """Every key of the second and third batch equals a cached key (share 100 %).  With real node sizes the root takes all of
    batch 1; the same points again find a file there, so the root samples (:272-275) and, new before cached on equal keys
    (merge_sorted), RANDOM_GRID's first point of every cell is a point of the batch, never its cached twin."""
    leg, batches, sp, sts, ex, c, _, _ = _case(family, sampler, "ACCURATE")
    keys = [O.index_points(b, *leg.bounds)[0] for b in batches]
    for k in (1, 2):
        assert np.isin(keys[k], np.concatenate(keys[:k])).mean() == 1.0
    fam = FAMILIES[family]
    n = len(batches[0])
    _, ex1, c1, _ = _oracle_run(leg.bounds, batches[:1], sampler, fam.max_points, sp, O.ACCURATE, 2)
    _, ex2, c2, _ = _oracle_run(leg.bounds, batches[:2], sampler, fam.max_points, sp, O.ACCURATE, 2)
    assert (c1["num_nodes"] == 1) == (n <= fam.max_points)
    assert c2["num_nodes"] > 1 and c["num_nodes"] >= c2["num_nodes"]
    if sampler == O.RANDOM_GRID:
        root2, root3 = _files(ex2)[(-1, 0)], _files(ex)[(-1, 0)]
        assert np.all(root2 >= n) and np.all(root3 >= 2 * n)


@pytest.mark.parametrize("family", [f for f in FAMILY_NAMES if f.startswith("4 ")])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=_leg_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_oracle_premise_stack_ends_in_a_terminal_node(family, sampler, mode):
    """A chain of nodes down to level 20, whose file is what came down in the last batch followed by what it held before
    (merge_node_data_unsorted: new ++ cached)."""
    leg, batches, sp, sts, ex, c, _, _ = _case(family, sampler, mode)
    assert int(ex["level"].max()) == 20
    terminal = [ids for (lv, key), ids in _files(ex).items() if lv == 20]
    assert len(terminal) == 1 and len(terminal[0]) > 50
    if len(batches) > 1:
        _, ex1, _, _ = _oracle_run(leg.bounds, batches[:-1], sampler, 50, sp, leg.strategy, leg.conc)
        before = [ids for (lv, key), ids in _files(ex1).items() if lv == 20]
        assert len(before) == 1 and 0 < len(before[0]) < len(terminal[0])
        assert np.array_equal(terminal[0][-len(before[0]):], before[0])
        first_new = sum(len(b) for b in batches[:-1])
        assert np.any(terminal[0][:-len(before[0])] >= first_new)
    if "cloud" not in family and mode == "ACCURATE":
        assert c["num_nodes"] == 22       # root .. level 19 hold one point each, level 20 the rest


@pytest.mark.parametrize("sampler", SAMPLERS, ids=_leg_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_oracle_premise_outside_points_clamp_onto_the_faces(sampler, mode):
    leg, batches, sp, sts, ex, c, _, _ = _case("5 outside the bounds", sampler, mode)
    xyz = np.vstack(batches)
    lo, hi = np.array(leg.bounds[0]), np.array(leg.bounds[1])
    outside = np.any((xyz < lo) | (xyz > hi), axis=1)
    assert outside.mean() > 0.6
    keys, clamped = O.index_points(xyz, *leg.bounds)
    assert np.array_equal(clamped, np.clip(xyz, lo, hi)) and np.array_equal(ex["xyz"], clamped)
    corner = np.all((clamped == lo) | (clamped == hi), axis=1)
    assert corner.sum() > 8 * 20 and {0, (1 << 63) - 1} <= set(keys[corner].tolist())   # key coordinates 0 and 2^21 - 1
    assert int(ex["level"].max()) == 20


@pytest.mark.parametrize("sampler", SAMPLERS, ids=_leg_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_oracle_premise_thresholds(sampler, mode):
    """The node in question (ACCURATE: the root; FAST: the start node of the box).  At first sight it takes all of exactly
    max_points points and samples max_points + 1 (TakeAllWhenCountBelowMaxPoints).  Once it has a file it ALWAYS samples
    (TilingAlgorithms.cpp:272-275: the switch is on the cached count, not on the total): one more point on a take-all file of
    max_points, and just the same on one of max_points - 1, although the total is then not above max_points."""
    strategy, conc = MODES[mode]
    for family, first, more in (("6 max_points then one more", 300, 1), ("6 one less than max_points then one more", 299, 1),
                                ("6 exactly max_points at first sight", 300, 0), ("6 max_points plus one at first sight", 301, 0)):
        leg, batches, sp, sts, ex, c, _, _ = _case(family, sampler, mode)
        assert sts == [0] * len(batches)
        if strategy == O.ACCURATE:
            at, prefix = (-1, 0), lambda key, lv: 0
        else:
            box_key = int(O.index_points(_world(leg.bounds, [[BOX_LO + BOX_W / 2] * 3]), *leg.bounds)[0][0])
            sh = (20 - (FAST_START - 1)) * 3
            at, prefix = (FAST_START - 1, (box_key >> sh) << sh), lambda key, lv: key >> sh
        below = lambda files: [k for k in files if k[0] > at[0] and prefix(k[1], k[0]) == prefix(at[1], at[0])]
        _, ex1, _, _ = _oracle_run(leg.bounds, batches[:1], sampler, 300, sp, leg.strategy, leg.conc)
        files1, files2 = _files(ex1), _files(ex)
        subtree = lambda files: len(files[at]) + sum(len(files[k]) for k in below(files))
        assert subtree(files1) == first and subtree(files2) == first + more
        if first <= 300:
            assert len(files1[at]) == first and not below(files1)      # took all at first sight
            if more:
                assert len(files2[at]) < first + more and below(files2)    # has a file: sampled, whatever the total
            else:
                assert len(files2[at]) == first and not below(files2)      # (the data set ends with the take-all file)
        else:
            assert len(files1[at]) < first and below(files1)


@pytest.mark.parametrize("sampler", SAMPLERS, ids=_leg_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_oracle_premise_last_batch_lands_in_the_deepest_leaf(sampler, mode):
    leg, batches, sp, sts, ex, c, _, _ = _case("6 last batch into the deepest leaf", sampler, mode)
    assert len(batches[-1]) == _min_batch(leg) and sts == [0, 0, 0]
    _, ex1, _, _ = _oracle_run(leg.bounds, batches[:-1], sampler, 300, sp, leg.strategy, leg.conc)
    deepest = int(ex1["level"].max())
    assert deepest >= 2
    first_new = sum(len(b) for b in batches[:-1])
    per_entry_level = np.repeat(ex["level"].astype(np.int64), ex["count"].astype(np.int64))
    new_levels = per_entry_level[ex["ids"] >= first_new]
    assert new_levels.max() >= deepest      # the batch reached the deepest level (or made a deeper one)


@pytest.mark.parametrize("mode", list(MODES))
def test_oracle_premise_ordered_batches(mode):
    leg = _leg("7 morton order", O.RANDOM_GRID, mode)
    fwd = np.vstack(_f_morton(False)(leg))
    rev = np.vstack(_f_morton(True)(leg))
    assert np.all(np.diff(O.index_points(fwd, *leg.bounds)[0].astype(np.int64)) >= 0)
    assert np.all(np.diff(O.index_points(rev, *leg.bounds)[0].astype(np.int64)) <= 0)
    leg = _leg("7 interleaved over the start nodes", O.RANDOM_GRID, mode)
    batches = _f_interleaved(leg)
    assert len(batches) == INTERLEAVED_BATCHES
    sh = np.uint64((20 - (FAST_START - 1)) * 3)
    cells = [np.sort(O.index_points(b, *leg.bounds)[0] >> sh) for b in batches]
    assert len(np.unique(cells[0])) == INTERLEAVED_CELLS       # one point per start node ...
    assert all(np.array_equal(cc, cells[0]) for cc in cells)    # ... and every batch touches every start node
    one = _leg("6 one level-2 octant after the whole cube", O.RANDOM_GRID, mode)
    last = _f_one_octant_later(one)[-1]
    assert len(np.unique(O.index_points(last, *one.bounds)[0] >> np.uint64(54))) == 1    # three octants: levels 0, 1, 2
    if mode != "ACCURATE":
        _, _, _, sts, ex, c, _, _ = _case("7 interleaved over the start nodes", O.RANDOM_GRID, mode)
        assert int((ex["level"] == FAST_START - 1).sum()) == INTERLEAVED_CELLS


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def _params(swz, sampler, max_points, spacing, strategy, conc, max_depth=100):
    return swz.TileParams(sampler=sampler, max_points_per_node=max_points, spacing_at_root=spacing, max_depth=max_depth,
                          strategy=strategy, fast_concurrency=conc)


WATCHED = ("num_points", "num_stored", "num_nodes", "num_batches", "fast_start_levels", "staged_bytes")


def _watched(t):
    info = t.info()
    return {k: info[k] for k in WATCHED}


def _read_files(t, ctx):
    import torch
    info = t.info()
    table = t.node_table()
    ns = int(info["num_stored"])
    d_keys = torch.empty(max(ns, 1), dtype=torch.int64, device="cuda")
    d_ids = torch.empty(max(ns, 1), dtype=torch.int32, device="cuda")
    d_lvl = torch.empty(max(ns, 1), dtype=torch.int8, device="cuda")
    t.export_device(d_keys.data_ptr(), d_ids.data_ptr(), d_lvl.data_ptr())
    torch.cuda.synchronize()
    n = int(info["num_points"])
    p_xyz, _ = t.pools_device()
    pool = ctx.copy_to_host(p_xyz, n * 24).view(np.float64).reshape(n, 3) if n else np.empty((0, 3))
    return dict(table=table, ids=d_ids.cpu().numpy().view(np.uint32)[:ns], level=d_lvl.cpu().numpy()[:ns], info=info, pool=pool)


def _refused(swz, call):
    """True when the call was refused with BAD_ARG, False when it went through; anything else is an error of the test."""
    try:
        call()
    except swz.SwzError as e:
        assert e.code == swz.api.ERR_BAD_ARG, (e.code, str(e))
        return True
    return False


def _gpu_run(ctx, bounds, batches, sampler, max_points, spacing, strategy, conc, path, expect, late=None):
    """Feeds every batch like _oracle_run; a batch must be refused exactly where expect (the oracle's status) is not 0, and a
    refusal must leave what info() reports as it was.  Returns the files, the pool, info and (device path) the caller's buffers
    after the call."""
    import schwarzwald_amd as swz
    import torch
    seen = []
    with swz.Tiler(ctx, bounds[0], bounds[1], _params(swz, sampler, max_points, spacing, strategy, conc)) as t:
        if path == "device":
            for b, st in zip(batches, expect):
                d = torch.from_numpy(b).cuda()          # (an empty batch: data_ptr() of an empty tensor is NULL)
                torch.cuda.synchronize()
                before = _watched(t)
                refused = _refused(swz, lambda: t.add_batch_device(d.data_ptr(), b.shape[0]))
                assert refused == (st != 0), "batch of %d points: library %s, oracle status %d" % (
                    len(b), "refused" if refused else "accepted", st)
                if refused:
                    assert _watched(t) == before
                else:
                    seen.append(d.cpu().numpy())
        else:
            pinned = []
            for b in batches:
                a = swz.pinned_empty(b.shape, np.float64)
                a[...] = b
                pinned.append(a)
            waiting = 0     # staged and not tiled: one batch ahead, like the loop in include/swz_gpu.h
            for a, st in zip(pinned, expect):
                before = _watched(t)
                refused = _refused(swz, lambda: t.stage_batch(a))
                assert refused == (st != 0), "batch of %d points: library %s, oracle status %d" % (
                    len(a), "refused" if refused else "accepted", st)
                if refused:
                    assert _watched(t) == before
                    continue
                waiting += 1
                if waiting == 2:
                    t.tile_staged()
                    waiting -= 1
            while waiting:
                t.tile_staged()
                waiting -= 1
        t.finalize()
        if late is not None:    # a batch after finalize is refused up front as well: nothing changes, nothing is poisoned
            before = _watched(t)
            d = torch.from_numpy(late).cuda()
            assert _refused(swz, (lambda: t.add_batch_device(d.data_ptr(), len(late))) if path == "device" else (lambda: t.add_batch(late)))
            assert _watched(t) == before
        g = _read_files(t, ctx)
    g["seen"] = seen
    return g


def _compare(g, ex, c):
    """tests/test_multibatch.py's _compare: node table, ids in file order, the per-entry level."""
    tb = g["table"]
    assert len(tb["level"]) == len(ex["level"]) == c["num_nodes"]
    assert np.array_equal(tb["level"], ex["level"])
    assert np.array_equal(tb["key"], ex["key"])
    assert np.array_equal(tb["offset"], ex["offset"])
    assert np.array_equal(tb["count"], ex["count"])
    assert np.array_equal(g["ids"], ex["ids"])
    assert np.array_equal(g["level"], np.repeat(ex["level"], ex["count"].astype(np.int64)))


def _compare_all(g, ex, c, sts):
    assert g["info"]["rekey_inversions"] == 0 and c["unsorted_cached_nodes"] == 0
    _compare(g, ex, c)
    info = g["info"]
    assert info["num_points"] == c["num_points"] and info["num_stored"] == c["num_stored"] and info["num_nodes"] == c["num_nodes"]
    assert info["num_batches"] == sum(1 for st in sts if st == 0)       # empty ACCURATE batches count, refused ones do not
    # the positions the tiler keeps: clamped like index_point clamps them, bit for bit, by point id
    assert g["pool"].tobytes() == ex["xyz"].tobytes()
    if g["seen"]:   # add_batch_device clamps the caller's buffer in place
        assert np.vstack(g["seen"]).tobytes() == ex["xyz"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("family,sampler,mode", ALL_LEGS, ids=_leg_id)
def test_gpu_degenerate_batches_match_oracle(ctx, family, sampler, mode, path):
    leg, batches, sp, sts, ex, c, late_st, late = _case(family, sampler, mode)
    assert late_st == ORC_ERR_BAD_ARG
    fam = FAMILIES[family]
    g = _gpu_run(ctx, leg.bounds, batches, sampler, fam.max_points, sp, leg.strategy, leg.conc, path, sts, late=late)
    _compare_all(g, ex, c, sts)


@pytest.mark.gpu
@pytest.mark.parametrize("conc", [2, 8])
@pytest.mark.parametrize("entry", ["add_batch_device", "add_batch_device NULL", "stage_batch", "add_batch"])
def test_gpu_fast_refuses_an_empty_batch_like_the_oracle(ctx, conc, entry):
    """[8000 points, 0 points, 12000 points] under FAST: the oracle answers [0, BAD_ARG, 0] (parallel::scatter throws for fewer
    points than indexing threads, util/threading/Parallel.h:181-186, and 0 is fewer).  The library must refuse the empty batch
    through every entry point, count neither a batch nor a point for it, stay usable, and end with the oracle's files."""
    import schwarzwald_amd as swz
    import torch
    a = _cloud(21, 20000)
    batches = [a[:8000], a[:0], a[8000:]]
    sp = O.spacing_from_diagonal(*UNIT, 32)
    sts, ex, c, _ = _oracle_run(UNIT, batches, O.RANDOM_GRID, 300, sp, O.FAST, conc)
    assert sts == [0, ORC_ERR_BAD_ARG, 0]
    with swz.Tiler(ctx, UNIT[0], UNIT[1], _params(swz, O.RANDOM_GRID, 300, sp, O.FAST, conc)) as t:
        t.add_batch(batches[0])
        before = _watched(t)
        assert before["num_batches"] == 1 and before["num_points"] == 8000
        valid = torch.zeros(3, dtype=torch.float64, device="cuda")
        empty = np.empty((0, 3))
        call = {"add_batch_device": lambda: t.add_batch_device(valid.data_ptr(), 0),
                "add_batch_device NULL": lambda: t.add_batch_device(None, 0),
                "stage_batch": lambda: t.stage_batch(empty), "add_batch": lambda: t.add_batch(empty)}[entry]
        with pytest.raises(swz.SwzError) as e:
            call()
        assert e.value.code == swz.api.ERR_BAD_ARG and "fast_concurrency" in str(e.value)
        assert _watched(t) == before
        if entry == "stage_batch":
            with pytest.raises(swz.SwzError) as e2:     # nothing was staged
                t.tile_staged()
            assert e2.value.code == swz.api.ERR_BAD_ARG and "nothing is staged" in str(e2.value)
        t.add_batch(batches[2])     # not poisoned
        t.finalize()
        g = _read_files(t, ctx)
    g["seen"] = []
    _compare_all(g, ex, c, sts)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["add_batch_device", "stage_batch", "add_batch"])
def test_gpu_refused_small_batch_between_staged_batches(ctx, entry):
    """FAST with 8 indexing threads, a batch of 7 points refused while another batch is staged and not yet tiled: the staged
    batch is tiled as if nothing had happened, the ids go on where they were."""
    import schwarzwald_amd as swz
    import torch
    a = _world(ODD, _cloud(22, 9007))
    batches = [a[:5000], a[5000:5007], a[5007:]]
    sp = O.spacing_from_diagonal(*ODD, 32)
    sts, ex, c, _ = _oracle_run(ODD, batches, O.MIN_DISTANCE, 300, sp, O.FAST, 8)
    assert sts == [0, ORC_ERR_BAD_ARG, 0]
    with swz.Tiler(ctx, ODD[0], ODD[1], _params(swz, O.MIN_DISTANCE, 300, sp, O.FAST, 8)) as t:
        if entry == "stage_batch":
            t.stage_batch(batches[0])
            before = _watched(t)
            assert _refused(swz, lambda: t.stage_batch(batches[1]))
            assert _watched(t) == before
            t.stage_batch(batches[2])
            t.tile_staged()
            t.tile_staged()
        else:
            t.add_batch(batches[0])
            before = _watched(t)
            d = torch.from_numpy(batches[1].copy()).cuda()
            assert _refused(swz, (lambda: t.add_batch_device(d.data_ptr(), 7)) if entry == "add_batch_device" else (lambda: t.add_batch(batches[1])))
            assert _watched(t) == before
            t.add_batch(batches[2])
        t.finalize()
        g = _read_files(t, ctx)
    g["seen"] = []
    _compare_all(g, ex, c, sts)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_gpu_tiler_that_never_saw_a_point(ctx, mode):
    """finalize, info, node table, export and pools of a tiler without points; ACCURATE counts its empty batches."""
    import schwarzwald_amd as swz
    strategy, conc = MODES[mode]
    with swz.Tiler(ctx, UNIT[0], UNIT[1], _params(swz, O.GRID_CENTER, 300, 0.05, strategy, conc)) as t:
        if strategy == O.ACCURATE:
            t.add_batch_device(None, 0)
            t.add_batch(np.empty((0, 3)))
            t.stage_batch(np.empty((0, 3)))
            t.tile_staged()
        t.finalize()
        t.finalize()    # (a second finalize is a no-op in both)
        g = _read_files(t, ctx)
        assert g["info"]["num_batches"] == (3 if strategy == O.ACCURATE else 0)
        assert g["info"]["num_points"] == g["info"]["num_stored"] == g["info"]["num_nodes"] == 0
        assert len(g["table"]["level"]) == 0 and len(g["ids"]) == 0
        assert g["info"]["fast_start_levels"] == -1


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", SAMPLERS, ids=_leg_id)
@pytest.mark.parametrize("n", [0, 1])
def test_gpu_single_batch_tile_of_no_point_and_of_one_point(ctx, sampler, n):
    import schwarzwald_amd as swz
    xyz = _world(ODD, _cloud(23, n))
    sp = O.spacing_from_diagonal(*ODD, 32)
    for strategy, conc in ((O.ACCURATE, 2), (O.FAST, 1)):
        ref = O.tile(xyz, *ODD, sampler, 300, sp, strategy=strategy, fast_concurrency=conc)
        assert ref["status"] == 0
        got = ctx.tile(xyz, *ODD, _params(swz, sampler, 300, sp, strategy, conc))
        assert np.array_equal(got.keys, ref["keys"]) and np.array_equal(got.perm, ref["perm"])
        assert np.array_equal(got.level, ref["level"]) and np.array_equal(got.dup, ref["dup"])
        assert got.stats["num_nodes"] == ref["stats"]["num_nodes"] and got.stats["max_level"] == ref["stats"]["max_level"]


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["4 stack in one batch", "4 stack in one batch inside a cloud", "5 outside the bounds"])
@pytest.mark.parametrize("sampler", SAMPLERS, ids=_leg_id)
@pytest.mark.parametrize("mode", ["ACCURATE", "FAST2"])
def test_gpu_single_batch_as_node_files_on_stacks_and_outside_points(ctx, family, sampler, mode):
    """swz_tile_nodes_begin_device / _end_device against the k = 1 oracle: the chain down to level 20 and its terminal node."""
    import schwarzwald_amd as swz
    import torch
    leg = _leg(family, sampler, mode)
    fam = FAMILIES[family]
    xyz = np.vstack(fam.make(leg))
    sp = O.spacing_from_diagonal(*leg.bounds, fam.d)
    sts, ex, c, _ = _oracle_run(leg.bounds, [xyz], sampler, fam.max_points, sp, leg.strategy, leg.conc)
    assert sts == [0] and int(ex["level"].max()) == 20 and c["unsorted_cached_nodes"] == 0
    d = torch.from_numpy(xyz.copy()).cuda()
    bufs = {}

    def alloc(ns):
        bufs["k"] = torch.empty(max(ns, 1), dtype=torch.int64, device="cuda")
        bufs["i"] = torch.empty(max(ns, 1), dtype=torch.int32, device="cuda")
        bufs["l"] = torch.empty(max(ns, 1), dtype=torch.int8, device="cuda")
        return bufs["k"].data_ptr(), bufs["i"].data_ptr(), bufs["l"].data_ptr()
    stats, table, ns = ctx.tile_nodes_device(d.data_ptr(), len(xyz), *leg.bounds, _params(swz, sampler, fam.max_points, sp, leg.strategy, leg.conc), alloc)
    torch.cuda.synchronize()
    g = dict(table=table, ids=bufs["i"].cpu().numpy().view(np.uint32)[:ns], level=bufs["l"].cpu().numpy()[:ns])
    _compare(g, ex, c)
    assert ns == c["num_stored"] and stats["max_level"] == 20
    assert d.cpu().numpy().tobytes() == ex["xyz"].tobytes()     # clamped in place
