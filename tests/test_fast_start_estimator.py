"""swz_fast_start_level_from_counts (estimate_start_level_host in swz_session.hip) on engineered 8^6 prefix histograms.

The estimate walks the depths 1 .. 6.  At a depth it counts the ranges (cells of that depth that hold points) and the large
ones (100 000 points or more); the score is 0 when ranges <= concurrency / 2 (integer division), float(large) /
float(concurrency) otherwise, and the first depth whose score reaches 1 gives the start level max(depth, 3); no such depth: 6.
start_level below restates that from swz_session.hip's comments on plain integers; where a histogram comes from a real cloud
the oracle's own estimate (on the sorted keys, not on counts) must agree too.

About the condition on the ranges: a score of 1 needs large >= concurrency, and large <= ranges, so whenever the score could
reach 1 there are at least `concurrency` ranges -- more than concurrency / 2.  The condition never decides the result, which
test_ranges_condition_never_decides pins; no test of the result can tell `<=` from `<` there."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from test_fast_start_levels_gpu import AXES, DEEP_PATH, LARGE, UNIT, prefix_of, sibling_cloud, sibling_path

NBINS = 1 << 18
CONCURRENCIES = [1, 2, 3, 4, 5, 8, 64, 2 ** 32 - 1]


def start_level(counts, concurrency):
    """The estimate, re-derived: exact integers (64-bit sums of totals below 2^32), the score in float32 as the library
    computes it."""
    counts = np.asarray(counts, dtype=np.uint64)
    assert counts.shape == (NBINS,) and concurrency >= 1 and int(counts.sum()) < 2 ** 32
    for depth in range(1, 7):
        cells = counts.reshape(8 ** depth, 8 ** (6 - depth)).sum(axis=1, dtype=np.uint64)
        ranges = int(np.count_nonzero(cells > 0))
        large = int(np.count_nonzero(cells >= 100000))
        score = np.float32(0.0)
        if not ranges <= concurrency // 2:
            score = np.float32(large) / np.float32(concurrency)
        if score >= np.float32(1.0):
            return max(depth, 3)
    return 6


def library_level(counts, concurrency):
    import schwarzwald_amd as swz
    return swz.api.fast_start_level_from_counts(np.asarray(counts, dtype=np.uint64), concurrency)


def cells_to_counts(cells, seed=0, spread=True):
    """2^18 counts from [(octant digits of a cell, points)]: a cell's points dealt at random over its depth-6 bins (spread), or
    all in its first bin."""
    rng = np.random.default_rng(seed)
    counts = np.zeros(NBINS, dtype=np.uint64)
    for digits, n in cells:
        width = 8 ** (6 - len(digits))
        first = prefix_of(digits) * width
        if spread and width > 1:
            counts[first:first + width] += rng.multinomial(n, np.full(width, 1.0 / width)).astype(np.uint64)
        else:
            counts[first] += np.uint64(n)
    return counts


def sibling_counts(d, na, nb, path=None, axis="x", seed=0, spread=True):
    path = [0] * d if path is None else list(path)
    return cells_to_counts([(path, na), (sibling_path(path, axis, d), nb)], seed, spread)


def check(counts, concurrency, expected=None):
    got = library_level(counts, concurrency)
    assert got == start_level(counts, concurrency), (concurrency, got)
    if expected is not None:
        assert got == expected, (concurrency, got, expected)
    return got


# ------------------------------------------------------------------------------------------ the threshold of a large range
@pytest.mark.parametrize("spread", [True, False], ids=["spread over the bins", "one bin per cell"])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6])
def test_large_range_threshold_from_both_sides(d, spread):
    """Two sibling cells of depth d, two threads: 100 000 + 100 000 points vote max(d, 3) -- d = 1 and d = 2 answer the floor,
    3 --, 100 000 + 99 999 vote 6, and so does one point fewer in either cell or in both."""
    for path, axis in (([0] * d, "x"), (DEEP_PATH[:d], "z"), ([7] * d, "y")):
        assert check(sibling_counts(d, LARGE, LARGE, path, axis, d, spread), 2) == max(d, 3)
        check(sibling_counts(d, LARGE, LARGE - 1, path, axis, d, spread), 2, 6)
        check(sibling_counts(d, LARGE - 1, LARGE, path, axis, d, spread), 2, 6)
        check(sibling_counts(d, LARGE - 1, LARGE - 1, path, axis, d, spread), 2, 6)
        check(sibling_counts(d, LARGE + 1, LARGE, path, axis, d, spread), 2, max(d, 3))


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6])
def test_sibling_layout_at_every_concurrency(d):
    """One thread is served by a single large range (ranges <= 0 is false): depth 1 already scores, S = 3.  Two threads need
    the two cells: S = max(d, 3).  Three threads and more never see `concurrency` large ranges: 6."""
    full = sibling_counts(d, LARGE, LARGE, DEEP_PATH[:d], "x", d)
    short = sibling_counts(d, LARGE, LARGE - 1, DEEP_PATH[:d], "x", d)
    for concurrency in CONCURRENCIES:
        want = {1: 3, 2: max(d, 3)}.get(concurrency, 6)
        check(full, concurrency, want)
        check(short, concurrency, {1: 3}.get(concurrency, 6))
    # two cells a point short each: their common ancestors hold 199 998 points, only children of the root have none
    check(sibling_counts(d, LARGE - 1, LARGE - 1, DEEP_PATH[:d], "x", d), 1, 6 if d == 1 else 3)


# ------------------------------------------------------------------------------------------ the score at 1.0 and just below
def _children(path, k):
    """k children of the node `path` (octant digits), octants 7, 6, ..."""
    return [list(path) + [7 - o] for o in range(k)]


@pytest.mark.parametrize("concurrency", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("depth", [1, 3, 4, 6])
def test_score_exactly_one_and_just_below(concurrency, depth):
    """`concurrency` large sibling cells of one depth: large / concurrency == 1.0, S = max(depth, 3).  One of them a point
    short, or one of them missing: (concurrency - 1) / concurrency, 6.  Odd thread counts divide by two rounding down."""
    cells = _children(DEEP_PATH[:depth - 1], concurrency)
    full = [(c, LARGE) for c in cells]
    want = 3 if concurrency == 1 else max(depth, 3)  # (one thread: the one range of depth 1 is large already)
    check(cells_to_counts(full, depth), concurrency, want)
    below = full[:-1] + [(cells[-1], LARGE - 1)]
    check(cells_to_counts(below, depth), concurrency, 6)
    if concurrency > 1:
        check(cells_to_counts(full[:-1], depth), concurrency, 6)
        # one large cell more than threads: the score passes 1.0
        if concurrency < 8:
            check(cells_to_counts(full + [(_children(DEEP_PATH[:depth - 1], concurrency + 1)[-1], LARGE)], depth), concurrency, want)
        # half as many ranges as threads (rounded down), all large: the condition on the ranges holds the score at 0
        check(cells_to_counts(full[:concurrency // 2], depth), concurrency, 6)


def test_sixty_four_threads():
    """64 large cells of depth 2 (all of them) score 1.0 there: 3.  63 of them and one a point short: no depth has 64."""
    cells = [([a, b], LARGE) for a in range(8) for b in range(8)]
    check(cells_to_counts(cells, 1), 64, 3)
    check(cells_to_counts(cells[:-1] + [(cells[-1][0], LARGE - 1)], 1), 64, 6)
    # 64 large cells at depth 4 under eight different parents: depths 1 .. 3 see fewer than 64 large ranges
    deep = [([a, 1, 2, b], LARGE) for a in range(8) for b in range(8)]
    check(cells_to_counts(deep, 2), 64, 4)
    check(cells_to_counts(deep, 2), 65, 6)
    check(cells_to_counts(deep, 2), 63, 4)
    check(cells_to_counts(deep, 2), 8, 3)   # eight large ranges of depth 1


def test_as_many_threads_as_a_uint32_holds():
    """2^32 - 1 threads: float(concurrency) is 2^32, no histogram has that many large ranges."""
    # every cell of depth 5 large (100 000 points in its first bin, 3 276 800 000 in all): the most large ranges a total
    # below 2^32 has room for at one depth
    everywhere = np.zeros(NBINS, dtype=np.uint64)
    everywhere[::8] = LARGE
    for counts in (sibling_counts(4, LARGE, LARGE), everywhere, np.zeros(NBINS, dtype=np.uint64)):
        check(counts, 2 ** 32 - 1, 6)
    check(everywhere, 32768, 5)   # as many threads as large ranges of depth 5: 1.0
    check(everywhere, 32769, 6)   # one thread more
    check(everywhere, 4096, 4)
    check(everywhere, 4097, 5)
    check(everywhere, 512, 3)
    check(everywhere, 513, 4)


# ------------------------------------------------------------------------------------------ deeper levels
def test_a_shallower_depth_fails_and_a_deeper_one_passes():
    # four cells of depth 4 under one parent, four threads: depths 1 .. 3 see one range
    four = [(DEEP_PATH[:3] + [o], LARGE) for o in (0, 3, 5, 6)]
    check(cells_to_counts(four, 3), 4, 4)
    check(cells_to_counts(four, 3), 2, 4)     # (two threads: four ranges, score 2.0, at depth 4 as well)
    check(cells_to_counts(four, 3), 5, 6)
    check(cells_to_counts(four[:3] + [(four[3][0], LARGE - 1)], 3), 4, 6)
    # two large cells of depth 3 with two large cells of depth 5 inside each: two threads stop at 3, four go on to 5
    nested = [(DEEP_PATH[:2] + [a] + [4, b], LARGE) for a in (1, 6) for b in (2, 7)]
    check(cells_to_counts(nested, 4), 2, 3)
    check(cells_to_counts(nested, 4), 4, 5)
    check(cells_to_counts(nested, 4), 3, 5)
    # the large ranges of a shallow depth dissolve further down: 3 threads, 3 large cells of depth 3 made of small bins
    check(cells_to_counts([(DEEP_PATH[:2] + [o], LARGE) for o in (0, 1, 2)], 5), 3, 3)
    # cells of several depths at once.  Depth 1: three ranges, [1] and [2] large; depth 2: [0, *] (eight ranges of some 12 500),
    # [1, 1], [1, 2] and [2, 0] large; depth 4: [2, 0, 0, 0 .. 2] large, the cells of depth 2 have dissolved; depth 5: none
    mixed = [([0], LARGE - 1), ([1, 1], LARGE), ([1, 2], LARGE), ([2, 0, 0, 0], LARGE), ([2, 0, 0, 1], LARGE), ([2, 0, 0, 2], LARGE)]
    check(cells_to_counts(mixed, 6), 2, 3)   # depth 1: 2 / 2
    check(cells_to_counts(mixed, 6), 3, 3)   # depth 2: 3 / 3, and the floor of 3
    check(cells_to_counts(mixed, 6), 4, 6)   # never four large ranges


def test_many_small_ranges_and_no_points():
    ones = np.ones(NBINS, dtype=np.uint64)
    zeros = np.zeros(NBINS, dtype=np.uint64)
    for concurrency in CONCURRENCIES:
        check(ones, concurrency, 6)
        check(zeros, concurrency, 6)
    assert int(ones.reshape(8, -1).sum(axis=1)[0]) == 32768   # per child of the root
    check(ones * np.uint64(4), 1, 3)          # eight ranges of 131 072 at depth 1
    check(ones * np.uint64(4), 8, 3)
    check(ones * np.uint64(4), 9, 6)
    check(ones * np.uint64(3), 1, 6)          # 98 304 each: none is large, and deeper ranges are smaller still
    one_bin = zeros.copy()
    one_bin[NBINS - 1] = LARGE
    check(one_bin, 1, 3)
    check(one_bin, 2, 6)
    one_bin[NBINS - 1] = LARGE - 1
    check(one_bin, 1, 6)


def test_first_and_last_bins():
    """The cells at the two ends of the histogram: bin 0 with its neighbour along x, bin 2^18 - 1 with its own."""
    for path in ([0] * 6, [7] * 6):
        for axis in AXES:
            full = sibling_counts(6, LARGE, LARGE, path, axis)
            assert int(full[prefix_of(path)]) == LARGE and int(np.count_nonzero(full)) == 2
            check(full, 2, 6)
            for d in (3, 4, 5):
                check(sibling_counts(d, LARGE, LARGE, path[:d], axis, d), 2, d)
                check(sibling_counts(d, LARGE, LARGE - 1, path[:d], axis, d), 2, 6)
                check(sibling_counts(d, LARGE - 1, LARGE, path[:d], axis, d), 2, 6)


# ------------------------------------------------------------------------------------------ random histograms
@pytest.mark.parametrize("seed", range(6))
def test_random_histograms_agree_with_the_restatement(seed):
    """Cells of random depth with counts around the threshold, on a background of small bins."""
    rng = np.random.default_rng(seed)
    cells = []
    for _ in range(int(rng.integers(1, 40))):
        depth = int(rng.integers(1, 7))
        cells.append(([int(v) for v in rng.integers(0, 8, depth)], int(LARGE + rng.integers(-2, 3))))
    counts = cells_to_counts(cells, seed, spread=bool(seed % 2))
    if seed >= 3:
        counts += rng.integers(0, 3, NBINS).astype(np.uint64)
    seen = {check(counts, concurrency) for concurrency in CONCURRENCIES + [6, 7, 9, 16, 33]}
    assert 6 in seen  # (2^32 - 1 threads)


# ------------------------------------------------------------------------------------------ split across ranks
@pytest.mark.parametrize("parts", [1, 4, 7])
def test_counts_split_across_ranks_sum_to_the_same_level(parts):
    """The function sees only the sum: the same histogram dealt out to 1, 4 and 7 ranks at random."""
    rng = np.random.default_rng(parts)
    for d, nb, want in ((4, LARGE, 4), (5, LARGE, 5), (5, LARGE - 1, 6), (3, LARGE, 3)):
        counts = sibling_counts(d, LARGE, nb, DEEP_PATH[:d], "y", d)
        left = counts.copy()
        shares = []
        for r in range(parts - 1):
            take = rng.binomial(left.astype(np.int64), 1.0 / (parts - r)).astype(np.uint64)
            shares.append(take)
            left -= take
        shares.append(left)
        total = np.zeros(NBINS, dtype=np.uint64)
        for s in shares:
            total += s
        assert np.array_equal(total, counts)
        check(total, 2, want)
        if parts > 1:  # no rank alone would vote like the sum
            assert {library_level(s, 2) for s in shares} == {6}


# ------------------------------------------------------------------------------------------ large totals
def test_totals_up_to_two_to_the_32():
    """The header documents totals below 2^32 (the estimate keeps 32-bit prefix sums)."""
    top = 2 ** 32 - 1
    # two sibling bins that hold almost everything
    check(cells_to_counts([([7] * 6, top - LARGE), ([7] * 5 + [3], LARGE)], spread=False), 2, 6)
    check(cells_to_counts([(DEEP_PATH[:3], top - LARGE), (sibling_path(DEEP_PATH[:3], "x", 3), LARGE)], spread=False), 2, 3)
    check(cells_to_counts([(DEEP_PATH[:4], top - LARGE + 1), (sibling_path(DEEP_PATH[:4], "x", 4), LARGE - 1)], spread=False), 2, 6)
    # the threshold at the far end of the prefix sums: the last cell's count is (2^32 - 1) - its start
    check(cells_to_counts([([0] * 4, top - LARGE), ([7, 7, 7, 3], LARGE)], spread=False), 2, 3)   # depth 1 separates them already
    check(cells_to_counts([([7, 7, 7, 3], top - LARGE), ([7] * 4, LARGE)], spread=False), 2, 4)
    check(cells_to_counts([([7, 7, 7, 3], top - LARGE), ([7] * 4, LARGE - 1)], spread=False), 2, 6)
    # every bin filled: 16 383 points per bin, 2^32 - 2^18 in all
    even = np.full(NBINS, 16383, dtype=np.uint64)
    assert int(even.sum()) == 2 ** 32 - 2 ** 18
    check(even, 8, 3)       # depth 1: eight ranges of 536 million
    check(even, 4096, 4)    # depth 4: 4 096 ranges of 1 048 512
    check(even, 4097, 5)    # depth 5: 32 768 ranges of 131 064
    check(even, 32769, 6)   # depth 6: none of the 262 144 ranges is large


# ------------------------------------------------------------------------------------------ real clouds: the oracle's own estimate
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6])
def test_histograms_of_real_clouds_against_the_oracle(d):
    """The histogram of a sibling cloud's keys, split over four ranks; the oracle estimates from the sorted keys themselves."""
    for nb, axis in ((LARGE, "x"), (LARGE - 1, "z")):
        path = DEEP_PATH[:d]
        xyz = sibling_cloud(d, LARGE, nb, 7 * d, path=path, axis=axis)
        keys, _ = O.index_points(xyz, *UNIT)
        bins = (keys >> np.uint64(45)).astype(np.int64)
        counts = np.zeros(NBINS, dtype=np.uint64)
        for part in np.array_split(np.arange(xyz.shape[0]), 4):
            counts += np.bincount(bins[part], minlength=NBINS).astype(np.uint64)
        cells = np.unique(bins >> (3 * (6 - d)))
        assert cells.tolist() == sorted([prefix_of(path), prefix_of(sibling_path(path, axis, d))])
        for concurrency in (1, 2, 3):
            want = {1: 3, 2: max(d, 3) if nb == LARGE else 6, 3: 6}[concurrency]  # (one thread: the first cell alone is large)
            got = check(counts, concurrency, want)
            o = O.tile(xyz, *UNIT, O.RANDOM_GRID, 20000, O.spacing_from_diagonal(*UNIT, 8), strategy=O.FAST, fast_concurrency=concurrency)
            assert o["status"] == 0 and o["stats"]["fast_start_levels"] == got
            assert int(o["level"].min()) == got - 1


# ------------------------------------------------------------------------------------------ the condition on the ranges
def test_ranges_condition_never_decides():
    """Whenever large >= concurrency there are more ranges than concurrency / 2.  The histograms closest to the condition --
    exactly concurrency / 2 ranges (rounded down), all large, and one range more -- vote what the score alone says."""
    for concurrency in (2, 3, 4, 5, 8, 9):
        half = concurrency // 2
        cells = [([o], LARGE) for o in range(half)]
        check(cells_to_counts(cells, 0), concurrency, 6)                              # half / concurrency < 1
        check(cells_to_counts(cells + [([half], LARGE)], 0), concurrency, 3 if half + 1 >= concurrency else 6)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    import schwarzwald_amd as swz
    L = swz.load_library()
    counts = sibling_counts(4, LARGE, LARGE)
    out = C.c_int32(-7)
    ptr = counts.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.swz_fast_start_level_from_counts(ptr, 0, C.byref(out)) == swz.api.ERR_BAD_ARG and out.value == -7
    assert L.swz_fast_start_level_from_counts(None, 2, C.byref(out)) == swz.api.ERR_BAD_ARG and out.value == -7
    assert L.swz_fast_start_level_from_counts(ptr, 2, None) == swz.api.ERR_BAD_ARG
    assert L.swz_fast_start_level_from_counts(ptr, 2, C.byref(out)) == 0 and out.value == 4
    with pytest.raises(swz.SwzError) as e:
        swz.api.fast_start_level_from_counts(counts, 0)
    assert e.value.code == swz.api.ERR_BAD_ARG
