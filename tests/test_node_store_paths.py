"""The node store of the multi-batch tiler (swz_tlevel.hip, swz_tstore.hip, the store half of swz_treroot.hip) at its edges:
merge (tl_merge_rank_kernel), pull (level_pull, tl_gather_files_kernel), store (level_store, store_compact, store_linearize,
tl_table_merge_kernel) and re-rooting against a populated store (tl_touch_kernel, SplitG, rr_store_node).

Every case is a list of batches on a power-of-two box whose points lie on centres of the 2^21 key grid (node_store_ref.py), so
no rounding takes part; node table and file contents are compared exactly with oracle_lib.Tiler.  Each case has two tests:
  test_premise[case]   no GPU: the traced restatement (node_store_ref.StoreTrace) agrees with O.Tiler on the case's input, and
                       the quantity that decides the path -- run lengths, the widest bracket of a merge workgroup against
                       swz_tiler_merge_lds(), the segments a gather workgroup spans against swz_tiler_gather_lds(), file
                       lengths -- lies on the intended side;
  test_gpu[case]       the library's files are the oracle's, rekey_inversions == 0, the oracle's unsorted_cached_nodes counts
                       nothing but terminal nodes (which append new ++ cached and are read back as they are), and the path
                       counters (swz_tiler_path_counts) the case is named after moved.

Path counter -> the GPU cases that assert it non-zero:
  pull_in_place       A1-*, A2-*, A3-*, B1-in-place (three levels)
  pull_gathered       B2-confined, B3-lengths, B4-*, C1-log, C2-compaction
  pull_whole_file     test_gpu_reroot_into_populated_level (D)
  resort              test_gpu_resort_counter_sees_the_constructed_inversion
  compact_full        C2-compaction, test_gpu_compaction_is_deterministic_and_survives_poison (E)
  linearize_moved     C1-log, C2-compaction (node table / export after log form; zero before them)
  append_behind       every case with more than one batch
  table_merge_nf0     every case (the root's table has one entry and the batch rewrites it)
  linearize_moved by RE-ROOTING (C.3's other half): cannot happen in the unsharded tiler.  rr_node linearizes its level before it
    splits it, but the levels from the first re-rooted one on are written by rr_store_node alone, always as a whole (linear):
    the level loop leaves for tiler_reroot_level there and never appends to them.  D asserts the counter ZERO before
    node table and export.
  A5-*: meant to read positions through the working pool (work_need_positions, tl_fill_kernel: MIN_DISTANCE, and GRID_CENTER
    on bounds that are no cube).  No counter observes that; they get there by construction only.
  rekey, table_merge_heads0: no sequence of calls of the unsharded tiler reaches them -- the level loop never pulls a level
    that re-rooting or finalize wrote (it leaves for tiler_reroot_level at that level, and no batch follows finalize), and
    every node takes at least one point, so a level step that stores always has a new file.  Every case asserts them ZERO:
    the day one of them moves, a case for it is missing here.
"""
import functools

import numpy as np
import pytest

import node_store_ref as R
import oracle_lib as O

CUBE = ([0.0, 0.0, 0.0], [1024.0, 1024.0, 1024.0])
SLAB = ([0.0, 0.0, 0.0], [1024.0, 1024.0, 512.0])  # no cube: the samplers read positions, the working pool is filled
HALF = R.CELLS // 2
UNREACHABLE = ("rekey", "table_merge_heads0")


def _spacing(g):
    """the root's sampling grid has 2^g cells per axis (and so has every node's)"""
    return float(np.float32(1024.0 / 2 ** g))


def _consts():
    from schwarzwald_amd import api
    return api.tiler_merge_tile(), api.tiler_merge_lds(), api.tiler_gather_lds()


def _case(cells, bounds=CUBE, sampler=O.RANDOM_GRID, max_points=3000, g=4, max_depth=100):
    return dict(bounds=bounds, sampler=sampler, max_points=max_points, spacing=_spacing(g), max_depth=max_depth,
                batches=[R.points_of_cells(c, bounds) for c in cells], cells=cells)


# --------------------------------------------------------------------------------------------------- the cases
def _a1(nc, m):
    """root file of nc entries (a first batch below max_points is taken whole), second batch of m points"""
    rng = np.random.default_rng(1000 + 7 * nc + m)
    c = R.random_cells(rng, nc + m)
    return _case([c[:nc], c[nc:]] if nc else [c])


def _a2(big_first, sampler=O.RANDOM_GRID, bounds=CUBE):
    small, big = R.lattice(8, offset=5000), R.lattice(16, offset=700)   # 512 / 4096 points, one per root cell at most
    extra = R.random_cells(np.random.default_rng(3), 700)
    # (4096 > max_points: the root samples its 16^3 grid and takes all 4096; 512 <= max_points: taken whole)
    return _case([big, small, extra] if big_first else [small, big, extra], bounds=bounds, sampler=sampler)


def _a3(kind):
    rng = np.random.default_rng(31)
    c = R.random_cells(rng, 7000)
    if kind == "edges":       # the second batch repeats the entries 1019..1029 of the root file, as ITS entries 1019..1029
        first = c[:3000]
        order = np.argsort(R.keys_of_cells(first), kind="stable")
        twins = first[order[1019:1030]]
        tk = R.keys_of_cells(twins)
        rest = c[3000:]
        rk = R.keys_of_cells(rest)
        below, above = rest[rk < tk[0]], rest[rk > tk[-1]]
        assert len(below) >= 1019
        return _case([first, np.vstack([below[:1019], twins, above[:400]])], max_depth=3)
    if kind == "new-stack":   # 1500 new points on one cached key: whole tiles of the new run are one key
        first = c[:3000]
        return _case([first, np.vstack([c[3000:3300], np.repeat(first[5:6], 1500, axis=0)])], max_depth=3)
    # "cached-stack": 2500 cached points on one key against one new point on it
    first = np.vstack([np.repeat(c[0:1], 2500, axis=0), c[1:400]])
    return _case([first, np.vstack([c[0:1], c[3000:3050]])], max_depth=3)


def _a4():
    """level 0 terminal: 8 nodes that append new ++ cached; three batches of ~1000 points per node"""
    rng = np.random.default_rng(44)
    c = R.random_cells(rng, 24000)
    return _case([c[:8000], c[8000:16000], c[16000:]], max_points=4, g=1, max_depth=0)


def _b1():
    rng = np.random.default_rng(51)
    c = R.random_cells(rng, 30000)
    return _case([c[:15000], c[15000:]], max_points=50, g=2)


def _b2():
    rng = np.random.default_rng(52)
    return _case([R.random_cells(rng, 15000), R.random_cells(rng, 6000, hi=(HALF, HALF, HALF))], max_points=50, g=2)


def _octant_box(o):
    lo = np.array([(o >> 2) & 1, (o >> 1) & 1, o & 1]) * HALF
    return lo, lo + HALF


def _b3():
    """level 0 terminal; the root (8 cells) takes the first point of every octant: files of 255, 256, 257 and 1 entries in
    octants 0..3 (and 300 in 4..7, which the second batch does not reach)"""
    rng = np.random.default_rng(53)
    first = [R.random_cells(rng, n + 1, *_octant_box(o)) for o, n in enumerate([255, 256, 257, 1, 300, 300, 300, 300])]
    second = [R.random_cells(rng, 40, *_octant_box(o)) for o in range(4)]
    return _case([np.vstack(first), np.vstack(second)], max_points=4, g=1, max_depth=0)


def _b4(kind):
    """level 3 terminal, 4096 nodes of 2^17 cells per axis; the first batch leaves files in two of them, the second reaches
    only the first of them -- the level is in log form from then on, so the third is gathered and not read in place --, the
    third reaches both and many nodes without a file between (or around) them"""
    rng = np.random.default_rng(54)
    w = R.CELLS // 16
    at = (1, 14) if kind == "global-open-ends" else (0, 15)   # node coordinates on the cube's diagonal
    first = np.vstack([R.random_cells(rng, 60, (a * w,) * 3, (a * w + w,) * 3) for a in at])
    per = 16 if kind != "lds" else 6
    # 6 points in every reached node: 4 may be taken on the way down (root, levels 0, 1, 2 take one per cell = per node below)
    nodes = R.lattice(per, lo=0, hi=R.CELLS) if kind != "lds" else R.lattice(6, lo=0, hi=6 * w)
    if kind == "lds":
        nodes = np.vstack([nodes, [[15 * w] * 3]])
    second = np.vstack([nodes + rng.integers(0, w, (len(nodes), 3)) // 2 * 2 + k % 2 for k in range(6)])
    _, i = np.unique(R.keys_of_cells(second), return_index=True)
    middle = R.random_cells(rng, 10, (at[0] * w,) * 3, (at[0] * w + w,) * 3)
    return _case([first, middle, second[np.sort(i)]], max_points=4, g=1, max_depth=3)


def _level1_box(j):
    """cells of the j-th level-1 node in Morton order (64 nodes, 2^19 cells per axis)"""
    x = ((j >> 5) & 1) * 2 + ((j >> 2) & 1)
    y = ((j >> 4) & 1) * 2 + ((j >> 1) & 1)
    z = ((j >> 3) & 1) * 2 + (j & 1)
    lo = np.array([x, y, z]) * (R.CELLS // 4)
    return lo, lo + R.CELLS // 4


def _c1():
    """level 1 terminal (64 nodes).  Batch 2 writes files before, between and behind the three that batch 1 left and pulls
    none of them; batch 3 rewrites one old and one new file out of the log"""
    rng = np.random.default_rng(61)
    put = lambda nodes: np.vstack([R.random_cells(rng, 60, *_level1_box(j)) for j in nodes])
    return _case([put([10, 30, 50]), put([5, 20, 40, 60]), put([10, 20, 55])], max_points=4, g=1, max_depth=1)


C2_CAP = 8     # batches within which a side of level 0 must have run full
C2_AFTER = 2   # batches that then pull from the compacted side


def _c2(batches=C2_CAP + C2_AFTER):
    """level 0 terminal; batches alternate between octants 0 and 7"""
    rng = np.random.default_rng(62)
    return _case([R.random_cells(rng, 3000, *_octant_box(0 if b % 2 == 0 else 7)) for b in range(batches)],
                 max_points=4, g=1, max_depth=0)


CASES = {
    "A1-nc0-m1025": lambda: _a1(0, 1025),
    "A1-nc1-m2049": lambda: _a1(1, 2049),
    "A1-nc1023-m1025": lambda: _a1(1023, 1025),
    "A1-nc1024-m1024": lambda: _a1(1024, 1024),
    "A1-nc1025-m1023": lambda: _a1(1025, 1023),
    "A1-nc2049-m1": lambda: _a1(2049, 1),
    "A2-small-batch-on-big-file": lambda: _a2(True),
    "A2-big-batch-on-small-file": lambda: _a2(False),
    "A3-ties-at-tile-edge": lambda: _a3("edges"),
    "A3-new-stack": lambda: _a3("new-stack"),
    "A3-cached-stack": lambda: _a3("cached-stack"),
    "A4-terminal": _a4,
    "A5-min-distance": lambda: _a2(True, O.MIN_DISTANCE),
    "A5-grid-center-slab": lambda: _a2(False, O.GRID_CENTER, SLAB),
    "B1-in-place": _b1,
    "B2-confined": _b2,
    "B3-lengths": _b3,
    "B4-lds": lambda: _b4("lds"),
    "B4-global": lambda: _b4("global"),
    "B4-global-open-ends": lambda: _b4("global-open-ends"),
    "C1-log": _c1,
    "C2-compaction": _c2,
}


@functools.lru_cache(maxsize=None)
def _built(name):
    """(case, oracle export, oracle counts, trace): computed once, shared by the premise and the GPU test, never changed"""
    case = CASES[name]()
    return (case,) + _oracle(case) + (_trace(case),)


def _oracle(case, upto=None):
    t = O.Tiler(case["bounds"][0], case["bounds"][1], case["sampler"], case["max_points"], case["spacing"], max_depth=case["max_depth"])
    for b in case["batches"][:upto]:
        assert t.add_batch(b) == 0
    assert t.finalize() == 0
    ex, c = t.export(), t.counts()
    t.close()
    return ex, c


def _trace(case):
    tr = R.StoreTrace(case["bounds"], case["sampler"], case["max_points"], case["spacing"], case["max_depth"])
    for b in case["batches"]:
        tr.add_batch(b)
    return tr


def _files(table, ids):
    return {(int(l), int(k)): ids[int(o):int(o + c)].tolist()
            for l, k, o, c in zip(table["level"], table["key"], table["offset"], table["count"])}


# --------------------------------------------------------------------------------------------------- premises (no GPU)
def _premise(name, case, tr, ex):
    tile, lds, seg_lds = _consts()
    nb = len(case["batches"])
    root = lambda b: tr.level_runs(b, -1)
    if name.startswith("A1"):
        nc, m = [int(s.lstrip("ncm")) for s in name.split("-")[1:]]
        new, old, _, _ = root(nb - 1)
        assert (len(old), len(new)) == (nc, m)
        assert tile == 1024  # (the run lengths of these cases are written around it)
    elif name.startswith("A2") or name.startswith("A5"):
        new, old, _, _ = root(1)
        wa, wb = R.merge_brackets(new, old, 0, tile)
        if len(new) <= 1024:
            assert len(old) >= 4096 and wa > lds >= wb, (wa, wb)   # new in cached: global memory; cached in new: LDS
        else:
            assert len(old) <= 1024 and wb > lds >= wa, (wa, wb)
    elif name == "A3-ties-at-tile-edge":
        new, old, _, _ = root(1)
        assert np.array_equal(new[1019:1030], old[1019:1030]) and len(new) > 1030   # ties at elements 1023 and 1024 of both runs
        base = len(case["batches"][0])
        f = _files(ex, ex["ids"])[(-1, 0)]
        keys = R.keys_of_cells(np.vstack(case["cells"]))
        won = [i for i in f if i >= base and keys[i] in set(old[1019:1030].tolist())]
        assert len(won) >= 2, "the root's file should hold new twins"
    elif name == "A3-new-stack":
        new, old, _, _ = root(1)
        k, n = np.unique(new, return_counts=True)
        assert n.max() > tile and k[n.argmax()] in old
    elif name == "A3-cached-stack":
        new, old, _, _ = root(1)
        k, n = np.unique(old, return_counts=True)
        assert n.max() > lds and int((new == k[n.argmax()]).sum()) == 1
    elif name == "A4-terminal":
        new, old, nodes, lens = tr.level_runs(2, 0)
        assert max(lens) > lds and len(nodes) == 8
        starts = np.cumsum([0] + [len(n[1]) for n in tr.batches[2][0]])
        inside = [e for e in range(tile, len(new), tile) if not np.any(starts == e)]
        assert inside, "a tile edge of the new run inside a node"
        wa, wb = R.merge_brackets(new, old, R.node_shift(0), tile)
        assert wa > lds   # a workgroup's new points span nodes whose cached files exceed the LDS bracket
        # the cached part of the third batch is itself batch 2 ++ batch 1
        f = _files(ex, ex["ids"])[(0, 0)]
        b1, b2 = len(case["batches"][0]), len(case["batches"][0]) + len(case["batches"][1])
        part = np.digitize(f, [b1, b2])
        # (points of earlier batches that the root displaced arrive as "new" ones: the head is not batch 3 alone)
        head, tail = part[:len(f) - lens[0]], part[len(f) - lens[0]:]
        assert int((head == 2).sum()) == int((part == 2).sum()) > 0 and set(tail) == {0, 1}
    elif name == "B1-in-place":
        for level in (-1, 0, 1):
            have = tr.files_before(1, level)
            reached = set(tr.level_runs(1, level)[2])
            assert have and set(have) <= reached, level
    elif name == "B2-confined":
        have, reached = tr.files_before(1, 0), set(tr.level_runs(1, 0)[2])
        assert len(have) == 8 and len(reached & set(have)) == 1
    elif name == "B3-lengths":
        _, _, nodes, lens = tr.level_runs(1, 0)
        assert lens == [255, 256, 257, 1] and len(tr.files_before(1, 0)) == 8
    elif name.startswith("B4"):
        assert tr.level_runs(1, 3)[3] == [tr.files_before(1, 3)[tr.level_runs(1, 3)[2][0]]] and len(tr.files_before(1, 3)) == 2
        _, _, nodes, lens = tr.level_runs(2, 3)
        span = R.gather_span(lens)
        assert sum(1 for n in lens if n) == 2 and lens.count(0) == len(lens) - 2
        i, j = [k for k, n in enumerate(lens) if n]
        if name == "B4-lds":
            assert 2 < span <= seg_lds and span == len(lens) and (i, j) == (0, len(lens) - 1), span
        elif name == "B4-global":
            assert span > seg_lds and (i, j) == (0, len(lens) - 1), span
        else:
            assert span > seg_lds and i > 0 and j < len(lens) - 1, (span, i, j)   # first and last head have no file
    elif name == "C1-log":
        have = sorted(tr.files_before(1, 1))
        _, _, reached, lens = tr.level_runs(1, 1)
        assert len(have) == 3 and not set(have) & set(reached)
        assert min(reached) < have[0] and max(reached) > have[2]
        assert any(have[0] < k < have[1] for k in reached) and any(have[1] < k < have[2] for k in reached)
        lens3 = tr.level_runs(2, 1)[3]
        assert sorted(n > 0 for n in lens3) == [False, True, True]   # batch 3: an old file, a new file, a node without one
    elif name == "C2-compaction":
        for b in range(nb):
            assert tr.level_runs(b, 0)[2] == [(0 if b % 2 == 0 else 7) << 60]
    else:
        raise AssertionError("no premise for " + name)


@pytest.mark.parametrize("name", list(CASES))
def test_premise(name):
    case, ex, c, tr = _built(name)
    # the restatement the premise is computed from is the oracle, file for file
    mine = R.M.files_table({k: v for k, v in tr.files.items()})
    for col in ("level", "key", "offset", "count", "ids"):
        assert np.array_equal(mine[col], ex[col]), col
    # (no internal node reads a file back out of order; what the oracle counts are terminal nodes, which append new ++ cached)
    assert tr.unsorted_cached_nodes == 0 and c["unsorted_cached_nodes"] == tr.unsorted_terminal
    n = sum(len(b) for b in case["batches"])
    assert c["num_stored"] == n and np.array_equal(np.sort(ex["ids"]), np.arange(n, dtype=np.uint32))
    _premise(name, case, tr, ex)


# --------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def _gpu(ctx, case, upto=None, after_batch=None):
    """the library's files of a case: dict(table, ids, level, info, paths, keys)"""
    import schwarzwald_amd as swz
    import torch
    params = swz.TileParams(sampler=case["sampler"], max_points_per_node=case["max_points"], spacing_at_root=case["spacing"],
                            max_depth=case["max_depth"])
    with swz.Tiler(ctx, case["bounds"][0], case["bounds"][1], params) as t:
        for i, b in enumerate(case["batches"][:upto]):
            d = torch.from_numpy(np.ascontiguousarray(b)).cuda()
            torch.cuda.synchronize()
            t.add_batch_device(d.data_ptr(), b.shape[0])
            if after_batch and after_batch(i, t):
                break
        batches_run = i + 1
        before_export = t.path_counts()
        t.finalize()
        info, table = t.info(), t.node_table()
        ns = int(info["num_stored"])
        d_keys = torch.empty(max(ns, 1), dtype=torch.int64, device="cuda")
        d_ids = torch.empty(max(ns, 1), dtype=torch.int32, device="cuda")
        d_lvl = torch.empty(max(ns, 1), dtype=torch.int8, device="cuda")
        t.export_device(d_keys.data_ptr(), d_ids.data_ptr(), d_lvl.data_ptr())
        paths = t.path_counts()
    return dict(table=table, ids=d_ids.cpu().numpy().view(np.uint32)[:ns], level=d_lvl.cpu().numpy()[:ns], info=info,
                keys=d_keys.cpu().numpy().view(np.uint64)[:ns], paths=paths, before_export=before_export, batches=batches_run)


def _compare(g, ex, c):
    """as test_multibatch._compare: node table, file contents in file order, the exported level of every entry"""
    tb = g["table"]
    assert len(tb["level"]) == len(ex["level"]) == c["num_nodes"]
    for col in ("level", "key", "offset", "count"):
        assert np.array_equal(tb[col], ex[col]), col
    assert np.array_equal(g["ids"], ex["ids"])
    assert np.array_equal(g["level"], np.repeat(ex["level"], ex["count"].astype(np.int64)))


def _moved(paths, *names):
    for n in names:
        assert paths[n] > 0, "path %s was not taken: %s" % (n, paths)
    for n in UNREACHABLE:
        assert paths[n] == 0, "path %s is reachable after all -- add a case for it: %s" % (n, paths)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n != "C2-compaction"])
def test_gpu(ctx, name):
    case, ex, c, tr = _built(name)
    g = _gpu(ctx, case)
    assert g["info"]["rekey_inversions"] == 0 and c["unsorted_cached_nodes"] == tr.unsorted_terminal
    _compare(g, ex, c)
    n = sum(len(b) for b in case["batches"])
    assert np.array_equal(np.sort(g["ids"]), np.arange(n, dtype=np.uint32))   # every id exactly once
    p = g["paths"]
    _moved(p, "table_merge_nf0")
    if len(case["batches"]) > 1:
        _moved(p, "append_behind")
    if name[:2] in ("A1", "A2", "A3", "A5") and len(case["batches"]) > 1:
        _moved(p, "pull_in_place")
    if name == "B1-in-place":
        assert p["pull_in_place"] >= 3 and p["pull_gathered"] == 0, p
    if name[:2] in ("B2", "B3", "B4", "C1"):
        _moved(p, "pull_gathered")
    if name == "C1-log":
        assert g["before_export"]["linearize_moved"] == 0
        _moved(p, "linearize_moved")   # (export and node table turned the log into the linear form)


def _c2_gpu(ctx):
    """C.2 on a context: batches until compact_full moves (at most C2_CAP), then C2_AFTER more"""
    case = _built("C2-compaction")[0]
    state = {}

    def stop(i, t):
        if "full_at" not in state and t.path_counts()["compact_full"] > 0:
            state["full_at"] = i
        return "full_at" in state and i == state["full_at"] + C2_AFTER

    g = _gpu(ctx, case, after_batch=stop)
    assert "full_at" in state and state["full_at"] < C2_CAP, "no side ran full within %d batches: %s" % (C2_CAP, g["paths"])
    return case, g


@pytest.mark.gpu
def test_gpu_compaction(ctx):
    """C.2 / C.4 on a context of its own (a side's capacity is what earlier tilers of the context left behind)."""
    import schwarzwald_amd as swz
    own = swz.Context(0)
    try:
        case, g = _c2_gpu(own)
    finally:
        own.close()
    ex, c = _oracle(case, upto=g["batches"])
    assert g["info"]["rekey_inversions"] == 0   # (the oracle's counter: level 0 is terminal here, see test_premise)
    _compare(g, ex, c)
    n = sum(len(b) for b in case["batches"][:g["batches"]])
    assert np.array_equal(np.sort(g["ids"]), np.arange(n, dtype=np.uint32))
    _moved(g["paths"], "compact_full", "pull_gathered", "append_behind", "linearize_moved", "table_merge_nf0")


@pytest.mark.gpu
def test_gpu_compaction_is_deterministic_and_survives_poison():
    """E: case C.2 twice on fresh tilers of one context: identical bytes; once more with SWZ_POISON: store or table memory
    that nobody wrote cannot read as zeros."""
    import schwarzwald_amd as swz
    case = _built("C2-compaction")[0]
    own = swz.Context(0)
    try:
        _, a = _c2_gpu(own)
        b = _gpu(own, case, upto=a["batches"])
    finally:
        own.close()
    poisoned = swz.Context(0)
    try:
        poisoned.set_option("SWZ_POISON", "205")
        _, p = _c2_gpu(poisoned)
    finally:
        poisoned.close()
    assert a["batches"] == p["batches"]
    for other in (b, p):
        for col in ("level", "key", "offset", "count"):
            assert a["table"][col].tobytes() == other["table"][col].tobytes(), col
        for col in ("ids", "keys", "level"):
            assert a[col].tobytes() == other[col].tobytes(), col
    ex, c = _oracle(case, upto=a["batches"])
    _compare(p, ex, c)


# --------------------------------------------------------------------------------------------------- D: re-rooting
REROOT_LEVEL = 9   # spacing = extent / 4096: the grid samplers need more than 21 key levels from node level 9 on


def _d_case():
    """Three blobs 0.002 wide, each inside one level-9 node (1.0 wide): the middle one is the subject, the others put files of
    other level-9 nodes before and after it in Morton order.  Two batches: the second re-roots the same nodes again and
    takes their files out of the populated level."""
    rng = np.random.default_rng(71)
    blob = lambda at, n: at + rng.random((n, 3)) * 0.002
    first = np.vstack([blob(100.3, 1500), blob(612.3, 2500), blob(900.3, 1500)])
    second = np.vstack([blob(100.3, 300), blob(612.3, 900), blob(900.3, 300)])
    return dict(bounds=CUBE, sampler=O.RANDOM_GRID, max_points=200, spacing=float(np.float32(1024.0 / 4096.0)), max_depth=100,
                batches=[first[rng.permutation(len(first))], second[rng.permutation(len(second))]])


@functools.lru_cache(maxsize=None)
def _d_built():
    case = _d_case()
    return case, _oracle(case, upto=1), _oracle(case)


def test_premise_reroot():
    case, (ex1, c1), (ex, c) = _d_built()
    assert O.lib().orc_required_morton_index_depth(case["sampler"], REROOT_LEVEL, O._vec3(CUBE[0]), O._vec3(CUBE[1]),
                                                   O.C.c_float(case["spacing"])) >= 21
    assert O.lib().orc_required_morton_index_depth(case["sampler"], REROOT_LEVEL - 1, O._vec3(CUBE[0]), O._vec3(CUBE[1]),
                                                   O.C.c_float(case["spacing"])) < 21
    # Three files at the re-rooted level.  When the second batch re-roots the middle node, the level holds the first node's file
    # as that batch has just rewritten it (two batches: its final length), then the middle file of the first batch: that is what
    # tl_touch_kernel and SplitG see, and the middle file lies across a 256-entry boundary of it.
    at1, at = np.flatnonzero(ex1["level"] == REROOT_LEVEL), np.flatnonzero(ex["level"] == REROOT_LEVEL)
    assert len(at1) == 3 and np.array_equal(ex1["key"][at1], ex["key"][at])
    start = int(ex["count"][at[0]])
    end = start + int(ex1["count"][at1[1]])
    assert start > 0 and start // 256 != (end - 1) // 256 and start % 256 != 0, (start, end)
    # no file is read back out of order, so the library must not count an inversion either and every file must be the oracle's
    assert c1["unsorted_cached_nodes"] == 0 and c["unsorted_cached_nodes"] == 0
    assert int(ex1["level"].max()) > REROOT_LEVEL and int(ex["level"].max()) > REROOT_LEVEL
    n = sum(len(b) for b in case["batches"])
    assert c["num_stored"] == n and np.array_equal(np.sort(ex["ids"]), np.arange(n, dtype=np.uint32))


@pytest.mark.gpu
def test_gpu_reroot_into_populated_level(ctx):
    case, _, (ex, c) = _d_built()
    g = _gpu(ctx, case)
    n = sum(len(b) for b in case["batches"])
    assert np.array_equal(np.sort(g["ids"]), np.arange(n, dtype=np.uint32))
    assert g["info"]["rekey_inversions"] == 0 and c["unsorted_cached_nodes"] == 0   # (test_premise_reroot: the oracle's is 0)
    _compare(g, ex, c)
    _moved(g["before_export"], "pull_whole_file", "append_behind", "pull_in_place")
    # rr_node's store_linearize finds its level linear: only re-rooting writes the levels from REROOT_LEVEL on, as a whole
    assert g["before_export"]["linearize_moved"] == 0, g["before_export"]


@pytest.mark.gpu
def test_gpu_resort_counter_sees_the_constructed_inversion(ctx):
    """the one case that WANTS an inversion (test_multibatch's construction): the re-sort is counted where it happens"""
    import schwarzwald_amd as swz
    from test_multibatch import ODD, _inversion_batches
    batches, _, _ = _inversion_batches(ODD)
    params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=100, spacing_at_root=O.spacing_from_diagonal(*ODD, 250))
    with swz.Tiler(ctx, ODD[0], ODD[1], params) as t:
        for part in batches:
            t.add_batch(part)
        info, paths = t.info(), t.path_counts()
    assert info["rekey_inversions"] >= 1 and paths["resort"] >= 1
    assert info["num_stored"] == sum(len(p) for p in batches)
