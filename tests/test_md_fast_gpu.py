"""MIN_DISTANCE_FAST on the GPU against tests/md_fast_ref.py: per-node sample_points, whole tiles (ACCURATE, FAST, node
files), the multi-batch tiler, every MIN_DISTANCE algorithm on the candidate set, and what the sampler refuses."""
import numpy as np
import pytest

import md_fast_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
FAST4 = R.MIN_DISTANCE_FAST


@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def _params(max_points, spacing, **kw):
    import schwarzwald_amd as swz
    return swz.TileParams(sampler=swz.MIN_DISTANCE_FAST, max_points_per_node=max_points, spacing_at_root=spacing, **kw)


def _sorted(xyz):
    keys, xc = O.index_points(xyz, *UNIT)
    perm = O.sort_by_key(keys)
    return keys[perm], perm, xc


# ------------------------------------------------------------------------------------------- one node, root, n = 4
@pytest.fixture(scope="module")
def root_cloud():
    return _sorted(np.random.default_rng(41).random((1100, 3)))


MAXP = 64
ROOT_COUNTS = [1, 2, 3, 4, 5, MAXP, MAXP + 1, 400, 401, 402, 403] + list(range(1021, 1030))


@pytest.mark.parametrize("behaviour", [O.TAKE_ALL_WHEN_BELOW_MAX, O.ALWAYS_ADHERE])
def test_sample_points_root_counts(ctx, root_cloud, behaviour):
    """counts 4k .. 4k+3, around max_points, tiny ranges, and the last candidate in the last lane of a 256-thread block
    and in the first lane of the next (1021 .. 1029); AlwaysAdhere strides below max_points too"""
    import torch
    skeys, perm, xc = root_cloud
    sp = 0.09
    d_xyz = torch.from_numpy(xc).cuda()
    for count in ROOT_COUNTS:
        # (any Morton-contiguous part of the cloud is a sorted range of the root)
        k, i = skeys[7:7 + count], perm[7:7 + count]
        expect = R.sample_points(MAXP, k, i, xc, 0, -1, *UNIT, sp, behaviour)
        got = ctx.sample_points(FAST4, MAXP, k, i, xc, 0, -1, *UNIT, sp, behaviour)
        assert np.array_equal(got, expect), (count, behaviour)
        d_k = torch.from_numpy(k.view(np.int64).copy()).cuda()
        d_i = torch.from_numpy(i.view(np.int32).copy()).cuda()
        d_t = torch.zeros(count, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        num = ctx.sample_points_device(FAST4, MAXP, d_k.data_ptr(), d_i.data_ptr(), count, d_xyz.data_ptr(), xc.shape[0], 0, -1,
                                       *UNIT, sp, behaviour, d_t.data_ptr())
        assert np.array_equal(d_t.cpu().numpy(), expect) and num == int(expect.sum()), (count, behaviour)
        if behaviour == O.ALWAYS_ADHERE and 4 < count <= MAXP:
            assert not expect.all() and not expect[np.arange(count) % 4 != 0].any()
        if behaviour == O.TAKE_ALL_WHEN_BELOW_MAX and count <= MAXP:
            assert expect.all()


# ------------------------------------------------------------------------------------------- whole tiles
def _tile_equal(ctx, xyz, max_points, spacing, strategy=O.ACCURATE, concurrency=2, max_depth=100):
    S = None
    if strategy == O.FAST:
        S = O.tile(xyz, *UNIT, O.MIN_DISTANCE, max_points, spacing, max_depth=max_depth, strategy=O.FAST,
                   fast_concurrency=concurrency)["stats"]["fast_start_levels"]
    ref = R.tile(xyz, *UNIT, max_points, spacing, max_depth=max_depth, strategy=strategy, fast_start_level=S)
    got = ctx.tile(xyz, *UNIT, _params(max_points, spacing, strategy=strategy, fast_concurrency=concurrency, max_depth=max_depth))
    for name in ("keys", "perm", "level", "dup"):
        assert np.array_equal(getattr(got, name), ref[name]), name
    assert got.stats["num_nodes"] == ref["num_nodes"]
    if strategy == O.ACCURATE:
        assert got.stats["points_visited"] == ref["points_visited"]
    return got, ref


def _octant_cloud(rng, populations):
    """uniform points, populations[o] of them in level-0 octant o (bit 2 = x, bit 1 = y, bit 0 = z)"""
    parts = []
    for o, cnt in enumerate(populations):
        lo = np.array([(o >> 2) & 1, (o >> 1) & 1, o & 1]) * 0.5
        parts.append(lo + rng.random((cnt, 3)) * 0.5)
    xyz = np.vstack(parts)
    return xyz[rng.permutation(len(xyz))]


def test_level_zero_counts_from_the_nodes_own_first_point(ctx):
    """n = 2 at level 0: the candidates are counted from each node's own first element -- nodes that start at odd and at even
    offsets of the level, a sampled node next to a take-all node, nodes across 256-point block boundaries"""
    rng = np.random.default_rng(42)
    max_points = 400
    xyz = _octant_cloud(rng, [1503, 300, 1024, 777, 2, 1333, 395, 401])
    got, ref = _tile_equal(ctx, xyz, max_points, 0.2)
    below_root = ref["level"] != -1
    octant = (ref["keys"][below_root] >> np.uint64(60)).astype(np.int64)
    counts = np.bincount(octant, minlength=8)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    sampled = counts > max_points
    assert {int(s) % 2 for s in starts[sampled]} == {0, 1}, "the level-0 nodes must start at odd and at even offsets"
    assert any(sampled[o] != sampled[o + 1] for o in range(7)), "a sampled node next to a take-all node"
    assert any(starts[o] // 256 != (starts[o] + counts[o] - 1) // 256 and starts[o] % 256 for o in range(8) if sampled[o])
    assert (ref["level"] == 0).sum() < below_root.sum()  # and level 0 hands points down


@pytest.mark.parametrize("spacing,first_only_level", [(float(np.nextafter(np.float32(0.5), np.float32(1))), -1),
                                                      (float(np.nextafter(np.float32(0.5), np.float32(0))), None),
                                                      (float(np.nextafter(np.float32(1.0), np.float32(2))), 0),
                                                      (float(np.nextafter(np.float32(1.0), np.float32(0))), None)])
def test_first_point_only_rule(ctx, spacing, first_only_level):
    """candidate level -1 keeps the first point of a sampled node: spacing_at_root just above 0.5 on the unit cube switches
    it on at the root, just above 1.0 at level 0 (and the root); MIN_DISTANCE has no such rule"""
    import schwarzwald_amd as swz
    xyz = np.random.default_rng(43).random((6000, 3))
    got, ref = _tile_equal(ctx, xyz, 100, spacing)
    md = ctx.tile(xyz, *UNIT, swz.TileParams(sampler=swz.MIN_DISTANCE, max_points_per_node=100, spacing_at_root=spacing))
    assert not np.array_equal(got.level, md.level)
    at_root = int((got.level == -1).sum())
    per_node0 = np.bincount((got.keys[got.level == 0] >> np.uint64(60)).astype(np.int64), minlength=8)
    md_node0 = np.bincount((md.keys[md.level == 0] >> np.uint64(60)).astype(np.int64), minlength=8)
    if first_only_level == -1:
        assert at_root == 1 and (md.level == -1).sum() > 1
    elif first_only_level == 0:
        assert at_root == 1 and np.all(per_node0 == 1) and md_node0.sum() > 8
    elif spacing < 0.5:
        assert at_root > 1
    else:
        assert per_node0.sum() > 8


@pytest.fixture(scope="module")
def medium():
    rng = np.random.default_rng(44)
    xyz = rng.random((90000, 3))
    sp = O.spacing_from_diagonal(*UNIT, 60)
    return xyz, sp, R.tile(xyz, *UNIT, 800, sp)


@pytest.fixture(scope="module")
def clustered():
    """many points within a spacing of each other: rejections dominate"""
    rng = np.random.default_rng(45)
    centres = rng.random((300, 3))
    xyz = np.clip(centres[rng.integers(0, 300, 60000)] + 0.004 * rng.standard_normal((60000, 3)), 0.0, 1.0)
    sp = O.spacing_from_diagonal(*UNIT, 40)
    return xyz, sp, R.tile(xyz, *UNIT, 300, sp)


PATHS = {
    "default": {},
    "position sweep": {"SWZ_MD_KEYS": "0", "SWZ_MD_SPARSE_LIMIT": "0"},
    "key sweep": {"SWZ_MD_SPARSE_LIMIT": "0"},
    "key sweep, cells compacted": {"SWZ_MD_SPARSE_LIMIT": "0", "SWZ_MD_DIRECT": "0"},
    "key sweep, cells by grid code": {"SWZ_MD_SPARSE_LIMIT": "0", "SWZ_MD_DIRECT": "1"},
    "block path": {"SWZ_MD_SPARSE_LIMIT": "1000"},
    "thread per point": {"SWZ_MD_SPARSE_LIMIT": "1000", "SWZ_SP_BLOCK": "0"},
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("cloud", ["medium", "clustered"])
def test_every_min_distance_algorithm_on_the_candidate_set(ctx, request, path, cloud):
    xyz, sp, ref = request.getfixturevalue(cloud)
    max_points = 800 if cloud == "medium" else 300
    for k, v in PATHS[path].items():
        ctx.set_option(k, v)
    try:
        got = ctx.tile(xyz, *UNIT, _params(max_points, sp))
    finally:
        for k in PATHS[path]:
            ctx.set_option(k, None)
    assert np.array_equal(got.keys, ref["keys"]) and np.array_equal(got.perm, ref["perm"])
    assert np.array_equal(got.level, ref["level"])
    if cloud == "clustered":  # most of the root's candidates are rejected
        assert (ref["level"] == -1).sum() * 4 < len(range(0, len(xyz), 4))


@pytest.mark.parametrize("strategy", [O.ACCURATE, O.FAST])
def test_tile_uniform(ctx, strategy):
    xyz = np.random.default_rng(46).random((24001, 3))
    got, ref = _tile_equal(ctx, xyz, 500, O.spacing_from_diagonal(*UNIT, 50), strategy=strategy)
    if strategy == O.FAST:
        assert got.stats["fast_start_levels"] >= 2 and (ref["dup"] & 1).any() and (ref["dup"] & 2).any()


def test_tile_terminal_level(ctx):
    """max_depth ends the tree at level 1: everything left is kept there"""
    xyz = np.random.default_rng(47).random((20000, 3))
    got, ref = _tile_equal(ctx, xyz, 100, 0.05, max_depth=1)
    assert got.level.max() == 1


def test_tile_with_poisoned_workspace():
    import schwarzwald_amd as swz
    xyz = np.random.default_rng(48).random((50000, 3))
    sp = O.spacing_from_diagonal(*UNIT, 50)
    ref = R.tile(xyz, *UNIT, 700, sp)
    with swz.Context(0) as c:
        c.set_option("SWZ_POISON", "205")
        got = c.tile(xyz, *UNIT, _params(700, sp))
    assert np.array_equal(got.level, ref["level"]) and np.array_equal(got.perm, ref["perm"])


def _table_of_single_batch(ref):
    files = {}
    for i in range(len(ref["keys"])):
        lv = int(ref["level"][i])
        sh = (20 - lv) * 3 if lv >= 0 else 63
        key = ((int(ref["keys"][i]) >> sh) << sh) if lv >= 0 else 0
        files.setdefault((lv, key), []).append(int(ref["perm"][i]))
    return R.files_table(files)


def _compare_tables(table, ids, expect):
    for name in ("level", "key", "offset", "count"):
        assert np.array_equal(table[name], expect[name]), name
    assert np.array_equal(ids, expect["ids"])


def test_tile_nodes(ctx):
    import torch
    xyz = np.random.default_rng(49).random((40000, 3))
    sp = O.spacing_from_diagonal(*UNIT, 50)
    expect = _table_of_single_batch(R.tile(xyz, *UNIT, 300, sp))
    d = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    bufs = {}

    def alloc(ns):
        bufs["i"] = torch.empty(max(ns, 1), dtype=torch.int32, device="cuda")
        return None, bufs["i"].data_ptr(), None
    torch.cuda.synchronize()
    stats, table, ns = ctx.tile_nodes_device(d.data_ptr(), len(xyz), *UNIT, _params(300, sp), alloc)
    torch.cuda.synchronize()
    _compare_tables(table, bufs["i"].cpu().numpy().view(np.uint32)[:ns], expect)


# ------------------------------------------------------------------------------------------- the multi-batch tiler
def _gpu_tiler_files(ctx, parts, params, options=None):
    import torch
    import schwarzwald_amd as swz
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    try:
        with swz.Tiler(ctx, UNIT[0], UNIT[1], params) as t:
            for p in parts:
                d = torch.from_numpy(np.ascontiguousarray(p)).cuda()
                torch.cuda.synchronize()
                t.add_batch_device(d.data_ptr(), p.shape[0])
            t.finalize()
            info, table = t.info(), t.node_table()
            ns = int(info["num_stored"])
            d_ids = torch.empty(max(ns, 1), dtype=torch.int32, device="cuda")
            d_keys = torch.empty(max(ns, 1), dtype=torch.int64, device="cuda")
            d_lvl = torch.empty(max(ns, 1), dtype=torch.int8, device="cuda")
            t.export_device(d_keys.data_ptr(), d_ids.data_ptr(), d_lvl.data_ptr())
            return info, table, d_ids.cpu().numpy().view(np.uint32)[:ns]
    finally:
        for k in (options or {}):
            ctx.set_option(k, None)


@pytest.fixture(scope="module")
def uneven_batches():
    """four uneven batches: one lies entirely in one level-0 octant, one is empty"""
    rng = np.random.default_rng(50)
    parts = [rng.random((30000, 3)), 0.5 + 0.5 * rng.random((9000, 3)), np.zeros((0, 3)), rng.random((17003, 3))]
    sp = O.spacing_from_diagonal(*UNIT, 50)
    mb = R.MultiBatch(*UNIT, 400, sp)
    for p in parts:
        mb.add_batch(p)
    return parts, sp, R.files_table(mb.files)


@pytest.mark.parametrize("options", [None, {"SWZ_MD_SPARSE_LIMIT": "1000", "SWZ_SP_INCREMENTAL": "1e-9", "SWZ_SP_INCREMENTAL_MAX": "1.0"}],
                         ids=["default", "incremental forced"])
def test_tiler_accurate_uneven_batches(ctx, uneven_batches, options):
    parts, sp, expect = uneven_batches
    info, table, ids = _gpu_tiler_files(ctx, parts, _params(400, sp), options)
    assert info["rekey_inversions"] == 0
    _compare_tables(table, ids, expect)
    assert (expect["level"] >= 2).any()


def test_tiler_fast_batches(ctx):
    """every stored level >= 1 has n = 1: the oracle's MIN_DISTANCE FAST tiler; levels 0 and -1 are rebuilt from those files"""
    rng = np.random.default_rng(51)
    parts = [rng.random((25000, 3)), rng.random((11001, 3)), rng.random((14000, 3))]
    sp = O.spacing_from_diagonal(*UNIT, 50)
    t = O.Tiler(*UNIT, O.MIN_DISTANCE, 400, sp, strategy=O.FAST, fast_concurrency=4)
    for p in parts:
        assert t.add_batch(p) == 0
    assert t.finalize() == 0
    ex, S = t.export(), t.stats()["fast_start_levels"]
    assert t.counts()["unsorted_cached_nodes"] == 0
    t.close()
    assert S >= 2, "the start nodes must lie at a level where n = 1"
    files = {}
    for j in range(len(ex["level"])):
        if int(ex["level"][j]) >= 1:
            files[(int(ex["level"][j]), int(ex["key"][j]))] = list(ex["ids"][int(ex["offset"][j]):int(ex["offset"][j] + ex["count"][j])])
    expect = R.files_table(R.reconstruct_files(files, ex["xyz"], *UNIT, 400, sp, 1))
    info, table, ids = _gpu_tiler_files(ctx, parts, _params(400, sp, strategy=O.FAST, fast_concurrency=4))
    assert info["fast_start_levels"] == S and info["rekey_inversions"] == 0
    _compare_tables(table, ids, expect)
    md_root = ex["count"][0]
    assert int(ex["level"][0]) == -1 and int(expect["level"][0]) == -1 and expect["count"][0] != md_root


# ------------------------------------------------------------------------------------------- what it refuses
def test_property_flag_is_refused(ctx):
    import schwarzwald_amd as swz
    xyz = np.random.default_rng(52).random((2000, 3))
    with pytest.raises(swz.SwzError) as e:
        ctx.tile(xyz, *UNIT, _params(100, 0.1, flags=swz.FLAG_MIN_DISTANCE_PROPERTY))
    assert e.value.code == swz.api.ERR_BAD_ARG and "MIN_DISTANCE_FAST" in str(e.value)
    with pytest.raises(swz.SwzError) as e:
        swz.Tiler(ctx, UNIT[0], UNIT[1], _params(100, 0.1, flags=swz.FLAG_MIN_DISTANCE_PROPERTY))
    assert e.value.code == swz.api.ERR_BAD_ARG


def test_sharded_entry_point_is_refused(ctx):
    import torch
    import schwarzwald_amd as swz
    d = torch.from_numpy(np.random.default_rng(53).random((2000, 3))).cuda()
    torch.cuda.synchronize()
    with pytest.raises(swz.SwzError) as e:
        ctx.shard_begin_device(d.data_ptr(), 2000, *UNIT, _params(100, 0.1), 2000)
    assert e.value.code == swz.api.ERR_BAD_ARG
    assert "shard" in str(e.value) and len(str(e.value)) > len("swz error 2: ")
