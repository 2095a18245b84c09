"""swz_merge_shard_node_tables (host only) through merge_shard_node_tables: a (level, key)-ordered node table is split by the
shard that owns a node's level-0 octant, the root into parts, and merged back."""
import numpy as np
import pytest

import schwarzwald_amd as swz


def _table(seed=5, nodes=400, octants=range(8)):
    """a node table as swz_tiler_node_table orders it: the root, then level after level by ascending node key"""
    rng = np.random.default_rng(seed)
    rows = {(-1, 0)}
    octants = list(octants)
    while len(rows) < nodes:
        level = int(rng.integers(0, 7))
        digits = [int(rng.choice(octants))] + [int(x) for x in rng.integers(0, 8, level)]
        key = 0
        for l, dgt in enumerate(digits):
            key |= dgt << (3 * (20 - l))
        rows.add((level, key))
    rows = sorted(rows)
    level = np.array([r[0] for r in rows], np.int8)
    key = np.array([r[1] for r in rows], np.uint64)
    count = rng.integers(1, 5000, len(rows)).astype(np.uint64)
    return level, key, count


def _split(level, key, count, shards, root_holders):
    """per shard (level, key, count); the root's count is spread over root_holders"""
    owner = (key >> np.uint64(60)).astype(np.int64) * shards // 8
    parts = np.zeros(shards, np.uint64)
    root = int(count[0])
    for i, s in enumerate(root_holders):
        parts[s] = root // len(root_holders) + (root % len(root_holders) if i == 0 else 0)
    out = []
    for s in range(shards):
        sel = (owner == s) & (level >= 0)
        lv, ky, ct = level[sel], key[sel], count[sel]
        if parts[s]:
            lv, ky, ct = np.r_[np.int8(-1), lv].astype(np.int8), np.r_[np.uint64(0), ky].astype(np.uint64), np.r_[parts[s], ct].astype(np.uint64)
        out.append((lv, ky, ct))
    return out, owner


@pytest.mark.parametrize("shards", [1, 2, 4, 8])
def test_split_tables_merge_back_to_the_original(shards):
    level, key, count = _table()
    holders = list(range(shards))[::2] if shards > 1 else [0]  # a root held by only some shards
    tables, owner = _split(level, key, count, shards, holders)
    lv, ky, ct, sh = swz.merge_shard_node_tables(tables)
    assert np.array_equal(lv, level) and np.array_equal(ky, key) and np.array_equal(ct, count)
    assert sh[0] == -1 and np.array_equal(sh[1:], owner[1:])
    assert swz.merge_shard_node_tables(tables, count_only=True) == len(level)
    # a larger capacity changes nothing
    lv2, ky2, ct2, sh2 = swz.merge_shard_node_tables(tables, max_nodes=len(level) + 7)
    assert np.array_equal(lv2, level) and np.array_equal(ky2, key) and np.array_equal(ct2, count) and np.array_equal(sh2, sh)


def test_shards_with_empty_tables_and_no_root():
    level, key, count = _table(seed=6, nodes=120, octants=[0, 5])  # at 8 shards six tables are empty
    tables, owner = _split(level, key, count, 8, [5])
    assert sum(len(t[0]) == 0 for t in tables) == 6
    lv, ky, ct, sh = swz.merge_shard_node_tables(tables)
    assert np.array_equal(lv, level) and np.array_equal(ky, key) and np.array_equal(ct, count)
    assert sh[0] == -1 and np.array_equal(sh[1:], owner[1:])
    # no root anywhere: the merged table has none either
    no_root = [(t[0][t[0] >= 0], t[1][t[0] >= 0], t[2][t[0] >= 0]) for t in tables]
    lv, ky, ct, sh = swz.merge_shard_node_tables(no_root)
    assert np.array_equal(lv, level[1:]) and np.array_equal(ky, key[1:]) and np.array_equal(ct, count[1:]) and (sh >= 0).all()
    # nothing at all
    empty = (np.zeros(0, np.int8), np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    assert swz.merge_shard_node_tables([empty] * 4, count_only=True) == 0
    assert len(swz.merge_shard_node_tables([empty] * 4)[0]) == 0


def test_a_node_below_the_root_on_two_shards_is_an_error():
    level, key, count = _table(seed=7, nodes=60)
    tables, _ = _split(level, key, count, 4, [0, 1, 2, 3])
    lv, ky, ct = tables[2]
    stray = (np.r_[tables[1][0], lv[-1:]].astype(np.int8), np.r_[tables[1][1], ky[-1:]].astype(np.uint64), np.r_[tables[1][2], ct[-1:]].astype(np.uint64))
    with pytest.raises(RuntimeError):
        swz.merge_shard_node_tables([tables[0], stray, tables[2], tables[3]])
    with pytest.raises(RuntimeError):
        swz.merge_shard_node_tables([tables[0], stray, tables[2], tables[3]], count_only=True)


def test_max_nodes_too_small_is_bad_arg():
    level, key, count = _table(seed=8, nodes=60)
    tables, _ = _split(level, key, count, 2, [0, 1])
    with pytest.raises(ValueError):
        swz.merge_shard_node_tables(tables, max_nodes=len(level) - 1)
    assert swz.merge_shard_node_tables(tables, count_only=True) == len(level)  # NULL outputs: the count only, any capacity
