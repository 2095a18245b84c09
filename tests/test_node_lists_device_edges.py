"""swz_build_node_lists_device (level_key_kernel, the stable partition by level, node_head_kernel, the scan, node_table_kernel;
swz_payload.hip) on synthesised inputs: node heads at workgroup, scan-tile and partition-tile seams, levels -1 and 20, equal keys
at different levels, neighbours that differ just below or just inside the node prefix, max_nodes met and one short, the
count-only call and levels out of range.  The reference is a stable group by level, then by key >> shift, in numpy; the host
entry swz_build_node_lists must give the same on every case."""
import ctypes as C

import numpy as np
import pytest

import edge_inputs as E

CASES = E.node_list_cases()
ERR_BAD_ARG = 2


# ------------------------------------------------------------------------------------------------------------ CPU: the premises
def test_cases_are_what_they_claim():
    names = list(CASES)
    assert len([n for n in names if n.startswith("heads at seams")]) >= 8
    for name, (keys, level) in CASES.items():
        assert keys.dtype == np.uint64 and level.dtype == np.int8 and len(keys) == len(level) > 0, name
        assert np.all(keys[1:] >= keys[:-1]) and int(keys[-1]) < 1 << 63, name
        assert level.min() >= -1 and level.max() <= 20, name
    order, nodes = E.node_lists_reference(*CASES["all level -1"])
    assert nodes["key"].tolist() == [0] and nodes["count"].tolist() == [1000] and np.array_equal(order, np.arange(1000))
    _, nodes = E.node_lists_reference(*CASES["all level 20"])
    assert len(nodes["key"]) == len(np.unique(CASES["all level 20"][0])) == 991
    _, nodes = E.node_lists_reference(*CASES["equal keys at different levels"])
    assert nodes["level"].tolist() == [-1, 0, 1, 3, 20] and nodes["count"].tolist() == [1, 1, 2, 3, 2]
    _, nodes = E.node_lists_reference(*CASES["neighbours at the node's shift"])
    assert nodes["count"].tolist() == [3, 2, 1]
    keys, level = CASES["levels -1 and 20 together"]
    assert level.min() == -1 and level.max() == 20
    keys, level = CASES["every point its own node"]
    assert len(E.node_lists_reference(keys, level)[1]["key"]) == len(keys)
    tiles = set()
    for name in names:
        if name.startswith("heads at seams"):
            _, nodes = E.node_lists_reference(*CASES[name])
            n = len(CASES[name][0])
            heads = set(nodes["offset"].tolist())
            assert {h for h in range(0, n, 256)} <= heads and n - 1 in heads, name
            tiles.add(n)
    # the tile sizes come from the sources: today's are the 2048 of the scan and the 4096 of the partition and the one-block scan
    assert {2047, 2048, 2049, 4095, 4096, 4097} <= tiles


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def _device(keys, level):
    import torch
    d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    d_level = torch.from_numpy(level).cuda()
    d_order = torch.full((len(keys) + 16,), -1, dtype=torch.int32, device="cuda:0")      # 16 guard entries behind n
    torch.cuda.synchronize()            # (the context runs on a stream of its own: uploads and fill must have landed)
    return d_keys, d_level, d_order


def _check(got_order, got, order, nodes, what):
    assert np.array_equal(got_order, order), what
    for col in ("level", "key", "offset", "count"):
        assert np.array_equal(got[col], nodes[col]), (what, col)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_node_lists_match_reference_and_host_entry(ctx, name):
    import torch
    keys, level = CASES[name]
    n = len(keys)
    order, nodes = E.node_lists_reference(keys, level)
    d_keys, d_level, d_order = _device(keys, level)
    got = ctx.build_node_lists_device(d_keys.data_ptr(), d_level.data_ptr(), n, d_order.data_ptr())
    torch.cuda.synchronize()
    o = d_order.cpu().numpy()
    _check(o[:n].view(np.uint32), got, order, nodes, name + ", device entry")
    assert np.all(o[n:] == -1), name                                             # nothing behind entry n
    horder, hnodes = ctx.build_node_lists(keys, level)
    _check(horder, hnodes, order, nodes, name + ", host entry")


def _raw(ctx, entry, keys, level, max_nodes, with_tables=True):
    """The C entry itself: (status, num_nodes_out, node table or None)"""
    import schwarzwald_amd as swz
    L = swz.load_library()
    n = len(keys)
    cap = max(int(max_nodes), 1)
    nl, nk = np.full(cap, 99, dtype=np.int8), np.zeros(cap, dtype=np.uint64)
    no, nc = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    num = C.c_uint64(12345)
    i8p, u64p = C.POINTER(C.c_int8), C.POINTER(C.c_uint64)
    tables = [nl.ctypes.data_as(i8p), nk.ctypes.data_as(u64p), no.ctypes.data_as(u64p), nc.ctypes.data_as(u64p)] if with_tables else [None] * 4
    if entry == "device":
        d_keys, d_level, d_order = _device(keys, level)
        st = L.swz_build_node_lists_device(ctx._ctx, C.c_void_p(d_keys.data_ptr()), C.c_void_p(d_level.data_ptr()), n,
                                           C.c_void_p(d_order.data_ptr()), int(max_nodes), *tables, C.byref(num))
    else:
        order = np.empty(n, dtype=np.uint32)
        st = L.swz_build_node_lists(ctx._ctx, keys.ctypes.data_as(u64p), level.ctypes.data_as(i8p), n,
                                    order.ctypes.data_as(C.POINTER(C.c_uint32)), int(max_nodes), *tables, C.byref(num))
    return st, int(num.value), dict(level=nl, key=nk, offset=no, count=nc)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["device", "host"])
def test_max_nodes_met_one_short_and_the_count_only_call(ctx, entry):
    for name in ("levels -1 and 20 together", "equal keys at different levels", "every point its own node"):
        keys, level = CASES[name]
        _, nodes = E.node_lists_reference(keys, level)
        nn = len(nodes["key"])
        st, num, got = _raw(ctx, entry, keys, level, nn)                          # exactly met
        assert (st, num) == (0, nn), name
        for col in nodes:
            assert np.array_equal(got[col][:nn], nodes[col]), (name, col)
        st, num, _ = _raw(ctx, entry, keys, level, nn - 1)                        # one short: an error, and the number needed
        assert (st, num) == (ERR_BAD_ARG, nn), name
        st, num, _ = _raw(ctx, entry, keys, level, len(keys), with_tables=False)  # count only
        assert (st, num) == (0, nn), name


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("bad", [21, -2, 127, -128])
def test_levels_out_of_range_are_refused(ctx, entry, bad):
    import schwarzwald_amd as swz
    keys, level = CASES["levels -1 and 20 together"]
    level = level.copy()
    level[len(level) // 2] = bad
    st, _, _ = _raw(ctx, entry, keys, level, len(keys))
    assert st == ERR_BAD_ARG
    assert "level out of range" in swz.load_library().swz_last_error(ctx._ctx).decode()
