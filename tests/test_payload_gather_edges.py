"""swz_gather_payload_device (compose_kernel and gather_rows_kernel<T, K>, swz_payload.hip) on its own: row i of every output
column is row perm[order[i]] (perm[i] without an order) of the input column -- for identity, reversed, random and repeating
indices, with and without an order, every attribute (row widths 1, 2, 3, 8 and 12 bytes) and the positions, columns given on
one side only, 64 guard rows behind row n, and sources whose bytes are NaNs with payloads, -0.0, denormals and 0xFF.  The
reference is numpy's take; everything is compared as raw bytes.  No index is ever out of range."""
import ctypes

import numpy as np
import pytest

import edge_inputs as E
import oracle_lib as O

pytestmark = pytest.mark.gpu

ATTRS = O.ATTRIBUTES                      # name -> (index, dtype, row width)
NAMES = list(ATTRS)
KINDS = ("identity", "reversed", "permutation", "repeats")


@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def test_every_row_width_is_covered(ctx):
    import schwarzwald_amd as swz
    L = swz.load_library()
    L.swz_attribute_row_bytes.restype = ctypes.c_uint32
    widths = {name: int(L.swz_attribute_row_bytes(idx)) for name, (idx, dt, w) in ATTRS.items()}
    assert widths == {name: np.dtype(dt).itemsize * w for name, (idx, dt, w) in ATTRS.items()}
    assert sorted(set(widths.values())) == [1, 2, 3, 8, 12] and len(widths) == 12
    assert int(L.swz_attribute_row_bytes(12)) == 0                               # SWZ_ATTR_COUNT: no attribute behind the twelfth


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _out(n, row_bytes):
    import torch
    return torch.full(((n + E.GUARD_ROWS) * row_bytes,), E.SENTINEL, dtype=torch.uint8, device="cuda:0")


def _run(ctx, n, perm, order, xyz, both, in_only, out_only, src):
    """One call: positions when xyz is given, attributes `both` on both sides, `in_only` / `out_only` on one.  Checks every
    output against numpy's take, the guard rows and the columns that must stay untouched."""
    import torch
    what = "n = %d, %s positions, both %s, input only %s, output only %s" % (n, "with" if xyz is not None else "no", both, in_only, out_only)
    d_perm, d_order = _up(perm), (None if order is None else _up(order))
    take = perm if order is None else perm[order]
    d_in = {name: _up(src[name]) for name in both + in_only}
    d_out = {name: _out(n, src[name][0].nbytes) for name in both + out_only}
    d_xyz = None if xyz is None else _up(xyz)
    d_xyz_out = None if xyz is None else _out(n, 24)
    torch.cuda.synchronize()            # (the context runs on a stream of its own: uploads and fills must have landed)
    ctx.gather_payload_device(d_perm.data_ptr(), None if d_order is None else d_order.data_ptr(), n,
                              None if d_xyz is None else d_xyz.data_ptr(), {k: v.data_ptr() for k, v in d_in.items()},
                              None if d_xyz_out is None else d_xyz_out.data_ptr(), {k: v.data_ptr() for k, v in d_out.items()})
    torch.cuda.synchronize()

    def check(got, source, name):
        got = got.cpu().numpy()
        row = source[0].nbytes
        want = np.take(source.view(np.uint8).reshape(n, row), take, axis=0)
        assert np.array_equal(got[:n * row].reshape(n, row), want), (what, name)
        assert np.all(got[n * row:] == E.SENTINEL), (what, name, "guard rows")

    if xyz is not None:
        check(d_xyz_out, xyz, "positions")
    for name in both:
        check(d_out[name], src[name], name)
    for name in out_only:
        assert bool((d_out[name] == E.SENTINEL).all()), (what, name, "a column without an input was written")


@pytest.mark.parametrize("with_order", [False, True], ids=["no order", "order"])
@pytest.mark.parametrize("n", E.GATHER_SIZES)
def test_gather_matches_take(ctx, n, with_order):
    rng = np.random.default_rng(1000 + n)
    src = {name: E.gather_source(dt, w, n, rng) for name, (idx, dt, w) in ATTRS.items()}
    xyz = E.gather_source(np.float64, 3, n, rng)
    for j, kind in enumerate(KINDS):
        perm = E.gather_indices(kind, n, rng)
        order = E.gather_indices(KINDS[(j + 1 + (n % 3)) % 4], n, rng) if with_order else None
        _run(ctx, n, perm, order, xyz, NAMES, [], [], src)                        # positions and every attribute
        # every attribute in turn on both sides, on the input only and on the output only; positions alone; attributes alone
        r = (j * 3) % 12
        rot = NAMES[r:] + NAMES[:r]
        _run(ctx, n, perm, order, None, rot[0:4], rot[4:8], rot[8:12], src)
        _run(ctx, n, perm, order, None, rot[4:8], rot[8:12], rot[0:4], src)
        _run(ctx, n, perm, order, xyz, rot[8:12], rot[0:4], rot[4:8], src)
        _run(ctx, n, perm, order, xyz, [], NAMES[j::4], NAMES[(j + 1) % 4::4], src)  # positions alone: no attribute on both sides


def test_order_and_perm_compose_in_that_order(ctx):
    """out[i] = in[perm[order[i]]], not in[order[perm[i]]]: two permutations that do not commute"""
    perm = np.array([1, 2, 0, 3], dtype=np.uint32)
    order = np.array([0, 1, 3, 2], dtype=np.uint32)
    assert not np.array_equal(perm[order], order[perm])
    src = {"intensity": np.array([[10], [20], [30], [40]], dtype=np.uint16)}
    _run(ctx, 4, perm, order, None, ["intensity"], [], [], src)


def test_positions_need_both_sides(ctx):
    import torch
    import schwarzwald_amd as swz
    n = 300
    perm = _up(np.arange(n, dtype=np.uint32))
    xyz = _up(np.zeros((n, 3)))
    out = _out(n, 24)
    torch.cuda.synchronize()
    for d_in, d_out in ((xyz.data_ptr(), None), (None, out.data_ptr())):
        with pytest.raises(swz.SwzError) as e:
            ctx.gather_payload_device(perm.data_ptr(), None, n, d_in, {}, d_out, {})
        assert e.value.code == swz.api.ERR_BAD_ARG and "positions" in str(e.value)
    with pytest.raises(swz.SwzError) as e:
        ctx.gather_payload_device(None, None, n, xyz.data_ptr(), {}, out.data_ptr(), {})
    assert e.value.code == swz.api.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == E.SENTINEL).all())                                       # nothing was launched
