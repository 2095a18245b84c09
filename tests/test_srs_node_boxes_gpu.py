"""swz_srs_project_node_boxes_device: a chunk of stored rows mapped to ECEF in place and the box of every node's mapped
rows, in one launch.  The yardsticks are existing code and numpy: the array afterwards has the bits srs_transform_device gives
a copy of it (the header's promise: the map gives the same bits in every kernel it is inlined into), the boxes are numpy's
min / max per node of that copy, compared with ==, and without a projection they are node_boxes_device's."""
import numpy as np
import pytest

import srs_ref as R
from world_util import nodes as _nodes, tables as _tables

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
GUARD = -7.25
DEFINITIONS = [R.utm_definition(32, False), R.utm_definition(19, True)]


def _rows(definition, n):
    """The points of srs_ref.py, replicated.  It has no group for zone 19: eastings and northings of a southern zone are
    those of any other, so the 19 south rows are the coordinates of its 32 south group, read in zone 19 -- the yardstick
    here is srs_transform_device, not the group's reference values."""
    source = R.utm_definition(32, True) if definition == DEFINITIONS[1] else definition
    g = next(x for x in R.points() if x["definition"] == source)
    return g["xyz"][np.arange(n) % len(g["xyz"])]


def _guarded(rows, front=3, back=5):
    import torch
    buf = torch.full((front + len(rows) + back, 3), GUARD, dtype=torch.float64, device="cuda:0")
    buf[front:front + len(rows)] = torch.from_numpy(np.ascontiguousarray(rows)).to("cuda:0")
    return buf, front


def _inside(buf, front, n):
    import torch
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:front] == GUARD).all() and (out[front + n:] == GUARD).all()      # the guard rows are untouched
    return out[front:front + n]


def _numpy_boxes(rows, table):
    lo = np.full((len(table), 3), np.inf)
    hi = np.full((len(table), 3), -np.inf)
    for k, (o, c) in enumerate(table):
        if c:
            lo[k], hi[k] = rows[o:o + c].min(axis=0), rows[o:o + c].max(axis=0)
    return lo, hi


@pytest.fixture(scope="module")
def ctx():
    import torch
    import schwarzwald_amd as swz
    with swz.Context(0) as c:
        c.set_stream(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
        yield c


@pytest.mark.parametrize("definition", DEFINITIONS)
def test_projected_rows_and_boxes(ctx, definition):
    import schwarzwald_amd as swz
    T = swz.srs_tile()
    srs = swz.Srs(definition)
    for name, (n, table) in _tables(T).items():
        rows = _rows(definition, n)
        ref_buf, front = _guarded(rows)
        ctx.srs_transform_device(srs, ref_buf.data_ptr() + 24 * front, n)
        want = _inside(ref_buf, front, n)
        buf, front = _guarded(rows)
        lo, hi = ctx.srs_project_node_boxes_device(srs, buf.data_ptr() + 24 * front, n, _nodes(table))
        got = _inside(buf, front, n)
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), name         # identical bits, gap rows included
        assert 6.3e6 < np.linalg.norm(want, axis=1).min()
        if definition == DEFINITIONS[1]:
            assert (want[:, 1] < 0).all() and (want[:, 2] <= 0).all()                  # zone 19 south: ECEF Y and Z negative
        want_lo, want_hi = _numpy_boxes(want, table)
        assert (lo == want_lo).all() and (hi == want_hi).all(), name                # count 0: (+inf, -inf)
        if name == "mixed":
            assert np.isinf(lo).all(axis=1).sum() == 5 and (lo[5:305] == hi[5:305]).all()


def test_without_a_projection_only_the_boxes(ctx):
    import torch
    import schwarzwald_amd as swz
    T = swz.srs_tile()
    for name, (n, table) in _tables(T).items():
        rows = _rows(DEFINITIONS[0], n)
        rows[::7, 1] = -0.0
        buf, front = _guarded(rows)
        lo, hi = ctx.srs_project_node_boxes_device(None, buf.data_ptr() + 24 * front, n, _nodes(table))
        got = _inside(buf, front, n)
        assert np.array_equal(got.view(np.int64), rows.view(np.int64)), name        # unchanged
        ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
        want_lo, want_hi = ctx.node_boxes_device(ids.data_ptr(), None, n, buf.data_ptr() + 24 * front, _nodes(table))
        assert (lo == want_lo).all() and (hi == want_hi).all(), name


def test_nothing_to_do_launches_nothing(ctx):
    lo, hi = ctx.srs_project_node_boxes_device(DEFINITIONS[0], 0, 0, _nodes([(0, 0), (0, 0)]))
    assert (lo == np.inf).all() and (hi == -np.inf).all() and lo.shape == (2, 3)
    lo, hi = ctx.srs_project_node_boxes_device(None, 0, 10, _nodes([]))             # no nodes, no projection: d_xyz is not looked at
    assert lo.shape == (0, 3)


def test_refusals(ctx):
    import schwarzwald_amd as swz
    rows = _rows(DEFINITIONS[0], 40)
    buf, front = _guarded(rows)
    p = buf.data_ptr() + 24 * front
    for table, word in (([(0, 10), (5, 10)], "overlap"), ([(0, 10), (35, 6)], "passes the last row"), ([(10, 5), (0, 5)], "ascending")):
        with pytest.raises(swz.SwzError) as e:
            ctx.srs_project_node_boxes_device(DEFINITIONS[0], p, 40, _nodes(table))
        assert e.value.code == ERR_BAD_ARG and word in str(e.value), str(e.value)
    with pytest.raises(swz.SwzError) as e:
        ctx.srs_project_node_boxes_device(DEFINITIONS[0], p, 2 ** 32 - 65535, _nodes([(0, 10)]))
    assert "2^32-65536" in str(e.value)
    with pytest.raises(swz.SwzError) as e:
        ctx.srs_project_node_boxes_device(DEFINITIONS[0], 0, 40, _nodes([(0, 10)]))
    assert e.value.code == ERR_BAD_ARG
    assert np.array_equal(_inside(buf, front, 40).view(np.int64), rows.view(np.int64))   # a refusal launched nothing
