"""swz_pnts_pack_origin_device: .pnts bodies relative to an origin per node.  The yardstick is the existing instantiation of
the same kernel: the image must be, byte for byte, what pnts_pack_device writes for positions from which numpy has
subtracted every node's origin in float64 -- the subtraction in double, then the plain narrowing."""
import numpy as np
import pytest

from world_util import nodes as _nodes, tables as _tables

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
PACK_TILE = 256
MASKS = [((), 0), (("rgb",), 0), (("rgb", "intensity"), 0), (("rgb", "intensity"), 2)]   # (attrs, rgb_from); 2: RGB_FROM_INTENSITY_LOG


@pytest.fixture(scope="module")
def ctx():
    import torch
    import schwarzwald_amd as swz
    with swz.Context(0) as c:
        c.set_stream(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
        yield c


def _cloud(n, seed):
    """ECEF-sized coordinates with millimetre fractions, negative ones too; the stored order is a permutation of the rows"""
    rng = np.random.default_rng(seed)
    xyz = np.array([4161242.0, -659126.0, 4772564.0]) + np.round(rng.random((n, 3)) * 900.0, 3)
    cols = dict(rgb=rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
                intensity=rng.integers(0, 65535, n, endpoint=True).astype(np.uint16))
    return xyz, cols, rng.permutation(n).astype(np.uint32)


def _pack(ctx, xyz, cols, perm, table, attrs, rgb_from, origin=None, fill=0xEE):
    import torch
    import schwarzwald_amd as swz
    dev = torch.device("cuda:0")
    n = len(xyz)
    nodes = _nodes(table)
    total = swz.pnts_layout(nodes["count"], attrs, rgb_from)["total"]
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz)).to(dev)
    d_cols = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    d_perm = torch.from_numpy(perm.view(np.int32)).to(dev)
    image = torch.full((total + 16,), fill, dtype=torch.uint8, device=dev)
    args = (d_perm.data_ptr(), None, n, d_xyz.data_ptr(), {k: v.data_ptr() for k, v in d_cols.items()}, nodes, image.data_ptr(), total)
    if origin is None:
        ctx.pnts_pack_device(*args, attrs=attrs, rgb_from=rgb_from)
    else:
        ctx.pnts_pack_origin_device(*args, origin, attrs=attrs, rgb_from=rgb_from)
    torch.cuda.synchronize()
    out = image.cpu().numpy()
    assert (out[total:] == fill).all()
    return out[:total]


def _shifted(xyz, perm, table, origin):
    """the source rows minus the origin of the node whose stored rows name them, in float64"""
    out = xyz.copy()
    for k, (o, c) in enumerate(table):
        src = perm[o:o + c]
        out[src] = xyz[src] - origin[k]
    return out


def _minima(xyz, perm, table):
    origin = np.full((len(table), 3), np.inf)            # an empty node: not finite, and accepted
    for k, (o, c) in enumerate(table):
        if c:
            origin[k] = xyz[perm[o:o + c]].min(axis=0)
    return origin


@pytest.mark.parametrize("attrs,rgb_from", MASKS)
def test_image_is_the_pack_of_shifted_positions(ctx, attrs, rgb_from):
    for seed, (name, (n, table)) in enumerate(_tables(PACK_TILE).items()):
        xyz, cols, perm = _cloud(n, seed)
        origin = _minima(xyz, perm, table)
        got = _pack(ctx, xyz, cols, perm, table, attrs, rgb_from, origin=origin)
        want = _pack(ctx, _shifted(xyz, perm, table, origin), cols, perm, table, attrs, rgb_from, fill=0x11)
        assert np.array_equal(got, want), name
        if name == "mixed":
            plain = _pack(ctx, xyz, cols, perm, table, attrs, rgb_from)
            assert len(got) > 12 * 3 * PACK_TILE and not np.array_equal(got, plain)      # the origin shows


def test_an_arbitrary_origin_with_negative_zero_and_negative_components(ctx):
    n, table = _tables(PACK_TILE)["mixed"]
    xyz, cols, perm = _cloud(n, 77)
    origin = np.tile([-0.0, -659126.375, 4772000.0009765625], (len(table), 1))
    origin[2] = [1e-3, -0.0, -7.5e6]
    got = _pack(ctx, xyz, cols, perm, table, ("rgb", "intensity"), 0, origin=origin)
    want = _pack(ctx, _shifted(xyz, perm, table, origin), cols, perm, table, ("rgb", "intensity"), 0, fill=0x11)
    assert np.array_equal(got, want)


def test_an_origin_that_is_not_finite(ctx):
    import schwarzwald_amd as swz
    table = [(0, 10), (10, 0), (12, 20)]
    xyz, cols, perm = _cloud(40, 5)
    origin = _minima(xyz, perm, table)
    assert not np.isfinite(origin[1]).any()
    _pack(ctx, xyz, cols, perm, table, ("rgb",), 0, origin=origin)                    # on an empty node: accepted
    for bad in (np.nan, np.inf):
        broken = origin.copy()
        broken[2, 1] = bad
        with pytest.raises(swz.SwzError) as e:
            _pack(ctx, xyz, cols, perm, table, ("rgb",), 0, origin=broken)
        assert e.value.code == ERR_BAD_ARG and "origin" in str(e.value), str(e.value)
