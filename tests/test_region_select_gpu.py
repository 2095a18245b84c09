"""swz_region_select_device alone: the stable compaction of the rows of a closed box cut by planes or by a polygon in x-y.

The reference is tests/region_ref.py, the formulas of include/swz_gpu.h in numpy, applied to the host copies: xyz[mask],
col[mask] and np.flatnonzero(mask), compared for byte equality.  Every output is pre-filled with a poison byte and carries
guard bands on both sides: nothing but the rows [0, count) may change."""
import numpy as np
import pytest

import region_ref as R

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
POISON = 0xA5
GUARD = 64
BOX = ([0.25, 0.25, 0.25], [0.75, 0.75, 0.75])
UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ALL = ("rgb", "normal", "intensity", "classification", "edge_of_flight_line", "gps_time", "number_of_returns", "return_number",
       "point_source_id", "scan_direction_flag", "scan_angle_rank", "user_data")
ONE_OF_EACH_WIDTH = ("classification", "intensity", "rgb", "gps_time", "normal")  # u8, u16, 3 x u8, f64, 3 x f32
# the two regions of the size / pattern cases, with where their selected and their refused rows lie -- the refused ones INSIDE
# the box, so that it is the kind's test that refuses them
KINDS = {"planes": (("planes", [[1.0, 0.0, 0.0, -0.4]]), ([0.45, 0.3, 0.3], [0.7, 0.7, 0.7]), ([0.3, 0.3, 0.3], [0.35, 0.7, 0.7])),
         "polygon": (("polygon", R.L_SHAPE), ([0.3, 0.3, 0.3], [0.45, 0.45, 0.7]), ([0.55, 0.55, 0.3], [0.7, 0.7, 0.7]))}


@pytest.fixture(scope="module")
def G():
    import torch
    import schwarzwald_amd as swz
    with swz.Context(0) as ctx:
        yield dict(ctx=ctx, T=swz.box_select_tile(), dev=torch.device("cuda", 0))


def _columns(n, names, seed=5):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(seed)
    out = {}
    for name in names:
        _, dt, width = swz.ATTRIBUTES[name]
        raw = rng.integers(0, 256, n * width * np.dtype(dt).itemsize, dtype=np.uint8)
        out[name] = raw.view(dt).reshape((n, width) if width > 1 else (n,))
    return out


def _positions(n, inside, kind, seed=7):
    _, (ilo, ihi), (olo, ohi) = KINDS[kind]
    rng = np.random.default_rng(seed)
    xyz = np.asarray(olo) + (np.asarray(ohi) - np.asarray(olo)) * rng.random((n, 3))
    k = int(np.count_nonzero(inside))
    xyz[inside] = np.asarray(ilo) + (np.asarray(ihi) - np.asarray(ilo)) * rng.random((k, 3))
    return xyz


class Outputs:
    """poisoned device buffers with guard bands: positions, columns, rows"""

    def __init__(self, G, capacity, names):
        import torch
        import schwarzwald_amd as swz
        self.widths = {"xyz": 24, "row": 4}
        self.widths.update({k: swz.ATTRIBUTES[k][2] * np.dtype(swz.ATTRIBUTES[k][1]).itemsize for k in names})
        self.buf = {k: torch.full(((capacity + 2 * GUARD) * w,), POISON, dtype=torch.uint8, device=G["dev"]) for k, w in self.widths.items()}

    def ptr(self, k):
        return self.buf[k].data_ptr() + GUARD * self.widths[k]

    def host(self, k):
        return self.buf[k].cpu().numpy()

    def rows_of(self, k, count, dtype, width):
        w = self.widths[k]
        raw = self.host(k)[GUARD * w:(GUARD + count) * w].copy()
        return raw.view(dtype).reshape((count, width) if width > 1 else (count,))

    def assert_poison_beyond(self, count):
        for k, w in self.widths.items():
            h = self.host(k)
            assert (h[:GUARD * w] == POISON).all(), k
            assert (h[(GUARD + count) * w:] == POISON).all(), k


def _upload(G, xyz, cols):
    import torch
    pad = np.zeros(8, np.uint8)  # (an empty tensor has no address)
    d_xyz = torch.from_numpy(np.concatenate([np.ascontiguousarray(xyz).view(np.uint8).reshape(-1), pad])).to(G["dev"])
    d_cols = {k: torch.from_numpy(np.concatenate([np.ascontiguousarray(v).view(np.uint8).reshape(-1), pad])).to(G["dev"]) for k, v in cols.items()}
    return d_xyz, d_cols


def _run(G, xyz, cols, box, region, capacity=None, call="region"):
    import torch
    import schwarzwald_amd as swz
    n = len(xyz)
    d_xyz, d_cols = _upload(G, xyz, cols)
    cap = n if capacity is None else capacity
    out = Outputs(G, cap, tuple(cols))
    ins, outs = {k: v.data_ptr() for k, v in d_cols.items()}, {k: out.ptr(k) for k in cols}
    if call == "box":
        count = G["ctx"].box_select_device(d_xyz.data_ptr(), n, box[0], box[1], cap, out.ptr("xyz"), ins, outs, d_row_out=out.ptr("row"))
    else:
        rg = region if isinstance(region, swz.Region) else R.as_region(swz, region)
        count = G["ctx"].region_select_device(d_xyz.data_ptr(), n, box[0], box[1], rg, cap, out.ptr("xyz"), ins, outs, d_row_out=out.ptr("row"))
    torch.cuda.synchronize()
    return count, out


def _check(G, xyz, cols, box, region):
    import schwarzwald_amd as swz
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    mask = R.region_mask(xyz, box, region)
    count, out = _run(G, xyz, cols, box, region)
    assert count == int(mask.sum())
    assert out.rows_of("xyz", count, np.float64, 3).tobytes() == xyz[mask].tobytes()
    for k, v in cols.items():
        _, dt, width = swz.ATTRIBUTES[k]
        assert out.rows_of(k, count, dt, width).tobytes() == v[mask].tobytes(), k
    assert np.array_equal(out.rows_of("row", count, np.uint32, 1), np.flatnonzero(mask).astype(np.uint32))
    out.assert_poison_beyond(count)
    return mask


def _sizes(T):
    return [0, 1, T - 1, T, T + 1, 5 * T + 3]


def _patterns(n, T):
    idx = np.arange(n)
    pats = {"all_in": np.ones(n, bool), "all_out": np.zeros(n, bool), "every_other": idx % 2 == 0}
    if n:
        pats["one_in_the_last_tile"] = idx == n - 1
    return pats


@pytest.mark.parametrize("columns", [(), ONE_OF_EACH_WIDTH, ALL], ids=["none", "widths", "all"])
@pytest.mark.parametrize("size", range(6))
@pytest.mark.parametrize("kind", ["planes", "polygon"])
def test_sizes_and_patterns(G, kind, size, columns):
    n = _sizes(G["T"])[size]
    cols = _columns(n, columns)
    for name, inside in _patterns(n, G["T"]).items():
        mask = _check(G, _positions(n, inside, kind), cols, BOX, KINDS[kind][0])
        assert np.array_equal(mask, inside), name    # the rows meant to be refused are refused by the kind's test, inside the box


def _cloud(n, seed):
    return np.random.default_rng(seed).random((n, 3))


def _tangent_planes(k, seed, distance=0.3):
    """k planes at `distance` from the centre of the unit cube, normals of any direction"""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(k, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return np.concatenate([nrm, (distance - nrm @ np.full(3, 0.5))[:, None]], axis=1)


@pytest.mark.parametrize("k", [1, 6, 16])
def test_planes_of_any_direction(G, k):
    xyz = _cloud(3 * G["T"] + 17, 20 + k)
    mask = _check(G, xyz, _columns(len(xyz), ("intensity",)), UNIT, ("planes", _tangent_planes(k, k)))
    assert 0 < mask.sum() < len(xyz)


def test_frustum(G):
    import schwarzwald_amd as swz
    planes = swz.frustum_planes(R.look_at_view_proj((-0.6, -0.4, 1.2), (0.5, 0.5, 0.3)))
    assert planes.shape == (6, 4) and np.allclose(np.linalg.norm(planes[:, :3], axis=1), 1.0)
    xyz = _cloud(4 * G["T"] + 5, 31)
    mask = _check(G, xyz, _columns(len(xyz), ("rgb",)), UNIT, ("planes", planes))
    assert 0.05 * len(xyz) < mask.sum() < 0.95 * len(xyz)
    # the camera looks at its target and not behind itself
    assert R.region_mask(np.array([[0.5, 0.5, 0.3]]), UNIT, ("planes", planes))[0]
    assert not R.planes_mask(np.array([[-1.7, -1.3, 2.1]]), planes)[0]


def _lattice(z=0.5):
    k = np.arange(65) / 64.0
    x, y = np.meshgrid(k, k, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], axis=1)


def test_dyadic_planes_zero_is_inside(G):
    xyz = _lattice()
    below = xyz[xyz[:, 0] == 0.5].copy()
    below[:, 0] = np.nextafter(0.5, -np.inf)                      # the next double below the plane
    xyz = np.concatenate([xyz, below])
    for planes in ([[1.0, 0.0, 0.0, -0.5]], [[1.0, 1.0, 0.0, -1.0]], [[1.0, 0.0, 0.0, -0.5], [1.0, 1.0, 0.0, -1.0]]):
        mask = _check(G, xyz, {}, UNIT, ("planes", planes))
        on = np.ones(len(xyz), bool)
        for a, b, c, d in planes:
            on &= a * xyz[:, 0] + b * xyz[:, 1] + d == 0.0          # exact on the lattice
        assert on.sum() >= 1 and mask[on].all()                     # an expression that is exactly 0: in
    mask = _check(G, xyz, {}, UNIT, ("planes", [[1.0, 0.0, 0.0, -0.5]]))
    assert mask[xyz[:, 0] == 0.5].all() and not mask[xyz[:, 0] == np.nextafter(0.5, -np.inf)].any()


def test_planes_that_empty_the_box(G):
    xyz = _cloud(2 * G["T"] + 1, 41)
    mask = _check(G, xyz, _columns(len(xyz), ("classification",)), UNIT, ("planes", [[1.0, 0.0, 0.0, -0.6], [-1.0, 0.0, 0.0, 0.4]]))
    assert mask.sum() == 0


SHAPES = {"square": R.SQUARE, "L": R.L_SHAPE, "U": R.U_SHAPE, "bow_tie": R.BOW_TIE, "circle1024": R.circle(1024)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_polygons_on_random_rows_and_both_vertex_orders(G, shape):
    v = SHAPES[shape]
    xyz = _cloud(5 * G["T"] + 3, 51)
    mask = _check(G, xyz, _columns(len(xyz), ("gps_time",)), UNIT, ("polygon", v))
    assert 0.05 * len(xyz) < mask.sum() < 0.6 * len(xyz)
    back = _check(G, xyz, {}, UNIT, ("polygon", v[::-1]))
    assert np.array_equal(mask, back)                               # no row of this cloud lies on an edge
    if shape in ("L", "U"):                                         # the notch is inside the bounding box and outside the outline
        notch = (xyz[:, 0] > 0.51) & (xyz[:, 0] < 0.74) & (xyz[:, 1] > 0.51) & (xyz[:, 1] < 0.74) if shape == "L" else \
            (xyz[:, 0] > 0.38) & (xyz[:, 0] < 0.62) & (xyz[:, 1] > 0.38)
        assert notch.sum() > 10 and not mask[notch].any()
    if shape == "bow_tie":                                          # the wedges left and right of the crossing are in, above and below out
        dx, dy = xyz[:, 0] - 0.5, xyz[:, 1] - 0.5
        inside = (np.abs(dx) < 0.24) & (np.abs(dy) < np.abs(dx) - 0.01)
        outside = (np.abs(dy) < 0.24) & (np.abs(dx) < np.abs(dy) - 0.01)
        assert inside.sum() > 10 and mask[inside].all() and outside.sum() > 10 and not mask[outside].any()


@pytest.mark.parametrize("shape", ["square", "L", "U", "bow_tie"])
def test_lattice_rows_on_edges_vertices_and_level_with_vertices(G, shape):
    """rows and vertices on one k/64 lattice: t is exact, many rows are level with vertices, on edges and on vertices; the
    horizontal and vertical edges of the shapes run through lattice rows.  The formula decides, in both vertex orders."""
    v = SHAPES[shape]
    xyz = _lattice()
    for order in (v, v[::-1]):
        mask = _check(G, xyz, {}, UNIT, ("polygon", order))
        assert 0 < mask.sum() < len(xyz)
    if shape == "square":
        x, y = xyz[:, 0], xyz[:, 1]
        mask = R.region_mask(xyz, UNIT, ("polygon", v))
        assert mask[(x > 0.25) & (x < 0.75) & (y > 0.25) & (y < 0.75)].all()              # strictly inside
        assert not mask[(x < 0.25) | (x > 0.75) | (y < 0.25) | (y > 0.75)].any()          # strictly outside
        assert mask[(y == 0.25) & (x > 0.25) & (x < 0.75)].all()                          # level with the lower vertices: counted once
        assert not mask[(y == 0.75)].any()                                                # the upper horizontal edge never counts
        # on the vertical edges t == 0: such an edge counts iff it runs downwards -- out for this counter-clockwise order,
        # in for the clockwise one
        on_vertical = ((x == 0.25) | (x == 0.75)) & (y >= 0.25) & (y < 0.75)
        assert not mask[on_vertical].any() and R.region_mask(xyz, UNIT, ("polygon", v[::-1]))[on_vertical].all()


def test_the_box_cuts_the_extrusion(G):
    xyz = _cloud(2 * G["T"] + 7, 61)
    box = ([0.0, 0.0, 0.4], [1.0, 1.0, 0.6])
    mask = _check(G, xyz, {}, box, ("polygon", R.L_SHAPE))
    full = R.region_mask(xyz, UNIT, ("polygon", R.L_SHAPE))
    assert 0 < mask.sum() < full.sum() and np.array_equal(mask, full & (xyz[:, 2] >= 0.4) & (xyz[:, 2] <= 0.6))


@pytest.mark.parametrize("region", [("planes", [[1.0, 0.0, 0.0, 0.0]]), ("polygon", R.SQUARE)], ids=["planes", "polygon"])
def test_nan_is_outside(G, region):
    xyz = np.tile([0.5, 0.5, 0.5], (8, 1))
    for a in range(3):
        xyz[1 + 2 * a, a] = np.nan
    mask = _check(G, xyz, _columns(8, ("classification",)), UNIT, region)
    assert mask.tolist() == [True, False, True, False, True, False, True, True]


def test_box_region_and_null_give_the_bytes_of_the_box_call(G):
    import schwarzwald_amd as swz
    xyz = _cloud(3 * G["T"] + 5, 71)
    cols = _columns(len(xyz), ALL)
    want_count, want = _run(G, xyz, cols, BOX, None, call="box")
    assert 0 < want_count < len(xyz)
    for region in (None, swz.Region.box()):
        count, got = _run(G, xyz, cols, BOX, region)
        assert count == want_count
        for k in want.buf:
            assert got.host(k).tobytes() == want.host(k).tobytes(), k


@pytest.mark.parametrize("region", [("planes", _tangent_planes(6, 3)), ("polygon", R.circle(1024))], ids=["planes", "polygon"])
def test_count_only_capacity_and_two_runs(G, region):
    import torch
    import schwarzwald_amd as swz
    n = 2 * G["T"] + 9
    xyz, cols = _cloud(n, 81), _columns(n, ONE_OF_EACH_WIDTH)
    want = int(R.region_mask(xyz, UNIT, region).sum())
    assert 1 < want < n
    d_xyz = torch.from_numpy(xyz).to(G["dev"])
    rg = R.as_region(swz, region)
    assert G["ctx"].region_select_device(d_xyz.data_ptr(), n, UNIT[0], UNIT[1], rg, 0, None) == want    # counts, writes nothing
    a, b = _run(G, xyz, cols, UNIT, region, capacity=want), _run(G, xyz, cols, UNIT, region, capacity=want)
    assert a[0] == b[0] == want
    a[1].assert_poison_beyond(want)
    for k in a[1].buf:
        assert a[1].host(k).tobytes() == b[1].host(k).tobytes(), k
    # one row short: refused with the needed count, every output still poison
    out = Outputs(G, want - 1, tuple(cols))
    _, d_cols = _upload(G, xyz, cols)
    with pytest.raises(swz.SwzError) as e:
        G["ctx"].region_select_device(d_xyz.data_ptr(), n, UNIT[0], UNIT[1], rg, want - 1, out.ptr("xyz"), {k: v.data_ptr() for k, v in d_cols.items()},
                                      {k: out.ptr(k) for k in cols}, d_row_out=out.ptr("row"))
    torch.cuda.synchronize()
    assert e.value.code == ERR_BAD_ARG and "capacity" in str(e.value) and e.value.needed == want
    out.assert_poison_beyond(0)


def test_refusals_launch_nothing(G):
    import torch
    import schwarzwald_amd as swz
    n = G["T"] + 1
    xyz = np.full((n, 3), 0.5)
    d_xyz = torch.from_numpy(xyz).to(G["dev"])
    out = Outputs(G, n, ())
    ctx = G["ctx"]
    plane, tri = [[1.0, 0.0, 0.0, 0.0]], [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]

    def refused(word, region, box=UNIT, xyz_out=None):
        with pytest.raises(swz.SwzError) as e:
            ctx.region_select_device(d_xyz.data_ptr(), n, box[0], box[1], region, n, out.ptr("xyz") if xyz_out is None else xyz_out,
                                     d_row_out=out.ptr("row"))
        assert e.value.code == ERR_BAD_ARG and "swz_region_select_device" in str(e.value) and word in str(e.value), str(e.value)

    refused("unknown kind", swz.Region(3, plane))
    refused("unknown kind", swz.Region(-1, plane))
    refused("reserved", swz.Region(swz.REGION_PLANES, plane, reserved=1))
    refused("1 to 16", swz.Region(swz.REGION_PLANES, plane, count=0))
    refused("1 to 16", swz.Region.planes(np.tile(plane, (17, 1))))
    refused("3 to 1024", swz.Region.polygon(tri[:2]))
    refused("3 to 1024", swz.Region.polygon(R.circle(1025)))
    refused("NULL values", swz.Region(swz.REGION_PLANES, None, count=1))
    refused("NULL values", swz.Region(swz.REGION_POLYGON, None, count=3))
    refused("not finite", swz.Region.planes([[1.0, 0.0, float("inf"), 0.0]]))
    refused("not finite", swz.Region.planes([[1.0, 0.0, 0.0, float("nan")]]))
    refused("not finite", swz.Region.polygon(tri[:2] + [[float("nan"), 1.0]]))
    refused("a = b = c = 0", swz.Region.planes([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]]))
    refused("count that is not 0", swz.Region(swz.REGION_BOX, None, count=1))
    # and what the box call refuses, with a region that is in order
    refused("box_min > box_max", swz.Region.polygon(tri), box=([0.5, 0.5, 0.5], [0.5, 0.4, 0.5]))
    refused("not finite", swz.Region.planes(plane), box=([0.0, 0.0, 0.0], [1.0, float("inf"), 1.0]))
    refused("aliases", swz.Region.polygon(tri), xyz_out=d_xyz.data_ptr())
    torch.cuda.synchronize()
    out.assert_poison_beyond(0)
    assert np.array_equal(d_xyz.cpu().numpy(), xyz)
    # n == 0: nothing is launched, the count is 0
    assert ctx.region_select_device(0, 0, UNIT[0], UNIT[1], swz.Region.polygon(tri), n, out.ptr("xyz")) == 0
    out.assert_poison_beyond(0)
