"""The source projection on the device: swz_srs_transform_device against the mpmath reference (srs_ref.py), the projecting
instantiation of the segment decode against decode -> transform -> shift bit for bit, and swz_tiler_add_las_files with a
projection against the recipe out of those calls.

ACCURACY CONDITION: every output coordinate within 1 um of the reference (see test_srs_cpu.py)."""
import json
import os

import numpy as np
import pytest

import srs_ref as R
from las_input_util import LasTile

pytestmark = pytest.mark.gpu

ERR_BAD_ARG = 2
TOL_M = 1e-6
UTM32 = R.utm_definition(32, False)
GUARD = -7.25


def _device_transform(ctx, srs, rows, target, front=3, back=5):
    """rows through srs_transform_device inside a guarded buffer; the guard rows must come back untouched"""
    import torch
    import schwarzwald_amd as swz
    n = len(rows)
    buf = torch.full((front + n + back, 3), GUARD, dtype=torch.float64, device="cuda:0")
    if n:
        buf[front:front + n] = torch.from_numpy(np.ascontiguousarray(rows)).to("cuda:0")
    ctx.srs_transform_device(srs, buf.data_ptr() + 24 * front, n, target)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:front] == GUARD).all() and (out[front + n:] == GUARD).all()
    return out[front:front + n]


def test_transform_device_within_a_micrometre_of_the_reference(capsys):
    import torch
    import schwarzwald_amd as swz
    T = swz.srs_tile()
    worst_m, worst_rad = 0.0, 0.0
    with swz.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
        for g in R.points():   # every group with its own projection, both targets
            got = _device_transform(ctx, g["definition"], g["xyz"], swz.SRS_ECEF)
            worst_m = max(worst_m, R.errors(got, g["ecef_hi"], g["ecef_lo"]).max())
            geo = _device_transform(ctx, swz.Srs(g["definition"]), g["xyz"], swz.SRS_WGS84)
            assert np.array_equal(geo[:, 2], g["xyz"][:, 2])
            worst_rad = max(worst_rad, R.errors(geo, g["wgs84_hi"], g["wgs84_lo"], angles=(0,))[:, :2].max())
        g = next(x for x in R.points() if x["definition"] == UTM32)
        for n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17):   # the points replicated and cut
            pick = np.arange(n) % len(g["xyz"])
            got = _device_transform(ctx, UTM32, g["xyz"][pick], swz.SRS_ECEF)
            again = _device_transform(ctx, UTM32, g["xyz"][pick], swz.SRS_ECEF, front=0, back=1)
            assert np.array_equal(got, again), n
            if n:
                worst_m = max(worst_m, R.errors(got, g["ecef_hi"][pick], g["ecef_lo"][pick]).max())
        # a tensor goes the same way; non-finite rows come out non-finite, the rows beside them right
        rows = g["xyz"][:4].copy()
        rows[1, 0], rows[2, 1] = np.nan, np.inf
        t = torch.from_numpy(rows).to("cuda:0")
        ctx.srs_transform_device(UTM32, t)
        torch.cuda.synchronize()
        out = t.cpu().numpy()
        assert not np.isfinite(out[1, :2]).all() and not np.isfinite(out[2, :2]).all()
        assert R.errors(out[[0, 3]], g["ecef_hi"][[0, 3]], g["ecef_lo"][[0, 3]]).max() <= TOL_M
        with pytest.raises(swz.SwzError) as e:
            ctx.srs_transform_device(UTM32, t.data_ptr(), 2 ** 32 - 65535)
        assert "2^32-65536" in str(e.value)
    with capsys.disabled():
        print("\nsrs device map: max |error| %.3g m (ECEF), %.3g rad (WGS84)" % (worst_m, worst_rad))
    assert worst_m <= TOL_M and worst_rad <= TOL_M / 6.4e6


# ------------------------------------------------------------------------------------------------ fused against staged
def test_projecting_decode_equals_decode_then_transform_bit_for_bit():
    import torch
    import schwarzwald_amd as swz
    T = swz.las_input_tile()
    rng = np.random.default_rng(99)
    # segment boundaries at rows T - 1 and T + 1, formats 0, 3 and 7, their own scales, offsets and (clamping) header boxes
    spec = [(T - 1, 0, 1, (1e-3, 2e-3, 1e-2), (412345.678, 5401234.321, 287.125)),
            (2, 3, 0, (2e-3, 1e-3, 5e-3), (500100.25, 1105000.5, 12.5)),
            (2 * T + 9, 7, 3, (1e-2, 1e-2, 1e-3), (733210.0, 8700000.125, -40.0))]
    tiles = [LasTile(rng, n, fmt, extra=extra, scale=scale, offset=offset, lo=-2 ** 17, hi=2 ** 18, clamp=True)
             for n, fmt, extra, scale, offset in spec]
    parts, segs, at, row = [], [], 0, 0
    for i, t in enumerate(tiles):   # odd byte offsets
        pad = 1 + at % 2 + 2 * (i == 2)
        parts.append(np.full(pad, 0xEE, np.uint8))
        at += pad
        assert at % 2 == 1
        segs.append(t.segment(row, at))
        parts.append(t.raw())
        at += t.n * t.record_bytes
        row += t.n
    raw = np.concatenate(parts)
    n = row
    clamped = sum(int(((t.oracle()[0] == t.bmin) | (t.oracle()[0] == t.bmax)).any()) for t in tiles)
    assert clamped >= 2                                                            # the clamp acts
    names = ["rgb", "intensity", "classification", "gps_time", "point_source_id"]
    import oracle_lib as O
    dev = torch.device("cuda:0")
    d_raw = torch.from_numpy(raw).to(dev)
    srs = swz.Srs(UTM32)

    def outputs():
        xyz = torch.full((n + 2, 3), GUARD, dtype=torch.float64, device=dev)
        cols = {}
        for name in names:
            _, dt, width = O.ATTRIBUTES[name]
            cols[name] = torch.zeros((n, width) if width > 1 else (n,), dtype=getattr(torch, np.dtype(dt).name), device=dev)
        return xyz, cols, xyz.data_ptr() + 24, {k: v.data_ptr() for k, v in cols.items()}

    with swz.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        plain, plain_cols, p, pc = outputs()
        ctx.las_decode_segments_device(d_raw.data_ptr(), len(raw), segs, p, pc)
        torch.cuda.synchronize()
        staged = plain[1:n + 1].clone()
        ctx.srs_transform_device(srs, staged)
        torch.cuda.synchronize()
        assert 6.3e6 < float(staged.norm(dim=1).min()) and float(staged.norm(dim=1).max()) < 6.4e6
        for center in (None, [4170000.5, 650000.25, 4760000.125]):
            fused, fused_cols, p, pc = outputs()
            ctx.las_decode_segments_device(d_raw.data_ptr(), len(raw), segs, p, pc, shift_center=center, srs=srs)
            torch.cuda.synchronize()
            want = staged
            if center is not None:
                want = (staged - torch.tensor(center, dtype=torch.float64, device=dev)).float().double()
                assert not torch.equal(want, staged - torch.tensor(center, dtype=torch.float64, device=dev))   # (the narrowing shows)
            assert torch.equal(fused[1:n + 1].view(torch.int64), want.view(torch.int64)), center     # identical bits
            assert (fused[0] == GUARD).all() and (fused[n + 1] == GUARD).all()
            for k in names:
                assert torch.equal(fused_cols[k], plain_cols[k]), k


# ------------------------------------------------------------------------------------------------ the one call
BATCH = 9000
CONCURRENCY = 8


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """Two files of 12 000 and 8 000 points in UTM 32N: one tile of 600 m x 660 m with 40 m of relief astride the central
    meridian at 10 degrees north, where ECEF Z is the longest axis of the data set's box, so the cubic root box is tight in
    Z.  Batches of 9 000 points: the second spans the file boundary.  Six records of the first file are placed by hand: the
    mid-point of the top north edge (and a point 1 m beside it), which maps ABOVE the box of the eight corners in Z -- the
    flat tile bulges, and a line of constant northing reaches its highest latitude on the central meridian --, two top
    north corners, the top face's centre and the mid-point of the bottom north edge, which stay inside."""
    import schwarzwald_amd as swz
    rng = np.random.default_rng(31)
    lo, hi = 0, 600000
    kw = dict(scale=(1e-3, 1.1e-3, 40.0 / 600000), offset=(499700.0, 1105000.0, 250.0), lo=lo, hi=hi)
    a, b = LasTile(rng, 12000, 3, **kw), LasTile(rng, 8000, 7, extra=1, **kw)
    mid = (lo + hi) // 2
    edge = [(mid, hi, hi), (lo, hi, hi), (hi, hi, hi), (mid, mid, hi), (mid, hi, lo), (mid - 1000, hi, hi)]
    for i, (X, Y, Z) in enumerate(edge):
        a.records["X"][100 + i], a.records["Y"][100 + i], a.records["Z"][100 + i] = X, Y, Z
    d = tmp_path_factory.mktemp("srs_in")
    paths = [a.write(d / "a.las"), b.write(d / "b.las")]
    files, ds = swz.las_scan_files(paths, srs=UTM32)
    # the reference's image of the engineered records (their decoded doubles)
    proj = R.TMerc.utm(32)
    dec = a.oracle(100, len(edge))[0]
    ref = np.array([[float(v) for v in R.image(proj, *row)[0]] for row in dec])
    return dict(tiles=[a, b], paths=paths, ds=ds, n=20000, edge_ids=np.arange(100, 100 + len(edge)), edge_ref=ref, proj=proj)


def _params(sampler, strategy, bounds):
    import oracle_lib as O
    import schwarzwald_amd as swz
    return swz.TileParams(sampler=sampler, max_points_per_node=300, spacing_at_root=O.spacing_from_diagonal(bounds[0], bounds[1], 32),
                          strategy=strategy, fast_concurrency=CONCURRENCY)


def _export(t):
    import torch
    info = t.info()
    ns = int(info["num_stored"])
    d_keys = torch.empty(ns, dtype=torch.int64, device="cuda")
    d_ids = torch.empty(ns, dtype=torch.int32, device="cuda")
    d_level = torch.empty(ns, dtype=torch.int8, device="cuda")
    t.export_device(d_keys.data_ptr(), d_ids.data_ptr(), d_level.data_ptr())
    return dict(info=info, table=t.node_table(), keys=d_keys.cpu().numpy().view(np.uint64), ids=d_ids.cpu().numpy().view(np.uint32),
                level=d_level.cpu().numpy())


def _pool_xyz(ctx, t, n):
    return ctx.copy_to_host(t.pools_device()[0], n * 24).view(np.float64).reshape(n, 3)


def test_premise_the_bulge_leaves_the_root_box(dataset):
    """from the reference positions alone: the top north edge's mid-point lies above the root box in Z by millimetres"""
    D = dataset
    over = D["edge_ref"][:, 2] - D["ds"]["center"][2] - D["ds"]["origin"][1][2]
    assert 1e-3 < over[0] < 1e-2 and over[5] > 1e-3 and over[1] <= 1e-8 and over[2] <= 1e-8   # the mid-point, not the corners
    assert (D["ds"]["cubic"][1][2] - D["ds"]["cubic"][0][2]) - (D["ds"]["tight"][1][2] - D["ds"]["tight"][0][2]) < 1e-6    # tight in Z


@pytest.mark.parametrize("sampler_name", ["MIN_DISTANCE", "RANDOM_GRID"])
@pytest.mark.parametrize("strategy_name", ["ACCURATE", "FAST"])
def test_one_call_equals_the_recipe(dataset, sampler_name, strategy_name):
    import torch
    import schwarzwald_amd as swz
    D = dataset
    sampler, strategy = getattr(swz, sampler_name), getattr(swz, strategy_name)
    bounds, center = D["ds"]["origin"], D["ds"]["center"]
    params = _params(sampler, strategy, bounds)
    cuts = swz.input_batches([t.n for t in D["tiles"]], BATCH, CONCURRENCY if strategy == swz.FAST else 0)
    assert list(cuts) == [0, 9000, 18000, 20000] and cuts[1] < D["tiles"][0].n < cuts[2]         # a batch spans the file boundary
    dev = torch.device("cuda:0")
    with swz.Context(0) as ctx:
        with swz.Tiler(ctx, bounds[0], bounds[1], params) as t:
            stats = t.add_las_files(D["paths"], batch_points=BATCH, attrs=[], shift_to_center=True, source_projection=UTM32)
            assert stats["points"] == D["n"] and stats["batches"] == 3
            t.finalize()
            one = _export(t)
            one_pool = _pool_xyz(ctx, t, D["n"])
    # the recipe: the same batches decoded unprojected, projected, shifted in torch, added from device memory
    a, b = D["tiles"]
    raw = np.concatenate([a.raw(), b.raw()])
    d_raw = torch.from_numpy(raw).to(dev)
    c = torch.tensor(center, dtype=torch.float64, device=dev)
    with swz.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        with swz.Tiler(ctx, bounds[0], bounds[1], params) as t:
            for p0, p1 in zip(cuts[:-1], cuts[1:]):
                p0, p1 = int(p0), int(p1)
                segs, row = [], 0
                for tile, first_point, byte0 in ((a, 0, 0), (b, a.n, a.n * a.record_bytes)):
                    lo_, hi_ = max(p0, first_point), min(p1, first_point + tile.n)
                    if lo_ < hi_:
                        segs.append(tile.segment(row, byte0 + (lo_ - first_point) * tile.record_bytes, lo_ - first_point, hi_ - lo_))
                        row += hi_ - lo_
                xyz = torch.empty((p1 - p0, 3), dtype=torch.float64, device=dev)
                ctx.las_decode_segments_device(d_raw.data_ptr(), len(raw), segs, xyz.data_ptr())
                ctx.srs_transform_device(UTM32, xyz)
                torch.cuda.synchronize()
                shifted = (xyz - c).float().double().contiguous()
                torch.cuda.synchronize()
                t.add_batch_device(shifted.data_ptr(), p1 - p0)
            t.finalize()
            two = _export(t)
            two_pool = _pool_xyz(ctx, t, D["n"])
    for k in ("keys", "ids", "level"):
        assert np.array_equal(one[k], two[k]), k
    for k in ("level", "key", "offset", "count"):
        assert np.array_equal(one["table"][k], two["table"][k]), k
    assert np.array_equal(one_pool.view(np.int64), two_pool.view(np.int64))
    assert one["info"]["num_points"] == D["n"] and len(one["table"]["level"]) > 20
    # the indexing clamped the bulging mid-point onto the root box, and only moved it by the bulge
    e = D["edge_ids"][0]
    assert one_pool[e, 2] == bounds[1][2] and 1e-3 < D["edge_ref"][0, 2] - center[2] - one_pool[e, 2] < 1e-2
    inside = D["edge_ids"][[1, 2, 3, 4]]
    assert np.abs(one_pool[inside] - (D["edge_ref"][[1, 2, 3, 4]] - center)).max() < float(bounds[1][0] - bounds[0][0]) / 2 * 2.0 ** -23 + TOL_M


def test_output_lands_on_the_globe(dataset, tmp_path):
    """3DTILES with global_offset = the scan's centre: positions + RTC_CENTER are the reference's ECEF within half the root
    box's extent x 2^-23 (the narrowing to float of a shifted coordinate of at most that size, half an ulp of float) + 1 um."""
    import schwarzwald_amd as swz
    D = dataset
    bounds, center = D["ds"]["origin"], D["ds"]["center"]
    out = str(tmp_path / "tiles")
    with swz.Context(0) as ctx:
        with swz.Tiler(ctx, bounds[0], bounds[1], _params(swz.RANDOM_GRID, swz.ACCURATE, bounds)) as t:
            t.add_las_files(D["paths"], batch_points=BATCH, attrs=[], shift_to_center=True, source_projection=swz.Srs(UTM32))
            t.finalize()
            ex = _export(t)
            t.write_output(out, "3DTILES", global_offset=center)
    table = ex["table"]
    assert int(table["level"][0]) == -1
    ids = ex["ids"][int(table["offset"][0]):int(table["offset"][0]) + int(table["count"][0])].astype(np.int64)
    xyz, _, rtc = swz.pnts_read_node(os.path.join(out, swz.node_name(-1, 0) + ".pnts"))[:3]
    assert list(rtc) == list(center) and len(xyz) == len(ids) > 30
    half = float(bounds[1][0] - bounds[0][0]) / 2
    a, b = D["tiles"]
    checked = 0
    for j in range(0, len(ids), max(len(ids) // 16, 1)):   # a sample: the reference takes 0.1 s per point
        g = int(ids[j])
        tile, rec = (a, g) if g < a.n else (b, g - a.n)
        ref = np.array([float(v) for v in R.image(D["proj"], *tile.oracle(rec, 1)[0][0])[0]])
        if ((ref - center < bounds[0]) | (ref - center > bounds[1])).any():
            continue   # (a point the indexing clamps)
        assert np.abs(xyz[j] + rtc - ref).max() <= half * 2.0 ** -23 + TOL_M, g
        checked += 1
    assert checked >= 12
    box = json.load(open(os.path.join(out, "r.json")))["root"]["boundingVolume"]["box"]
    mid = np.array([float(v) for v in R.image(D["proj"], 500000.0, 1105000.0 + 330.0, 270.0)[0]])
    assert np.abs(np.array(box[:3]) - mid).max() <= half
    assert 6.3e6 < np.linalg.norm(box[:3]) < 6.4e6


def test_refusals(dataset):
    import torch
    import schwarzwald_amd as swz
    D = dataset
    bounds = D["ds"]["origin"]
    params = _params(swz.RANDOM_GRID, swz.ACCURATE, bounds)
    with swz.Context(0) as ctx:
        # a root box that is the source CRS's box: the existing refusal, and the tiler is untouched
        _, plain = swz.las_scan_files(D["paths"])
        with swz.Tiler(ctx, plain["cubic"][0], plain["cubic"][1], _params(swz.RANDOM_GRID, swz.ACCURATE, plain["cubic"])) as t:
            with pytest.raises(swz.SwzError) as e:
                t.add_las_files(D["paths"], batch_points=BATCH, attrs=[], source_projection=UTM32)
            assert e.value.code == ERR_BAD_ARG and "does not contain" in str(e.value)
            assert t.info()["num_points"] == 0 and t.info()["num_batches"] == 0
            t.add_las_files(D["paths"], batch_points=BATCH, attrs=[])     # ... without the projection it is the data set's box
            assert t.info()["num_points"] == D["n"]
            with pytest.raises(swz.SwzError) as e:                        # set after a batch
                t.set_source_srs(UTM32)
            assert e.value.code == ERR_BAD_ARG and "swz_tiler_set_source_srs" in str(e.value)
            with pytest.raises(swz.SwzError):
                t.set_source_srs(None)
            assert t.info()["num_points"] == D["n"]
        with swz.Tiler(ctx, bounds[0], bounds[1], params) as t:
            with pytest.raises(swz.SwzError) as e:
                t.add_las_files(D["paths"], batch_points=BATCH, attrs=[], shift_to_center=True, source_projection="+proj=merc +datum=WGS84")
            assert "+proj=merc" in str(e.value) and t.info()["num_points"] == 0
            t.set_source_srs(UTM32)
            t.set_source_srs(None)
            t.set_source_srs(swz.Srs(UTM32))
            t.add_las_files(D["paths"], batch_points=BATCH, attrs=[], shift_to_center=True)     # the set projection holds
            assert t.info()["num_points"] == D["n"]
