"""The Morton encode (encode_kernel, swz_encode.hip) and the synthetic generator (generate_kernel) where a truncating cast, a
clamp or a tail block can go wrong: points on and one or two steps beside cell faces in boxes whose extent is no power of two,
the box's own faces, infinities, NaN, -0.0 and denormals at the seams of the 256-point blocks, and bounds at the ends of the
double range.  Everything is compared bit for bit with the CPU oracle (index_points, generate_uniform).

Bounds at the ends of the double range: the oracle's answers are pinned by test_oracle_on_extreme_bounds.  Where 2^21 / extent
is finite (extents 1e-300 and 1e300) the kernel agrees with it and the comparison is the test.  Where it is inf or 0 (extents
5e-324 and 1e-310; -1e308 .. 1e308, whose extent overflows; max = +inf) products such as 0 * inf are NaN or inf, the oracle's
answers are those of x86-64's conversion of NaN and inf to an integer (NaN -> cell 2^21 - 1, inf -> cell 0), the kernel's
conversion saturates (NaN -> cell 0, inf -> cell 2^21 - 1): no answer is worth matching, so check_bounds refuses such bounds and
test_bounds_without_a_finite_scale_are_refused holds that nothing is launched."""
import numpy as np
import pytest

import edge_inputs as E
import oracle_lib as O

BOX_NAMES = list(E.BOXES)
LIM = E.TWO21 - 1
FULL = 0x7FFFFFFFFFFFFFFF
X_ALL, Y_ALL, Z_ALL = 0x4924924924924924, 0x2492492492492492, 0x1249249249249249


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------ CPU: the premises
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("box", BOX_NAMES)
def test_cell_face_points_straddle_their_faces(box, axis):
    """The family does what it is for: the oracle puts a point within two steps of the face between cells k - 1 and k into
    one of those two cells, and (in the boxes whose extent is no power of two) the face itself lands on either side."""
    xyz, k, ulps = E.cell_face_points(E.BOXES[box], axis, 7 + axis)
    keys, _ = O.index_points(xyz, *E.BOXES[box])
    cell = E.key_cell(keys, axis)
    assert np.all((cell == k) | (cell == np.maximum(k - 1, 0)))
    assert np.any((cell == k) & (k > 0)) and np.any(cell == k - 1)
    if box != "unit":
        on_face = (ulps == 0) & (k > 0)
        assert np.any(cell[on_face] == k[on_face]) and np.any(cell[on_face] == k[on_face] - 1)


def test_specials_are_inside_or_outside_as_meant():
    """-0.0, the smallest denormal and max itself are inside the unit cube: the oracle hands them back bit for bit."""
    sp, names = E.special_points(E.UNIT, 3)
    keys, clamped = O.index_points(sp, *E.UNIT)
    for row, name in enumerate(names):
        if name.split(" on ")[0] in ("min", "max", "-0.0", "denormal") or name.startswith("max on"):
            assert np.array_equal(_bits(clamped[row]), _bits(sp[row])), name
        else:
            assert not np.array_equal(_bits(clamped[row]), _bits(sp[row])), name
            assert np.all(clamped[row] >= 0.0) and np.all(clamped[row] <= 1.0), name
    at_max = names.index("max on axis 0")
    assert E.key_cell(keys[at_max:at_max + 1], 0)[0] == LIM


def test_oracle_on_extreme_bounds():
    """What the oracle (x86-64) returns for bounds at the ends of the double range, recorded: with a finite scale the keys
    are those of a unit cube; with scale inf or 0 they are the conversion's answers for NaN and inf."""
    def run(name, pts):
        box = E.EXTREME_BOUNDS[name][0]
        keys, clamped = O.index_points(np.array(pts, dtype=np.float64), *box)
        return [int(k) for k in keys], clamped

    # (the centre of the small box: 2^21 / 1e-300 rounds down, so 5e-301 lands just below cell 2^20)
    for name, ext, centre in (("extent 1e-300", 1e-300, 0x0FFFFFFFFFFFFFFF), ("extent 1e300", 1e300, 0x7000000000000000)):
        keys, clamped = run(name, [[0, 0, 0], [ext] * 3, [ext / 2] * 3, [-1, 5 * ext, np.nan], [ext, 0, 0]])
        assert keys == [0, FULL, centre, Y_ALL, X_ALL], name
        assert np.array_equal(clamped[3], [0.0, ext, 0.0]), name
    for name, ext in (("extent 5e-324", 5e-324), ("extent 1e-310", 1e-310)):      # scale inf
        keys, _ = run(name, [[0, 0, 0], [ext] * 3, [ext, 0, 0]])
        assert keys == [FULL, 0, Y_ALL | Z_ALL], name                             # 0 * inf = NaN -> last cell; inf -> cell 0
    keys, _ = run("-1e308 .. 1e308", [[0, 0, 0], [-1e308] * 3, [1e308] * 3, [1e308, -1e308, -1e308]])
    assert keys == [0, 0, FULL, X_ALL]                                            # scale 0; (max - min) * 0 = inf * 0 = NaN
    keys, _ = run("max = +inf", [[0, 0, 0], [1, 2, 3], [np.inf] * 3, [1e308, 0, 0]])
    assert keys == [0, 0, FULL, 0]
    for name, (box, verdict) in E.EXTREME_BOUNDS.items():
        with np.errstate(all="ignore"):
            scale = float(E.TWO21) / (np.array(box[1]) - np.array(box[0]))
        finite = bool(np.all(np.isfinite(box[0])) and np.all(np.isfinite(box[1])) and np.all(np.isfinite(scale)) and np.all(scale > 0))
        assert finite == (verdict == "accepted"), name


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    yield c
    c.close()


def _same_as_oracle(ctx, xyz, box, what):
    keys, clamped = ctx.morton_encode(xyz, *box)
    okeys, oclamped = O.index_points(xyz, *box)
    bad = np.flatnonzero(keys != okeys)
    assert bad.size == 0, "%s: %d keys differ, first at %d: %r -> %x, oracle %x" % (
        what, bad.size, bad[0], xyz[bad[0]].tolist(), int(keys[bad[0]]), int(okeys[bad[0]]))
    bad = np.flatnonzero((_bits(clamped) != _bits(oclamped)).any(axis=1))
    assert bad.size == 0, "%s: %d positions differ, first at %d: %r -> %r, oracle %r" % (
        what, bad.size, bad[0], xyz[bad[0]].tolist(), clamped[bad[0]].tolist(), oclamped[bad[0]].tolist())
    return keys


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("box", BOX_NAMES)
def test_cell_faces_match_oracle(ctx, box, axis):
    xyz, k, ulps = E.cell_face_points(E.BOXES[box], axis, 7 + axis)
    keys = _same_as_oracle(ctx, xyz, E.BOXES[box], "%s, axis %d" % (box, axis))
    # and without the oracle: the cell never decreases along the axis
    order = np.argsort(xyz[:, axis], kind="stable")
    cell = E.key_cell(keys[order], axis)
    assert np.all(np.diff(cell) >= 0)
    assert cell[0] == 0 and cell[-1] == LIM


@pytest.mark.gpu
@pytest.mark.parametrize("n", E.SPECIAL_SIZES)
@pytest.mark.parametrize("box", BOX_NAMES)
def test_specials_at_block_seams_match_oracle(ctx, box, n):
    """Faces, one step outside, infinities, NaN, +-1e308, -0.0 and a denormal at positions 0, 255, 256, 511 and n - 1 of clouds
    whose sizes end a block early, exactly and late (the staging through LDS reads three runs of 256 doubles per block)."""
    for j, xyz in enumerate(E.special_clouds(E.BOXES[box], n, 3)):
        _same_as_oracle(ctx, xyz, E.BOXES[box], "%s, n = %d, cloud %d" % (box, n, j))


@pytest.mark.gpu
def test_inside_points_keep_their_sign_bit(ctx):
    """-0.0 and a denormal are inside a box with min = 0.0, also next to a coordinate that lies ON the upper face: nothing is
    written back (a clamp would turn -0.0 into +0.0).  No oracle needed."""
    sp, names = E.special_points(E.UNIT, 3)
    rows = [r for r, name in enumerate(names) if name.split(" on ")[0] in ("-0.0", "denormal", "max") or name.startswith("max on")]
    keys, clamped = ctx.morton_encode(sp[rows], *E.UNIT)
    assert np.array_equal(_bits(clamped), _bits(sp[rows]))
    for r, key in zip(rows, keys):
        if names[r].startswith("max on axis"):
            axis = int(names[r][len("max on axis ")])
            assert E.key_cell(np.array([key]), axis)[0] == LIM, names[r]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, (_, verdict) in E.EXTREME_BOUNDS.items() if verdict == "accepted"])
def test_extreme_bounds_with_a_finite_scale_match_oracle(ctx, name):
    box = E.EXTREME_BOUNDS[name][0]
    _same_as_oracle(ctx, E.extreme_points(box, 5), box, name)


@pytest.mark.gpu
def test_bounds_without_a_finite_scale_are_refused(ctx):
    """Non-finite bounds and bounds whose 2^21 / extent is not finite and positive: SWZ_ERR_BAD_ARG, and nothing is launched
    (keys and positions on the device keep their fill)."""
    import torch
    import schwarzwald_amd as swz
    n = 66
    cases = {name: box for name, (box, verdict) in E.EXTREME_BOUNDS.items() if verdict == "refused"}
    cases["min = -inf"] = ([-np.inf, 0.0, 0.0], [1.0, 1.0, 1.0])
    cases["NaN in min"] = ([0.0, np.nan, 0.0], [1.0, 1.0, 1.0])
    cases["NaN in max"] = ([0.0, 0.0, 0.0], [1.0, 1.0, np.nan])
    cases["one axis without a finite scale"] = ([0.0, 0.0, 0.0], [1.0, 1e-310, 1.0])
    assert len(cases) == 8
    xyz = torch.full((n, 3), 0.25, dtype=torch.float64, device="cuda:0")
    keys = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for name, box in cases.items():
        with pytest.raises(swz.SwzError) as e:
            ctx.morton_encode_device(xyz.data_ptr(), n, box[0], box[1], keys.data_ptr())
        assert e.value.code == swz.api.ERR_BAD_ARG and "bounds" in str(e.value), (name, str(e.value))
        with pytest.raises(swz.SwzError) as e:
            ctx.morton_encode(np.full((n, 3), 0.25), *box)
        assert e.value.code == swz.api.ERR_BAD_ARG, name
    torch.cuda.synchronize()
    assert bool((keys == -1).all()) and bool((xyz == 0.25).all())                # nothing was launched
    # the refusal from before stays, and the same buffers are taken with bounds that have a scale
    with pytest.raises(swz.SwzError) as e:
        ctx.morton_encode_device(xyz.data_ptr(), n, [0.0, 0.0, 0.0], [1.0, 0.0, 1.0], keys.data_ptr())
    assert e.value.code == swz.api.ERR_BAD_ARG and "positive extent" in str(e.value)
    ctx.morton_encode_device(xyz.data_ptr(), n, *E.UNIT, keys.data_ptr())
    torch.cuda.synchronize()
    assert bool((keys == 7 << 57).all())                                          # cell 2^19 on every axis: octants 0, 7, 0, 0, ...


# ------------------------------------------------------------------------------------------------------------ generator
def _generate(ctx, seed, first, n, guard=8):
    import torch
    d = torch.full((n + guard, 3), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()            # (the context runs on a stream of its own: the fill must have landed)
    ctx.generate_uniform_device(seed, first, n, d.data_ptr())
    torch.cuda.synchronize()
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("first", [0, 1, 1 << 32, (1 << 40) + 3])
@pytest.mark.parametrize("n", [1, 85, 86, 257])
def test_generator_matches_oracle(ctx, n, first):
    got = _generate(ctx, 2024, first, n).cpu().numpy()
    assert np.array_equal(_bits(got[:n]), _bits(O.generate_uniform(2024, n, first)))
    assert np.all(got[n:] == -7.0)                                                # nothing behind row n


@pytest.mark.gpu
def test_generator_grid_stride_branch_matches_oracle(ctx):
    """3 n > 65536 * 256: the launch is capped at 65536 blocks and every thread writes a second value."""
    n, first, chunk = 5_600_000, 12345, 700_000
    assert 3 * n > 65536 * 256
    d = _generate(ctx, 99, first, n)
    for at in range(0, n, chunk):
        m = min(chunk, n - at)
        got = d[at:at + m].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(O.generate_uniform(99, m, first + at))), "rows %d .. %d" % (at, at + m)
    assert bool((d[n:] == -7.0).all())
