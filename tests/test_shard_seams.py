"""The MIN_DISTANCE root of a sharded batch -- the one node in which a point can be rejected by a point that lives on another
shard -- on the data that puts points ON the seams between the shards: lattices with whole layers on the three octant
planes and pairs exactly one root spacing apart across them (decided by the reference's strict '<' on the float-squared
spacing), the same at pitch 0.001 (every such pair deep inside any key band: only the compare on the other shard's original
positions decides it), stacks of hundreds of duplicates on the planes with partner stacks just below them, and LAS records
with cubic bounds and with their own box (not cubic: no joint root, the chain of ghosts on positions).

N shards run on ONE device from one process through swz_group_tile (tests/cpp/test_group_seams.cpp, one run per leg); both
root drivers -- all shards sweeping at once with the lower shards' records read in place (MdShardRoot / MdPeerView), and the
chain of ghosts from shard to shard, on keys and on positions -- must give the oracle's result point for point.

The CPU tests at the top check that each generator really produces its hard case, so that a later change to a generator
cannot quietly remove it."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_min_distance_adversarial import FINE_LATTICE, FINE_LATTICE_LO, LATTICE, UNIT, _aabb, _cubic_bounds, _las_cloud, _level_spacing, _sq_dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ----------------------------------------------------------------------------------------------------------- data families
BLOCK_LO, BLOCK_HI = 96, 160  # the pitch-1 block: centred on (128, 128, 128), layers 128 exactly ON the three planes
STACK_FRACTION = 0.3          # a partner stack sits this much of the root spacing below its plane stack, per plane coordinate


def _seam_lattice_cells(seed):
    """Integer lattice coordinates in [0, 256]^3: the full pitch-1 block around the centre of the box (it lies in all eight
    octants), a coarse lattice over the whole box, plane points included -- pitch 32 (pairs exactly one spacing apart for
    spacing 32) with the centres of its cubes (corner and centre are sqrt(3) * 16 apart: exactly one spacing for the float
    16 * sqrt(3), whose square rounds to 768) --, and a little scattered background that stays away from the block."""
    rng = np.random.default_rng(seed)
    g = np.arange(BLOCK_LO, BLOCK_HI + 1, dtype=np.int64)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    c = np.arange(0, 257, 32, dtype=np.int64)
    corners = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    m = np.arange(16, 256, 32, dtype=np.int64)
    centres = np.stack(np.meshgrid(m, m, m, indexing="ij"), axis=-1).reshape(-1, 3)
    scatter = rng.integers(0, 257, size=(300, 3))
    away = np.any((scatter < BLOCK_LO - 40) | (scatter > BLOCK_HI + 40), axis=1)
    cells = np.vstack([block, corners, centres, scatter[away]])
    return cells[rng.permutation(cells.shape[0])]


def _seam_stacks(seed):
    """Unit bounds.  Stacks of 1 to 400 duplicates exactly on the octant planes -- one, two or all three coordinates 0.5 --,
    each with a partner stack STACK_FRACTION of the root spacing below the plane in every plane coordinate (a LOWER octant:
    earlier in Morton order, and for the right shard count on a lower shard), and a uniform background.
    Returns (xyz, plane stack positions, partner positions, stack sizes, partner sizes)."""
    rng = np.random.default_rng(seed)
    s = O.spacing_from_diagonal(*UNIT, 250)
    masks = [(1, 0, 0)] * 60 + [(0, 1, 0)] * 60 + [(0, 0, 1)] * 60 + [(1, 1, 0)] * 15 + [(1, 0, 1)] * 15 + [(0, 1, 1)] * 15 + [(1, 1, 1)]
    masks = np.array(masks, dtype=bool)
    pos = 0.05 + 0.9 * rng.random((masks.shape[0], 3))
    pos[masks] = 0.5
    partner = pos - STACK_FRACTION * s * masks
    reps = rng.integers(1, 401, masks.shape[0])
    reps[:12] = 400  # (stacks larger than a node are always there, four per plane orientation)
    reps[60:64] = 400
    reps[120:124] = 400
    reps[-1] = 400
    preps = rng.integers(1, 401, masks.shape[0])
    xyz = np.vstack([np.repeat(pos, reps, axis=0), np.repeat(partner, preps, axis=0), rng.random((40000, 3))])
    return xyz[rng.permutation(xyz.shape[0])], pos, partner, reps, preps


def _exactly_cubic_bounds(xyz):
    """_cubic_bounds with its corner on whole numbers and an extent of whole eighths: at UTM offsets min + extent is rounded,
    and the three extents max - min then differ in their last bits -- bounds that the key sweep, and with it the joint root,
    do not accept as a cube."""
    lo, hi = _cubic_bounds(xyz)
    lo = np.floor(np.array(lo))
    extent = np.ceil((xyz.max(axis=0) - lo).max() * 8.0) / 8.0
    return lo.tolist(), (lo + extent).tolist()


@functools.lru_cache(maxsize=None)
def family(name):
    """name -> (xyz, bounds, [(spacing_at_root, max_points_per_node), ...])"""
    if name == "seam-lattice":
        # 32 reaches the coarse pitch exactly; float32(sqrt 3) * 16 squares to exactly 3 * 256 in float: ties by rounding
        return _seam_lattice_cells(21).astype(np.float64), LATTICE, [(32.0, 500), (16.0 * float(np.float32(np.sqrt(3.0))), 500)]
    if name == "seam-lattice-0.001":
        # integer * 0.001 + offset, as LAS decoding computes it
        return FINE_LATTICE_LO + _seam_lattice_cells(21).astype(np.float64) * 0.001, FINE_LATTICE, [(float(np.float32(0.032)), 500)]
    if name == "seam-stacks":
        return _seam_stacks(22)[0], UNIT, [(O.spacing_from_diagonal(*UNIT, 250), 300)]
    if name in ("las-cubic", "las-aabb"):
        xyz = _las_cloud(3)
        bounds = _exactly_cubic_bounds(xyz) if name == "las-cubic" else _aabb(xyz)
        return xyz, bounds, [(O.spacing_from_diagonal(*bounds, 250), 2000)]
    raise KeyError(name)


FAMILIES = ["seam-lattice", "seam-lattice-0.001", "seam-stacks", "las-cubic", "las-aabb"]
CASES = [(name, case) for name in FAMILIES for case in range(2 if name == "seam-lattice" else 1)]
# the grid samplers: a spacing the sharded root takes, and one above half the extent -- the root plan's candidate level is
# then -1, which a sharded root declines
GRID_FAMILIES = ["las-cubic", "seam-lattice"]


def _grid_case(name, k):
    xyz, bounds, cases = family(name)
    extent = bounds[1][0] - bounds[0][0]
    return [cases[0], (float(np.float32(0.625 * extent)), 500)][k]


def _root_candidate_level(bounds, spacing_at_root):
    """get_node_level_to_sample_from at the root (Node.cpp:37-57): the level of the grid cells RANDOM_GRID and GRID_CENTER
    take their candidates from; -1 = "just the first point"."""
    ratio = np.float32((bounds[1][0] - bounds[0][0]) / float(np.float32(spacing_at_root)))
    return max(-1, int(np.floor(np.log2(ratio))) - 1)


@functools.lru_cache(maxsize=None)
def _oracle(name, case, sampler=O.MIN_DISTANCE, strategy=O.ACCURATE, concurrency=8, grid=False):
    """The oracle's result per (family, case, sampler, strategy), computed once.  The grid legs may end in one of the reference's
    own errors (status != 0), which the caller then expects of the library too."""
    xyz, bounds, cases = family(name)
    sp, mppn = _grid_case(name, case) if grid else cases[case]
    o = O.tile(xyz, *bounds, sampler, mppn, sp, strategy=strategy, fast_concurrency=concurrency)
    assert grid or o["status"] == 0, (name, case, sampler, o["status"])
    return o


def _by_index(o):
    """The oracle's keys, levels and dup masks by input index."""
    n = o["perm"].shape[0]
    key, level, dup = np.empty(n, np.uint64), np.empty(n, np.int32), np.empty(n, np.uint32)
    key[o["perm"]], level[o["perm"]], dup[o["perm"]] = o["keys"], o["level"], o["dup"]
    return key, level, dup


@functools.lru_cache(maxsize=None)
def _octant_bits(name):
    """(octant of every input point, the bit of the octant number that each axis sets): from the keys themselves."""
    xyz, bounds, _ = family(name)
    keys, clamped = O.index_points(xyz, *bounds)
    octant = (keys >> np.uint64(60)).astype(np.int64)
    mid = 0.5 * (np.array(bounds[0]) + np.array(bounds[1]))
    inside = np.all(clamped != mid, axis=1)
    bits = []
    for axis in range(3):
        upper = clamped[inside, axis] > mid[axis]
        bit = [b for b in range(3) if np.array_equal((octant[inside] >> b) & 1, upper.astype(np.int64))]
        assert len(bit) == 1, (name, axis, bit)
        bits.append(bit[0])
    assert sorted(bits) == [0, 1, 2]
    return octant, tuple(bits)


@functools.lru_cache(maxsize=None)
def _position_groups(name):
    """An id per distinct position (points at identical positions are interchangeable)."""
    xyz = family(name)[0]
    _, inv = np.unique(xyz, axis=0, return_inverse=True)
    return np.asarray(inv).reshape(-1)


# --------------------------------------------------------------------------------------------------------- CPU: premises
@pytest.mark.parametrize("name", FAMILIES)
def test_equal_keys_imply_equal_positions(name):
    """Then the order among tied keys cannot change the expected result."""
    xyz, bounds, _ = family(name)
    assert xyz.shape[0] <= 300000
    keys, clamped = O.index_points(xyz, *bounds)
    assert np.array_equal(clamped, xyz)  # (nothing outside the bounds: the rows the shards hold are the input's)
    order = np.argsort(keys, kind="stable")
    same_key = keys[order][1:] == keys[order][:-1]
    same_pos = np.all(xyz[order][1:] == xyz[order][:-1], axis=1)
    assert np.array_equal(same_key, same_key & same_pos), "%d neighbours in key order share a key but not a position" % int((same_key & ~same_pos).sum())


def _cross_octant_root_ties(name, case):
    """Pairs of points the oracle takes at the root, in different level-0 octants, exactly at the spacing: d^2 == float(s^2).
    Returns (pairs, pairs whose octants differ along x, y, z)."""
    from scipy.spatial import cKDTree
    xyz, bounds, cases = family(name)
    s, sq = _level_spacing(cases[case][0], -1)
    _, level, _ = _by_index(_oracle(name, case))
    octant, bits = _octant_bits(name)
    root = np.flatnonzero(level == -1)
    pairs = cKDTree(xyz[root]).query_pairs(s * (1.0 + 1e-6), output_type="ndarray")
    a, b = root[pairs[:, 0]], root[pairs[:, 1]]
    d2 = _sq_dist(xyz[a], xyz[b])
    assert not (d2 < sq).any()  # (two distinct positions taken at the root are never closer than the spacing)
    tie = (d2 == sq) & (octant[a] != octant[b])
    a, b = a[tie], b[tie]
    per_axis = [int(((((octant[a] ^ octant[b]) >> bits[axis]) & 1) == 1).sum()) for axis in range(3)]
    return int(tie.sum()), per_axis


@pytest.mark.parametrize("case", [0, 1])
def test_seam_lattice_has_exact_ties_across_the_planes(case):
    """Both points of such a pair are taken only because the compare is strict; with 2, 4 and 8 shards the planes along the
    key's first, first two and all three axes separate shards, so every orientation must be crossed."""
    xyz, bounds, cases = family("seam-lattice")
    total, per_axis = _cross_octant_root_ties("seam-lattice", case)
    print("seam-lattice case %d (spacing %r): %d root pairs exactly at the spacing in different octants; across the x / y / z plane: %r"
          % (case, cases[case][0], total, per_axis))
    assert total >= 50
    assert min(per_axis) >= 10
    # a point ON a plane belongs to the upper octant
    octant, bits = _octant_bits("seam-lattice")
    for axis in range(3):
        on = xyz[:, axis] == 128.0
        assert on.any() and (((octant[on] >> bits[axis]) & 1) == 1).all()


def _fine_cross_plane_near_ties():
    """Pairs of the pitch-0.001 lattice 32 pitches apart along an axis, in different octants (all points are active at the root)."""
    xyz, bounds, cases = family("seam-lattice-0.001")
    s, sq = _level_spacing(cases[0][0], -1)
    cells = _seam_lattice_cells(21)
    octant, _ = _octant_bits("seam-lattice-0.001")
    code = (cells[:, 0] * 1024 + cells[:, 1]) * 1024 + cells[:, 2]
    order = np.argsort(code, kind="stable")
    sorted_code = code[order]
    near = exact = 0
    for axis, step in enumerate((1024 * 1024, 1024, 1)):
        want = code + 32 * step
        at = np.minimum(np.searchsorted(sorted_code, want), sorted_code.size - 1)
        found = (sorted_code[at] == want) & (cells[:, axis] + 32 <= 256)
        a, b = np.flatnonzero(found), order[at[found]]
        cross = octant[a] != octant[b]
        d2 = _sq_dist(xyz[a[cross]], xyz[b[cross]])
        near += int((np.abs(d2 / sq - 1.0) < 1e-6).sum())
        exact += int((d2 == sq).sum())
    return near, exact


def test_fine_seam_lattice_has_near_ties_across_the_planes():
    near, exact = _fine_cross_plane_near_ties()
    print("seam-lattice-0.001: %d pairs in different octants within 1e-6 of the root spacing (%d exactly at it)" % (near, exact))
    assert near >= 1000


def test_seam_stacks_premise():
    xyz, pos, partner, reps, preps = _seam_stacks(22)
    _, bounds, cases = family("seam-stacks")
    sp, mppn = cases[0]
    s, sq = _level_spacing(sp, -1)
    assert xyz.shape[0] <= 300000
    assert int((reps > mppn).sum()) >= 10
    _, counts = np.unique(xyz, axis=0, return_counts=True)
    assert counts.max() == 400 and int((counts > mppn).sum()) >= 10
    assert ((pos == 0.5).sum(axis=1) >= 1).all() and {1, 2, 3} <= set((pos == 0.5).sum(axis=1).tolist())
    key, level, _ = _by_index(_oracle("seam-stacks", 0))
    pkey, _ = O.index_points(pos, *bounds)
    qkey, _ = O.index_points(partner, *bounds)
    lower = ((qkey >> np.uint64(60)) < (pkey >> np.uint64(60))) & (_sq_dist(pos, partner) < sq)
    assert int(lower.sum()) >= 20
    good = 0
    for j in np.flatnonzero(lower):
        stack = np.flatnonzero(np.all(xyz == pos[j], axis=1))
        mate = np.flatnonzero(np.all(xyz == partner[j], axis=1))
        assert stack.size == reps[j] and mate.size == preps[j]
        if (level[mate] == -1).any():
            # the lower partner comes first in Morton order; once it is taken no point of the plane stack can be
            assert (level[stack] != -1).all(), j
            good += 1
    print("seam-stacks: %d plane stacks with a partner in a lower octant within the spacing, %d of them rejected as a whole by "
          "a partner taken at the root; %d stacks larger than a node" % (int(lower.sum()), good, int((reps > mppn).sum())))
    assert good >= 20


def test_las_bounds_are_cubic_and_not():
    lo, hi = family("las-aabb")[1]
    assert len({round(h - l, 3) for l, h in zip(lo, hi)}) == 3
    lo, hi = family("las-cubic")[1]
    assert len({h - l for l, h in zip(lo, hi)}) == 1


@pytest.mark.parametrize("name", GRID_FAMILIES)
def test_grid_leg_spacings_cover_the_refusal_and_the_run(name):
    bounds = family(name)[1]
    assert _root_candidate_level(bounds, _grid_case(name, 0)[0]) >= 0
    assert _root_candidate_level(bounds, _grid_case(name, 1)[0]) == -1


# ----------------------------------------------------------------------------------------------------------- the driver
def _build(tmpdir):
    exe = os.path.join(tmpdir, "test_group_seams")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_group_seams.cpp"), "-o", exe,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_group_seams_driver_compiles_against_the_abi(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    assert os.path.exists(_build(str(tmp_path)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("seams_driver")))


@pytest.fixture(scope="module")
def cloud_files(tmp_path_factory):
    """family -> the raw file of n x 3 little-endian doubles the driver reads (written once per module)."""
    d = tmp_path_factory.mktemp("seams_clouds")
    files = {}

    def get(name):
        if name not in files:
            files[name] = str(d / (name + ".f64"))
            np.ascontiguousarray(family(name)[0], dtype="<f8").tofile(files[name])
        return files[name]
    return get


RECORD = np.dtype([("key", "<u8"), ("index", "<u4"), ("dup", "<u4"), ("level", "<i4"), ("shard", "<u4")])
REFUSAL = "sharded root with candidate level -1"
SWZ_ERR_BAD_ARG, SWZ_ERR_JITTER_GRID_TOO_SMALL = 2, 3  # include/swz_gpu.h


def _run(driver, cloud_files, tmp_path, name, sp, mppn, shards, what, sampler=O.MIN_DISTANCE, strategy=O.ACCURATE, concurrency=8,
         flags=0, options=(), expect_error=None):
    """One run of the driver = one leg.  Returns dict(rows, joint_possible, points, stamps); a non-zero exit, a time-out or a
    signal fails the test with the driver's output (subprocess.run kills the child when the time is up)."""
    xyz, bounds, _ = family(name)
    out = str(tmp_path / "rows.bin")
    if os.path.exists(out):
        os.remove(out)
    bits = int(np.array([sp], dtype=np.float32).view(np.uint32)[0])
    assert float(np.float32(sp)) == sp
    cmd = [driver, cloud_files(name), str(xyz.shape[0]), out] + [float(v).hex() for v in bounds[0] + bounds[1]] + [
        "0x%08x" % bits, str(mppn), str(sampler), str(strategy), str(concurrency), str(flags), str(shards)] + list(options)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if expect_error:  # (code, part of the message): swz_group_tile must decline the batch, and say why
        code, text = expect_error
        assert r.returncode == 3 and ("code %d:" % code) in r.stderr and text in r.stderr, "%s: expected error %d (%s)\n%s%s" % (
            what, code, text, r.stdout, r.stderr)
        return None
    assert r.returncode == 0, "%s: exit code %d\n%s%s" % (what, r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines and lines[-1] == "done", what + "\n" + r.stdout + r.stderr
    joint = [int(ln.split()[1]) for ln in lines if ln.startswith("joint_root_possible ")]
    shard_lines = [ln.split() for ln in lines if ln.startswith("shard ")]
    assert len(joint) == 1 and len(shard_lines) == shards, what + "\n" + r.stdout
    points = np.array([int(f[3]) for f in shard_lines])
    stamps = np.array([[float(v) for v in f[5:9]] for f in shard_lines])
    return dict(rows=np.fromfile(out, dtype=RECORD), joint_possible=joint[0], points=points, stamps=stamps)


def _compare(name, what, shards, rows, want_key, want_level, want_dup=None):
    """Point by point through the input index: every index once, its key the oracle's, its level (and dup mask) the oracle's --
    points at identical positions are interchangeable, their levels compared as sorted groups per position."""
    n = family(name)[0].shape[0]
    assert rows.shape[0] == n and np.array_equal(np.sort(rows["index"]), np.arange(n, dtype=np.uint32)), "%s: not every input index exactly once" % what
    idx = rows["index"].astype(np.int64)
    key, level, dup = np.empty(n, np.uint64), np.empty(n, np.int64), np.zeros(n, np.int64)
    key[idx], level[idx], dup[idx] = rows["key"], rows["level"], rows["dup"]
    assert np.array_equal(key, want_key), "%s: %d keys differ from the oracle's" % (what, int((key != want_key).sum()))
    got = (level & 0xFF) | (dup << 8)
    want = (want_level.astype(np.int64) & 0xFF) | ((want_dup.astype(np.int64) << 8) if want_dup is not None else 0)
    group = _position_groups(name)
    og, ow = np.lexsort((got, group)), np.lexsort((want, group))
    differs = got[og] != want[ow]
    if differs.any():
        # (both orders list the groups alike, so position k belongs to the same stack in both)
        pytest.fail("%s: %d points differ; %s" % (what, int(differs.sum()), _describe(name, shards, int(og[np.flatnonzero(differs)[0]]), level, want_level)))


def _describe(name, shards, i, level, want_level):
    """The first differing point, both levels, and whether its nearest point of the oracle's root lies on another shard."""
    xyz = family(name)[0]
    octant, _ = _octant_bits(name)
    root = np.flatnonzero((want_level == -1) & np.any(xyz != xyz[i], axis=1))
    j = int(root[np.argmin(_sq_dist(xyz[root], xyz[i]))])
    mine, other = int(octant[i]) * shards // 8, int(octant[j]) * shards // 8
    return ("first: input point %d at %r (octant %d, shard %d) has level %d, oracle %d (its stack: oracle %r); the nearest point of the oracle's root, "
            "%d at %r, squared distance %r, lies on %s shard (%d)" % (
                i, xyz[i].tolist(), int(octant[i]), mine, int(level[i]), int(want_level[i]),
                sorted(want_level[np.all(xyz == xyz[i], axis=1)].tolist())[:8], j, xyz[j].tolist(),
                float(_sq_dist(xyz[j], xyz[i])), "ANOTHER" if other != mine else "the same", other))


def _stamps_say_joint(run):
    """All shards that hold points begin the root before the first of them is done with it: they sweep together."""
    held = run["points"] > 0
    return run["stamps"][held, 1].max() < run["stamps"][held, 2].min()


def _stamps_say_turns(run):
    """No shard that holds points begins its root before the shard below it is done with its own."""
    t = run["stamps"][run["points"] > 0]
    return bool(np.all(t[1:, 1] >= t[:-1, 2]))


# ----------------------------------------------------------------------------------------------------------- GPU: the legs
@pytest.mark.gpu
@pytest.mark.parametrize("shards", [2, 4, 8])
@pytest.mark.parametrize("name,case", CASES)
def test_sharded_min_distance_root_matches_oracle(driver, cloud_files, tmp_path, name, case, shards):
    """Exact MIN_DISTANCE: the default root (joint where the bounds are cubic), the chain of ghosts on keys and on positions."""
    xyz, bounds, cases = family(name)
    sp, mppn = cases[case]
    want_key, want_level, _ = _by_index(_oracle(name, case))
    cubic = name != "las-aabb"
    several = None
    for leg, options in (("default", ()), ("chain on keys", ("SWZ_GROUP_JOINT_ROOT=0",)),
                         ("chain on positions", ("SWZ_GROUP_JOINT_ROOT=0", "SWZ_MD_KEYS=0"))):
        what = "%s, spacing %r, max_points %d, %s, %d shards" % (name, sp, mppn, leg, shards)
        run = _run(driver, cloud_files, tmp_path, name, sp, mppn, shards, what, options=options)
        several = int((run["points"] > 0).sum()) > 1
        print("%s: points per shard %r, root begun %r, root done %r" % (what, run["points"].tolist(), run["stamps"][:, 1].tolist(), run["stamps"][:, 2].tolist()))
        if leg == "default":
            assert run["joint_possible"] == (1 if cubic else 0), what
        else:
            assert run["joint_possible"] == 0, what
        if several:
            if leg == "default" and cubic:
                assert _stamps_say_joint(run), what + ": the shards did not sweep the root together"
            else:
                assert _stamps_say_turns(run), what + ": the shards did not take the root in turns"
        _compare(name, what, shards, run["rows"], want_key, want_level)
    assert several, "the family must put points on more than one shard"


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [2, 4, 8])
@pytest.mark.parametrize("name,case", CASES)
def test_sharded_property_mode_keeps_the_exact_root(driver, cloud_files, tmp_path, name, case, shards):
    """SWZ_FLAG_MIN_DISTANCE_PROPERTY: the root of a sharded batch is sampled exactly -- the oracle's set up to duplicates --, below
    it the mode's properties hold on the union of the shards."""
    from test_min_distance_property import _check_property
    xyz, bounds, cases = family(name)
    sp, mppn = cases[case]
    what = "%s, spacing %r, max_points %d, property mode, %d shards" % (name, sp, mppn, shards)
    want_key, want_level, _ = _by_index(_oracle(name, case))
    run = _run(driver, cloud_files, tmp_path, name, sp, mppn, shards, what, flags=1)
    rows = run["rows"]
    n = xyz.shape[0]
    assert rows.shape[0] == n and np.array_equal(np.sort(rows["index"]), np.arange(n, dtype=np.uint32)), what
    idx = rows["index"].astype(np.int64)
    key, level = np.empty(n, np.uint64), np.empty(n, np.int64)
    key[idx], level[idx] = rows["key"], rows["level"]
    assert np.array_equal(key, want_key), what
    assert level.min() >= -1 and level.max() <= 20, what
    # the root: the same number of points of every position as the oracle took
    group = _position_groups(name)
    got_root = np.bincount(group[level == -1], minlength=int(group.max()) + 1)
    want_root = np.bincount(group[want_level == -1], minlength=int(group.max()) + 1)
    if not np.array_equal(got_root, want_root):
        bad = np.flatnonzero(got_root != want_root)
        i = int(np.flatnonzero(group == bad[0])[0])
        pytest.fail("%s: the root differs at %d positions; %s" % (what, bad.size, _describe(name, shards, i, level, want_level)))
    order = np.lexsort((idx, rows["key"]))
    max_level = int(level.max()) - (1 if name == "seam-stacks" else 0)  # (stacks reach the deepest key level, where a node keeps what it holds)
    a, b = _check_property(rows["key"][order], rows["level"][order].astype(np.int64), xyz[idx[order]], sp, mppn, max_level)
    assert a > 0 and b > 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [2, 4, 8])
@pytest.mark.parametrize("name,case", [("seam-lattice", 0), ("seam-stacks", 0)])
def test_sharded_fast_root_matches_oracle(driver, cloud_files, tmp_path, name, case, shards):
    """FAST: the root is rebuilt on shard 0 from every shard's level-0 nodes; levels and dup masks are the oracle's."""
    xyz, bounds, cases = family(name)
    sp, mppn = cases[case]
    for conc in (2, 8):
        what = "%s, spacing %r, max_points %d, FAST %d, %d shards" % (name, sp, mppn, conc, shards)
        want_key, want_level, want_dup = _by_index(_oracle(name, case, O.MIN_DISTANCE, O.FAST, conc))
        run = _run(driver, cloud_files, tmp_path, name, sp, mppn, shards, what, strategy=O.FAST, concurrency=conc)
        _compare(name, what, shards, run["rows"], want_key, want_level, want_dup)


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [2, 4, 8])
@pytest.mark.parametrize("sampler", [O.RANDOM_GRID, O.GRID_CENTER, O.JITTERED])
@pytest.mark.parametrize("name", GRID_FAMILIES)
def test_sharded_grid_samplers_match_oracle(driver, cloud_files, tmp_path, name, sampler, shards):
    """The grid samplers with points on the faces of the root's cells and of the octants; where the root plan's candidate
    level is -1, RANDOM_GRID and GRID_CENTER decline a sharded root (SWZ_ERR_BAD_ARG, documented); where the reference's JITTERED
    throws, the sharded batch ends in the same error.  las-cubic at its own spacing runs all three samplers."""
    bounds = family(name)[1]
    for k in (0, 1):
        sp, mppn = _grid_case(name, k)
        what = "%s, spacing %r, max_points %d, %s, %d shards" % (name, sp, mppn, O.SAMPLER_NAMES[sampler], shards)
        o = _oracle(name, k, sampler, grid=True)
        if sampler != O.JITTERED and _root_candidate_level(bounds, sp) < 0:
            assert o["status"] == 0 and int((o["level"] == -1).sum()) == 1  # ("just take the first point")
            _run(driver, cloud_files, tmp_path, name, sp, mppn, shards, what, sampler=sampler, expect_error=(SWZ_ERR_BAD_ARG, REFUSAL))
        elif o["status"] == O.ERR_JITTER_GRID_TOO_SMALL:
            # (JitteredSampling throws for a root grid below its pattern's size: the reference's own error, sharded or not)
            _run(driver, cloud_files, tmp_path, name, sp, mppn, shards, what, sampler=sampler, expect_error=(SWZ_ERR_JITTER_GRID_TOO_SMALL, ""))
        else:
            assert o["status"] == 0, what
            want_key, want_level, _ = _by_index(o)
            run = _run(driver, cloud_files, tmp_path, name, sp, mppn, shards, what, sampler=sampler)
            _compare(name, what, shards, run["rows"], want_key, want_level)
