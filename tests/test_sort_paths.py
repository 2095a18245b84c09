"""The radix sort, the scan under it and the octant partition (schwarzwald_amd/csrc/swz_sort.hip) on every way through
the file and at the edges of each, against np.argsort(kind="stable"): the order is (key, original index).

Every sort also says which way it took.  With profiling on, the ProfScope names count the launches of one call, and
`_expected_launches` works out from the keys and the options what the code as it stands must show:

  one-sweep eight passes   radix_hist 1, radix_scatter 8, radix_copy 1
  three-kernel passes      radix_hist 8, radix_scan 8, radix_scatter 8, radix_copy 1
  hybrid, top K digits     radix_hist 1, radix_scatter 8 + K (the sample is sorted by eight passes first), radix_runs 1
  hybrid that fell back    radix_hist 2, radix_scatter 8 + K + 8, radix_runs 1, radix_copy 1
  hybrid whose sample      radix_hist 1, radix_scatter 8 + 8, radix_copy 1
    asks for all 8 digits

so a case cannot pass on a path it did not mean to test.  The device entry points get their output buffers filled
with 0xFF first: a slot the run pass never wrote shows."""
import contextlib

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

U = np.uint64
KEY_MAX = (1 << 63) - 1
SWZ_ERR_TOO_MANY_POINTS = 6  # include/swz_gpu.h
# constants of swz_sort.hip the cases are built around
RS_TILE, SC_TILE, SCAN_ONE_BLOCK, FIX_TILE, FIX_SHORT, FIX_LONG, SAMPLES = 4096, 2048, 4096, 1024, 16, 4096, 32768


@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    c.profile_enable(True)
    yield c
    c.profile_enable(False)
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@contextlib.contextmanager
def _options(ctx, opts):
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in opts:
            ctx.set_option(k, None)


# ----------------------------------------------------------------------------------------- which path a call takes
def _sampled_top(keys):
    """radix_sample_kernel + radix_sample_ties_kernel: the K the sort reads off its sorted sample."""
    n = keys.shape[0]
    samples = min(n, SAMPLES)
    s = np.sort(keys[(np.arange(samples, dtype=U) * U(n)) // U(samples)])
    ties32 = int(np.count_nonzero((s[1:] >> U(32)) == (s[:-1] >> U(32))))
    ties48 = int(np.count_nonzero((s[1:] >> U(16)) == (s[:-1] >> U(16))))
    return 4 if ties32 <= 2 else (6 if ties48 <= 2 else 8)


def _longest_run(keys, shift):
    p = np.sort(keys >> U(shift))
    edges = np.flatnonzero(np.concatenate(([True], p[1:] != p[:-1], [True])))
    return int(np.diff(edges).max())


def _expected_launches(keys, opts):
    """(launch counts per radix_* ProfScope of one sort call, short description of the path)"""
    if opts.get("SWZ_SORT_ONESWEEP") == "0":
        return dict(radix_hist=8, radix_scan=8, radix_scatter=8, radix_copy=1), "three-kernel"
    if "SWZ_SORT_HYBRID_MIN_N" not in opts:
        assert keys.shape[0] < (1 << 24)
        return dict(radix_hist=1, radix_scatter=8, radix_copy=1), "one-sweep"
    assert opts["SWZ_SORT_HYBRID_MIN_N"] == "1"
    top = int(opts["SWZ_SORT_HYBRID_TOP"]) if "SWZ_SORT_HYBRID_TOP" in opts else _sampled_top(keys)
    if top == 8:
        return dict(radix_hist=1, radix_scatter=16, radix_copy=1), "sampled-8"
    short_max = max(1, min(FIX_SHORT, int(opts.get("SWZ_SORT_FIX_SHORT", FIX_SHORT))))
    long_max = max(short_max, min(FIX_LONG, int(opts.get("SWZ_SORT_FIX_LONG", FIX_LONG))))
    if _longest_run(keys, 64 - 8 * top) > long_max:
        return dict(radix_hist=2, radix_scatter=8 + top + 8, radix_runs=1, radix_copy=1), "hybrid-%d-fallback" % top
    return dict(radix_hist=1, radix_scatter=8 + top, radix_runs=1), "hybrid-%d" % top


def _launches(ctx):
    return {k: v["launches"] for k, v in ctx.profile_get().items() if k.startswith("radix_")}


# ----------------------------------------------------------------------------------------- the three entry points
def _check(tag, perm, ks, keys, want):
    assert np.array_equal(perm, want), tag
    if ks is not None:
        assert np.array_equal(ks, keys[want]), tag


def _sort_host(ctx, keys, want, launches, tag):
    ctx.profile_reset()
    perm, ks = ctx.sort_by_key(keys)
    assert _launches(ctx) == launches, tag
    _check(tag, perm, ks, keys, want)


class _DeviceBuffers:
    """torch tensors for swz_sort_by_key_device, made once per size"""

    def __init__(self, torch, n):
        self.torch, self.n = torch, n
        self.keys = torch.empty(n, dtype=torch.int64, device="cuda")
        self.perm = torch.empty(n, dtype=torch.int32, device="cuda")
        self.sorted = torch.empty(n, dtype=torch.int64, device="cuda")

    def sort(self, ctx, keys, want, launches, tag, with_sorted):
        t = self.torch
        self.keys.copy_(t.from_numpy(keys.view(np.int64)))
        self.perm.fill_(-1)
        self.sorted.fill_(-1)
        t.cuda.synchronize()
        ctx.profile_reset()
        ctx.sort_by_key_device(self.keys.data_ptr(), self.n, self.perm.data_ptr(), self.sorted.data_ptr() if with_sorted else None)
        assert _launches(ctx) == launches, tag
        perm = self.perm.cpu().numpy().view(np.uint32)
        ks = self.sorted.cpu().numpy().view(U)
        _check(tag, perm, ks if with_sorted else None, keys, want)
        if not with_sorted:
            assert np.all(ks == U(0xFFFFFFFFFFFFFFFF)), tag  # a buffer that was not passed is not written
        assert np.array_equal(self.keys.cpu().numpy().view(U), keys), tag  # the input keys stay as they were


# ----------------------------------------------------------------------------------------- 1. path x size x key family
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769,
         65536, 65537]
STRIDE = U(KEY_MAX // 65537)  # n distinct multiples stay below 2^63 and differ in every byte
BYTE_BASE = 0x3C5A96E14B2D7788


def _families(n):
    rng = np.random.default_rng(1000 + n)
    idx = np.arange(n, dtype=U)
    fam = {
        "random63": rng.integers(0, 1 << 63, size=n, dtype=U),
        "all_zero": np.zeros(n, dtype=U),                      # 1024 equal digits per wave: the most a 16-bit counter holds
        "all_max": np.full(n, KEY_MAX, dtype=U),
        "two_alternating": np.where(idx % U(2) == 0, U(0x5A5A5A5A5A5A5A5A), U(0x25A5A5A5A5A5A5A5)),
        "ascending": idx * STRIDE,
        "descending": idx[::-1] * STRIDE,
        "descending_x3": ((idx[::-1] // U(3)) * STRIDE),
        # a few distinct keys that differ in the top digit only
        "top_digit_only": (np.array([0, 1, 0x10, 0x40, 0x7F], dtype=U)[rng.integers(0, 5, size=n)] << U(56)) | U(BYTE_BASE & ((1 << 56) - 1)),
        # the top 48 bits tell all keys apart, the top 32 do not (a large sample chooses six digits)
        "top48_distinct": (U(0x1234) << U(48)) | (rng.permutation(1 << 17)[:n].astype(U) << U(16)) | rng.integers(0, 1 << 16, size=n, dtype=U),
    }
    for b in range(8):  # a constant with only byte b random (7 bits of byte 7)
        base = U(BYTE_BASE & ~(0xFF << (8 * b)) & KEY_MAX)
        fam["byte%d_only" % b] = base | (rng.integers(0, 128 if b == 7 else 256, size=n, dtype=U) << U(8 * b))
    return {k: np.ascontiguousarray(v) for k, v in fam.items()}


@pytest.fixture(scope="module")
def cases():
    """{(family, n): (keys, expected permutation)}: made once, read by every path"""
    out = {}
    for n in SIZES:
        for name, keys in _families(n).items():
            assert keys.dtype == U and keys.shape == (n,) and int(keys.max()) <= KEY_MAX
            want = np.argsort(keys, kind="stable").astype(np.uint32)
            assert np.array_equal(want, O.sort_by_key(keys)), (name, n)  # the oracle's order is the same one
            out[(name, n)] = (keys, want)
    return out


PATHS = {
    "default": {},
    "three_kernel": {"SWZ_SORT_ONESWEEP": "0"},
    "hybrid_top2": {"SWZ_SORT_HYBRID_MIN_N": "1", "SWZ_SORT_HYBRID_TOP": "2"},
    "hybrid_top4": {"SWZ_SORT_HYBRID_MIN_N": "1", "SWZ_SORT_HYBRID_TOP": "4"},
    "hybrid_top6": {"SWZ_SORT_HYBRID_MIN_N": "1", "SWZ_SORT_HYBRID_TOP": "6"},
    "hybrid_sampled": {"SWZ_SORT_HYBRID_MIN_N": "1"},
}
# the paths a sweep over all families and sizes must have met (no case list that quietly stops reaching one)
PATHS_MET = {
    "default": {"one-sweep"},
    "three_kernel": {"three-kernel"},
    "hybrid_top2": {"hybrid-2", "hybrid-2-fallback"},
    "hybrid_top4": {"hybrid-4", "hybrid-4-fallback"},
    "hybrid_top6": {"hybrid-6", "hybrid-6-fallback"},
    "hybrid_sampled": {"hybrid-4", "hybrid-6", "sampled-8"},
}


@pytest.mark.parametrize("path", list(PATHS))
def test_sort_every_path_size_and_key_family(ctx, torch, cases, path):
    """Each path of radix_sort_pairs at sizes around the wave (64), the workgroup (256), the run-pass tile (1024), the
    sort tile (4096, 8192), the sample (32768) and 4096 scan entries of the three-kernel path (65536 keys = 16 tiles x 256
    digits; 65537 is one more tile), on keys that are random, all equal, alternating, sorted, reversed, reversed with
    ties, different in one byte only or in the top digit only; through swz_sort_by_key and swz_sort_by_key_device with
    and without d_keys_sorted."""
    opts = PATHS[path]
    assert (65536 // RS_TILE) * 256 == SCAN_ONE_BLOCK  # the last two sizes straddle the one-block scan
    met = set()
    with _options(ctx, opts):
        for n in SIZES:
            dev = _DeviceBuffers(torch, n)
            for (name, m), (keys, want) in cases.items():
                if m != n:
                    continue
                launches, what = _expected_launches(keys, opts)
                met.add(what)
                tag = "%s n=%d %s (%s)" % (name, n, path, what)
                _sort_host(ctx, keys, want, launches, tag + " host")
                dev.sort(ctx, keys, want, launches, tag + " device", with_sorted=True)
                dev.sort(ctx, keys, want, launches, tag + " device, no sorted keys", with_sorted=False)
    assert met == PATHS_MET[path]


# ----------------------------------------------------------------------------------------- 2. the run pass, runs placed by hand
LIMITS = {"default": (16, 4096, {}),
          "short3": (3, 4096, {"SWZ_SORT_FIX_SHORT": "3", "SWZ_SORT_FIX_LONG": "4096"}),
          "short1": (1, 4096, {"SWZ_SORT_FIX_SHORT": "1", "SWZ_SORT_FIX_LONG": "4096"}),
          "short2_long5": (2, 5, {"SWZ_SORT_FIX_SHORT": "2", "SWZ_SORT_FIX_LONG": "5"})}
LOWS = ("ties", "equal", "distinct")
HYBRID4 = {"SWZ_SORT_HYBRID_MIN_N": "1", "SWZ_SORT_HYBRID_TOP": "4"}
RUNS_DONE = dict(radix_hist=1, radix_scatter=12, radix_runs=1)            # the run pass finished the sort
RUNS_FELL_BACK = dict(radix_hist=2, radix_scatter=20, radix_runs=1, radix_copy=1)


def _run_keys(lengths, low, seed):
    """Keys (run_id << 32) | low with run r of the sorted order lengths[r] long, in shuffled input order.  low: "ties" draws
    from 0..3 (runs full of equal keys), "equal" is one value, "distinct" has no two alike."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = int(lengths.sum())
    rng = np.random.default_rng(seed)
    run_id = np.repeat(np.arange(1, lengths.shape[0] + 1, dtype=U), lengths)
    if low == "ties":
        lo = rng.integers(0, 4, size=n, dtype=U)
    elif low == "equal":
        lo = np.full(n, 3, dtype=U)
    else:
        lo = rng.permutation(n).astype(U)
    return np.ascontiguousarray(((run_id << U(32)) | lo)[rng.permutation(n)])


def _lengths_with(placements, n):
    """run lengths of n keys with a run of L keys starting at sorted position start for every (start, L); runs of 1 between"""
    out, pos = [], 0
    for start, L in sorted(placements):
        assert start >= pos
        out += [1] * (start - pos) + [L]
        pos = start + L
    assert pos <= n
    return out + [1] * (n - pos)


def _sort_runs(ctx, torch, lengths, opts, launches, tag, placements=()):
    for low in LOWS:
        keys = _run_keys(lengths, low, seed=len(lengths))
        want = np.argsort(keys, kind="stable").astype(np.uint32)
        top = keys[want] >> U(32)
        for start, L in placements:  # the construction puts the run where it says
            assert np.all(top[start:start + L] == top[start]) and (start == 0 or top[start - 1] != top[start])
            assert start + L == keys.shape[0] or top[start + L] != top[start]
        assert _expected_launches(keys, opts)[0] == launches, tag
        t = "%s low=%s" % (tag, low)
        _sort_host(ctx, keys, want, launches, t + " host")
        _DeviceBuffers(torch, keys.shape[0]).sort(ctx, keys, want, launches, t + " device", with_sorted=True)


@pytest.mark.parametrize("limits", list(LIMITS))
def test_run_pass_every_run_length(ctx, torch, limits):
    """Runs of every length from 1 to short_max + 2 (e - s <= short_max decides between the element's own ranking and
    the workgroup's), of long_max - 1 and long_max (ranked by a workgroup, no fall-back, radix_copy absent), and of
    long_max + 1 (len > long_max: eight passes after all, the result still exact)."""
    short_max, long_max, lim = LIMITS[limits]
    opts = dict(HYBRID4, **lim)
    rng = np.random.default_rng(short_max * 7 + long_max)
    lengths = list(range(1, short_max + 3)) * 3 + [long_max - 1, long_max] + [1] * 700
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    with _options(ctx, opts):
        _sort_runs(ctx, torch, lengths, opts, RUNS_DONE, "%s lengths to long_max" % limits)
        for at in (0, len(lengths) // 2, len(lengths)):
            longer = lengths[:at] + [long_max + 1] + lengths[at:]
            _sort_runs(ctx, torch, longer, opts, RUNS_FELL_BACK, "%s long_max + 1 as run %d" % (limits, at))


@pytest.mark.parametrize("limits", list(LIMITS))
def test_run_pass_runs_at_seams_and_ends(ctx, torch, limits):
    """A run of short_max, short_max + 1 or long_max keys at sorted position 0, ending exactly at n, and starting
    1024 k - j keys in for j in {0, 1, L - 1, L, 17, 18}: across and against the seams of the 1024-key tiles of
    radix_fix_short_kernel, whose halo of 17 keys is read at exactly own slot +- 17; and two long runs back to back."""
    short_max, long_max, lim = LIMITS[limits]
    opts = dict(HYBRID4, **lim)
    tail = 1500
    with _options(ctx, opts):
        for L in sorted({short_max, short_max + 1, long_max}):
            _sort_runs(ctx, torch, _lengths_with([(0, L)], L + tail), opts, RUNS_DONE, "%s L=%d at 0" % (limits, L), [(0, L)])
            _sort_runs(ctx, torch, _lengths_with([(tail + 1, L)], tail + 1 + L), opts, RUNS_DONE, "%s L=%d ends at n" % (limits, L),
                       [(tail + 1, L)])
            k0 = L // FIX_TILE  # seams 1 and 2, and the first two that a run of L keys can start L keys in front of
            for k in sorted({1, 2, k0 + 1, k0 + 2}):
                for j in sorted({0, 1, L - 1, L, 17, 18}):
                    start = FIX_TILE * k - j
                    if start < 0:
                        continue
                    _sort_runs(ctx, torch, _lengths_with([(start, L)], start + L + tail), opts, RUNS_DONE,
                               "%s L=%d at 1024*%d-%d" % (limits, L, k, j), [(start, L)])
        for a, b in ((short_max + 1, long_max), (long_max, short_max + 1), (long_max, long_max)):
            for start in (0, 1000):
                pl = [(start, a), (start + a, b)]
                _sort_runs(ctx, torch, _lengths_with(pl, start + a + b + tail), opts, RUNS_DONE,
                           "%s long runs of %d and %d back to back at %d" % (limits, a, b, start), pl)
                _sort_runs(ctx, torch, _lengths_with(pl, start + a + b), opts, RUNS_DONE,
                           "%s long runs of %d and %d back to back at %d, ending at n" % (limits, a, b, start), pl)


def test_run_pass_more_long_runs_than_workgroups(ctx, torch):
    """radix_fix_long_kernel is launched with 1024 workgroups and loops r += gridDim.x: 1500 runs of 3 to 5 keys with
    short_max = 2 are 1500 long runs."""
    opts = dict(HYBRID4, SWZ_SORT_FIX_SHORT="2")
    lengths = np.random.default_rng(5).integers(3, 6, size=1500).tolist()
    assert len(lengths) > 1024 and min(lengths) > 2
    with _options(ctx, opts):
        _sort_runs(ctx, torch, lengths, opts, RUNS_DONE, "1500 long runs")


@pytest.mark.parametrize("limits", list(LIMITS))
def test_run_pass_fills_the_long_run_list(ctx, torch, limits):
    """Every run exactly short_max + 1 long and n a multiple of that: n / (short_max + 1) long runs, all that the
    list of n / (short_max + 1) + 1 entries is ever asked to hold."""
    short_max, long_max, lim = LIMITS[limits]
    opts = dict(HYBRID4, **lim)
    runs = 1200
    with _options(ctx, opts):
        _sort_runs(ctx, torch, [short_max + 1] * runs, opts, RUNS_DONE, "%s %d runs of short_max + 1" % (limits, runs))


# ----------------------------------------------------------------------------------------- 3. octant partition
def _partition_families(n):
    rng = np.random.default_rng(2000 + n)
    low = rng.integers(0, 1 << 56, size=n, dtype=U)
    return {
        "uniform": rng.integers(0, 1 << 63, size=n, dtype=U),
        "octant0": rng.integers(0, 1 << 60, size=n, dtype=U),
        "octant7": (U(7) << U(60)) | rng.integers(0, 1 << 60, size=n, dtype=U),
        "octants_0_and_7": (rng.integers(0, 2, size=n, dtype=U) * U(7) << U(60)) | rng.integers(0, 1 << 60, size=n, dtype=U),
        # every top byte 0..127 in rotation: inside an octant the bits 56..59 run against the index order, which
        # tells (octant, index) from (top byte, index)
        "top_bytes_in_rotation": ((U(127) - np.arange(n, dtype=U) % U(128)) << U(56)) | low,
    }


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 65536, 65537, 300001])
def test_partition_by_octant_counts_and_order(ctx, torch, n):
    """swz_partition_by_octant_device against its contract (include/swz_gpu.h): counts per octant, and the permutation
    ordered by (octant, original index) whatever the key bits below the octant are."""
    for name, keys in _partition_families(n).items():
        octant = (keys >> U(60)).astype(np.int64)
        d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
        d_perm = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        counts = ctx.partition_by_octant_device(d_keys.data_ptr(), n, d_perm.data_ptr())
        assert counts == np.bincount(octant, minlength=8).tolist(), name
        assert np.array_equal(d_perm.cpu().numpy().view(np.uint32), np.argsort(octant, kind="stable").astype(np.uint32)), name
        assert np.array_equal(d_keys.cpu().numpy().view(U), keys), name


def test_partition_by_octant_scan_second_recursion(ctx, torch):
    """n = 2^27 + 1 keys are 32769 tiles, 32769 x 256 histogram entries, 4097 scan tiles of 2048: one more than the 4096
    partial sums a single block scans, so scan_exclusive_u32 recurses a second time.  Keys and the expected order are
    made on the device."""
    n = (1 << 27) + 1
    ntiles = -(-n // RS_TILE)
    assert -(-(ntiles * 256) // SC_TILE) == SCAN_ONE_BLOCK + 1
    gen = torch.Generator(device="cuda")
    gen.manual_seed(27)
    d_keys = torch.randint(0, KEY_MAX, (n,), dtype=torch.int64, device="cuda", generator=gen)
    d_perm = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    counts = ctx.partition_by_octant_device(d_keys.data_ptr(), n, d_perm.data_ptr())
    octant = (d_keys >> 60).to(torch.uint8)
    assert counts == torch.bincount(octant.to(torch.int32), minlength=8).tolist()
    want = torch.sort(octant, stable=True).indices.to(torch.int32)
    assert torch.equal(d_perm, want)
    del want, octant, d_keys, d_perm
    torch.cuda.empty_cache()
    ctx.release_workspace()


# ----------------------------------------------------------------------------------------- 4. limits of n
def test_too_many_points_is_refused_before_any_buffer_is_touched(ctx, torch):
    import schwarzwald_amd as swz
    n = (1 << 32) - 65535
    d_keys = torch.arange(16, dtype=torch.int64, device="cuda")
    d_perm = torch.full((16,), -1, dtype=torch.int32, device="cuda")
    d_sorted = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(swz.SwzError) as e:
        ctx.sort_by_key_device(d_keys.data_ptr(), n, d_perm.data_ptr(), d_sorted.data_ptr())
    assert e.value.code == SWZ_ERR_TOO_MANY_POINTS
    with pytest.raises(swz.SwzError) as e:
        ctx.partition_by_octant_device(d_keys.data_ptr(), n, d_perm.data_ptr())
    assert e.value.code == SWZ_ERR_TOO_MANY_POINTS
    assert d_keys.tolist() == list(range(16)) and d_perm.tolist() == [-1] * 16 and d_sorted.tolist() == [-1] * 16
    # the largest n that is allowed is refused for its NULL buffers, not for its size
    with pytest.raises(swz.SwzError) as e:
        ctx.sort_by_key_device(None, (1 << 32) - 65536, None, None)
    assert e.value.code == swz.api.ERR_BAD_ARG


def test_no_points_need_no_buffers(ctx):
    ctx.profile_reset()
    ctx.sort_by_key_device(None, 0, None, None)
    assert ctx.partition_by_octant_device(None, 0, None) == [0] * 8
    perm, ks = ctx.sort_by_key(np.zeros(0, dtype=U))
    assert perm.shape == (0,) and ks.shape == (0,)
    assert _launches(ctx) == {}
