"""The one-sweep scatter pass (radix_onesweep_kernel, schwarzwald_amd/csrc/swz_sort.hip) in BOTH of its shapes, at the
edges of each: 4096 keys per tile on 256 threads (keys and values in LDS images of their own) and 8192 keys per tile on 512
threads (keys, then values through ONE image; the upper four wavefronts own no digit).  The sort picks the shape from n
(SWZ_SORT_WIDE_MIN_N); here the threshold is moved so that either shape sorts every size.

Expected: np.argsort(kind="stable"), i.e. the order (key, original index).  Every family below has ties or can have them,
so the PERMUTATION is compared, not only the sorted keys: stability is the property under test (the ranking must count
the elements of a wavefront in element order whatever the shape).  `test_expectation_sees_an_unstable_sort` shows on the CPU
that the comparison rejects two equal keys in the wrong order.

Two ways through the sort, told apart by the launches the profile counts:
  eight passes       radix_hist 1, radix_scatter 8, radix_copy 1      (SWZ_SORT_HYBRID_MIN_N at its default: no sample)
  top four digits    radix_hist 1, radix_scatter 4, radix_runs 1      (SWZ_SORT_HYBRID_TOP=4)
    that fell back   radix_hist 2, radix_scatter 4 + 8, radix_runs 1, radix_copy 1   (a run of equal top 32 bits > 4096)
"""
import contextlib

import numpy as np
import pytest

U = np.uint64
KEY_MAX = (1 << 63) - 1
FIX_LONG = 4096                      # swz_sort.hip: the longest run of equal top bits the run pass ranks
TILES = {"tile4096": 4096, "tile8192": 8192}
SHAPE_OPTS = {"tile4096": {"SWZ_SORT_WIDE_MIN_N": str((1 << 32) - 1)}, "tile8192": {"SWZ_SORT_WIDE_MIN_N": "1"}}
PATH_OPTS = {"eight_passes": {}, "top4": {"SWZ_SORT_HYBRID_TOP": "4"}}


def _sizes(T):
    # T + 1, 2T + 1 and 40T + 1 are odd and leave ONE element in the last tile;
    # 40 tiles: the look-back walks over several LOCAL entries
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 3 * T + 17, 40 * T + 1]


ALL_SIZES = sorted({n for T in TILES.values() for n in _sizes(T)})
STRIDE = U(KEY_MAX // (max(ALL_SIZES) + 1))
ONES = U(0x0101010101010101)


def _families(n):
    rng = np.random.default_rng(77 + n)
    idx = np.arange(n, dtype=U)
    three = np.array([0x00, 0x5A, 0x7F], dtype=U)
    few = np.zeros(n, dtype=U)
    for b in range(8):
        few |= three[rng.integers(0, 3, size=n)] << U(8 * b)
    last_alone = rng.integers(0, 1 << 63, size=n, dtype=U)
    last_alone[-1] = U(KEY_MAX)  # next to the padding keys ~0 of a partial tile in every pass
    last_alone[0] = U(KEY_MAX)   # and tied with the first element
    fam = {
        "random63": rng.integers(0, 1 << 63, size=n, dtype=U),
        "all_equal": np.full(n, 0x3C5A96E14B2D7788, dtype=U),
        "two_alternating": np.where(idx % U(2) == 0, U(0x5A5A5A5A5A5A5A5A), U(0x25A5A5A5A5A5A5A5)),
        "descending": idx[::-1] * STRIDE,
        # every byte of the key is the digit (bit 63 stays clear: the top digit is the index mod 128)
        "digit_is_index": ((idx % U(256)) * ONES) & U(KEY_MAX),
        "digit_is_half_index": (((idx // U(2)) % U(256)) * ONES) & U(KEY_MAX),
        "three_digits": few,
        "last_alone": last_alone,
    }
    return {k: np.ascontiguousarray(v) for k, v in fam.items()}


@pytest.fixture(scope="module")
def cases():
    """{(family, n): (keys, expected permutation)}: made once, read by every shape and path"""
    out = {}
    for n in ALL_SIZES:
        for name, keys in _families(n).items():
            assert keys.dtype == U and keys.shape == (n,) and int(keys.max()) <= KEY_MAX
            out[(name, n)] = (keys, np.argsort(keys, kind="stable").astype(np.uint32))
    return out


def _longest_run(keys, shift):
    p = np.sort(keys >> U(shift))
    edges = np.flatnonzero(np.concatenate(([True], p[1:] != p[:-1], [True])))
    return int(np.diff(edges).max())


def _expected_launches(keys, path):
    assert keys.shape[0] < (1 << 24)  # below SWZ_SORT_HYBRID_MIN_N's default: no sample is sorted
    if path == "eight_passes":
        return dict(radix_hist=1, radix_scatter=8, radix_copy=1)
    if _longest_run(keys, 32) > FIX_LONG:
        return dict(radix_hist=2, radix_scatter=4 + 8, radix_runs=1, radix_copy=1)
    return dict(radix_hist=1, radix_scatter=4, radix_runs=1)


def _stable_order_error(perm, keys, want):
    """None if perm is the stable order of keys, else what is wrong with it"""
    if not np.array_equal(np.sort(perm), np.arange(keys.shape[0], dtype=perm.dtype)):
        return "not a permutation"
    if not np.array_equal(keys[perm], keys[want]):
        return "keys out of order"
    if not np.array_equal(perm, want):
        return "equal keys out of input order"
    return None


def test_expectation_sees_an_unstable_sort():
    keys = np.array([5, 3, 5, 1, 3], dtype=U)
    want = np.argsort(keys, kind="stable").astype(np.uint32)
    assert want.tolist() == [3, 1, 4, 0, 2] and _stable_order_error(want, keys, want) is None
    swapped = want.copy()
    swapped[[3, 4]] = swapped[[4, 3]]  # the two 5s: the keys are still sorted
    assert np.array_equal(keys[swapped], keys[want])
    assert _stable_order_error(swapped, keys, want) == "equal keys out of input order"
    wrong = want.copy()
    wrong[[0, 1]] = wrong[[1, 0]]
    assert _stable_order_error(wrong, keys, want) == "keys out of order"


@pytest.fixture(scope="module")
def ctx():
    import schwarzwald_amd as swz
    c = swz.Context(0)
    c.profile_enable(True)
    yield c
    c.profile_enable(False)
    c.close()


@contextlib.contextmanager
def _options(ctx, opts):
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in opts:
            ctx.set_option(k, None)


def _launches(ctx):
    return {k: v["launches"] for k, v in ctx.profile_get().items() if k.startswith("radix_")}


SHAPE_SIZES = [(shape, n) for shape, T in TILES.items() for n in _sizes(T)]


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATH_OPTS))
@pytest.mark.parametrize("shape,n", SHAPE_SIZES, ids=["%s-n%d" % sn for sn in SHAPE_SIZES])
def test_scatter_shape_at_its_tile_edges(ctx, cases, shape, n, path):
    import torch
    d_keys = torch.empty(n, dtype=torch.int64, device="cuda")
    d_perm = torch.empty(n, dtype=torch.int32, device="cuda")
    d_sorted = torch.empty(n, dtype=torch.int64, device="cuda")
    with _options(ctx, {**SHAPE_OPTS[shape], **PATH_OPTS[path]}):
        for name in _families(1):
            keys, want = cases[(name, n)]
            tag = "%s %s %s n=%d" % (shape, path, name, n)
            launches = _expected_launches(keys, path)
            ctx.profile_reset()
            perm, ks = ctx.sort_by_key(keys)
            assert _launches(ctx) == launches, tag
            assert _stable_order_error(perm, keys, want) is None, tag + " (host): " + str(_stable_order_error(perm, keys, want))
            assert np.array_equal(ks, keys[want]), tag

            d_keys.copy_(torch.from_numpy(keys.view(np.int64)))
            d_perm.fill_(-1)
            d_sorted.fill_(-1)
            torch.cuda.synchronize()
            ctx.profile_reset()
            ctx.sort_by_key_device(d_keys.data_ptr(), n, d_perm.data_ptr(), d_sorted.data_ptr())
            assert _launches(ctx) == launches, tag
            perm = d_perm.cpu().numpy().view(np.uint32)
            assert _stable_order_error(perm, keys, want) is None, tag + " (device): " + str(_stable_order_error(perm, keys, want))
            assert np.array_equal(d_sorted.cpu().numpy().view(U), keys[want]), tag
            assert np.array_equal(d_keys.cpu().numpy().view(U), keys), tag  # the input stays as it was
