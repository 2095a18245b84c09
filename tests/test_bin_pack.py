"""BIN node files packed on the device: swz_bin_layout, swz_bin_pack_device, swz_bin_persist_nodes_image.

The expected bytes of every body are the file swz_bin_write_node writes from the gathered host rows (tests/test_bin_persistence.py
holds that writer against the reference's format); nothing here comes from the code under test.  A body of the image is the
whole file, every body starts on a multiple of 8, and the bytes up to the next multiple of 8 are zeros.

CPU part: the layout's file sizes against written files, the alignment of the bodies, the refusals of the host functions, and
that the counts the GPU part uses put the normals' floats on every byte alignment.  GPU part: a node table placed by the 256-row
tile, four masks, with and without `order`, guards around a pre-filled image, and the files out of a host copy of the image.
"""
import os

import numpy as np
import pytest

ERR_BAD_ARG = 2
ALL = ("rgb", "normal", "intensity", "classification", "edge_of_flight_line", "gps_time", "number_of_returns", "return_number",
       "point_source_id", "scan_direction_flag", "scan_angle_rank", "user_data")
MASKS = [(), ("rgb",), ("rgb", "normal", "gps_time"), ALL]
EDGE_COUNTS = [0, 1, 3, 4, 5, 255, 256, 257]
GUARD = 64
TILE = 256
N = 3 * TILE + 37


def _columns(rng, n):
    return {
        "rgb": rng.integers(0, 255, (n, 3), endpoint=True).astype(np.uint8),
        "normal": rng.standard_normal((n, 3)).astype(np.float32),
        "intensity": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16),
        "classification": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "edge_of_flight_line": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "gps_time": rng.random(n) * 1e9,
        "number_of_returns": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "return_number": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "point_source_id": rng.integers(0, 65535, n, endpoint=True).astype(np.uint16),
        "scan_direction_flag": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
        "scan_angle_rank": rng.integers(-128, 127, n, endpoint=True).astype(np.int8),
        "user_data": rng.integers(0, 255, n, endpoint=True).astype(np.uint8),
    }


def _written_file(tmp, xyz, cols, names, rows):
    """the bytes swz_bin_write_node writes for these rows"""
    import schwarzwald_amd as swz
    path = os.path.join(str(tmp), "want.bin")
    if os.path.exists(path):
        os.remove(path)
    swz.bin_write_node(path, xyz[rows], {a: cols[a][rows] for a in names})
    return open(path, "rb").read()


def _small_nodes():
    """(offset, count): nodes of 1, 2, 3 and 5 points back to back in one wavefront, empty nodes, unlisted rows in between"""
    nodes = [(0, 1), (1, 2), (3, 3), (6, 5), (11, 0),  # back to back, then an empty node
             (20, 3), (23, 0), (23, 1),                # unlisted rows 11..19 in front; an empty node between two others
             (30, 7), (40, 0)]
    off = np.array([o for o, _ in nodes], np.uint64)
    cnt = np.array([c for _, c in nodes], np.uint64)
    return off, cnt


def _tables():
    """Two tables over n = N rows (a node of 700 rows and one of exactly 256 rows on a tile edge do not fit one table of 805
    rows together with the small ones): A the small nodes, then 700 rows from mid-tile to the last row; B a node of exactly one
    tile on a tile edge between small ones, the last node ending at n."""
    off, cnt = _small_nodes()
    a_off = np.concatenate([off, np.array([N - 700], np.uint64)])
    a_cnt = np.concatenate([cnt, np.array([700], np.uint64)])
    assert int(a_off[-1]) % TILE != 0 and int(a_off[-1]) > 40 and int(a_off[-1] + a_cnt[-1]) == N
    assert (int(a_off[-1]) // TILE, (N - 1) // TILE) == (0, 3)  # it reaches from the first tile into the fourth
    b = [(0, 5), (5, 0), (100, 156), (TILE, TILE), (2 * TILE, 4), (2 * TILE + 4, 257), (3 * TILE + 5, 0), (3 * TILE + 10, 27)]
    b_off = np.array([o for o, _ in b], np.uint64)
    b_cnt = np.array([c for _, c in b], np.uint64)
    assert int(b_off[-1] + b_cnt[-1]) == N
    return [(a_off, a_cnt), (b_off, b_cnt)]


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("names", MASKS)
def test_layout_file_sizes_equal_written_files(tmp_path, names):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(3)
    n = max(EDGE_COUNTS)
    xyz, cols = rng.random((n, 3)), _columns(rng, n)
    lay = swz.bin_layout(EDGE_COUNTS, names)
    at = 0
    for k, c in enumerate(EDGE_COUNTS):
        want = len(_written_file(tmp_path, xyz, cols, names, np.arange(c))) if c else 0
        assert int(lay["file_size"][k]) == want, (names, c)
        assert int(lay["offset"][k]) == at and at % 8 == 0
        assert int(lay["size"][k]) == (want + 7) // 8 * 8
        at += int(lay["size"][k])
    assert lay["total"] == at


def test_chosen_counts_put_the_normals_on_every_alignment():
    # the normals' floats start at 12 + (24 + 3) * count of a body that starts on a multiple of 8
    counts = [int(c) for _, cnt in _tables() for c in cnt if c]
    assert {(12 + 27 * c) % 4 for c in counts} == {0, 1, 2, 3}
    # ... and the GPS doubles, behind 24 + 3 + 12 bytes per row, on every alignment mod 8 a body allows
    assert len({(12 + 39 * c) % 8 for c in counts}) >= 4


def test_host_refusals(tmp_path):
    import ctypes as C
    import schwarzwald_amd as swz
    L = swz.load_library()
    cnt = np.array([3, 4], np.uint64)
    p = cnt.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.swz_bin_layout(2, p, 0, None, None, None, None) == 0
    assert L.swz_bin_layout(2, None, 0, None, None, None, None) == ERR_BAD_ARG           # no counts
    assert L.swz_bin_layout(2, p, 1 << 12, None, None, None, None) == ERR_BAD_ARG         # a bit that does not exist
    big = np.array([2 ** 32], np.uint64)
    assert L.swz_bin_layout(1, big.ctypes.data_as(C.POINTER(C.c_uint64)), 0, None, None, None, None) == ERR_BAD_ARG
    nodes = dict(level=np.array([-1, 0], np.int8), key=np.zeros(2, np.uint64), count=cnt)
    image = np.zeros(swz.bin_layout(cnt)["total"], np.uint8)
    with pytest.raises(swz.SwzError):  # the image is shorter than the layout
        swz.bin_persist_nodes_image(str(tmp_path), nodes, image[:-8])
    with pytest.raises(swz.SwzError):  # a mask bit that does not exist
        swz.bin_persist_nodes_image(str(tmp_path), nodes, image, attrs=1 << 12)
    with pytest.raises(swz.SwzError):  # a level that has no name
        swz.bin_persist_nodes_image(str(tmp_path), dict(nodes, level=np.array([-1, 21], np.int8)), image)
    with pytest.raises(swz.SwzError):  # a directory that is not there
        swz.bin_persist_nodes_image(str(tmp_path / "missing"), nodes, image)
    assert os.listdir(str(tmp_path)) == []
    assert L.swz_bin_persist_nodes_image(None, None, 0, None, None, None, None, 0, 0, 0) == ERR_BAD_ARG


def test_persist_image_slices_on_the_host(tmp_path):
    """no GPU: an image put together from written files comes back as those files, plain and compressed"""
    import schwarzwald_amd as swz
    rng = np.random.default_rng(5)
    counts = np.array([3, 0, 5, 1], np.uint64)
    n = int(counts.sum())
    xyz, cols = rng.random((n, 3)), _columns(rng, n)
    names = ("rgb", "normal", "gps_time")
    files, image, at = [], b"", 0
    for c in counts:
        f = _written_file(tmp_path, xyz, cols, names, np.arange(at, at + int(c))) if c else b""
        files.append(f)
        image += f + bytes(-len(f) % 8)
        at += int(c)
    os.remove(str(tmp_path / "want.bin"))
    nodes = dict(level=np.array([-1, 0, 0, 0], np.int8), key=np.array([0, 0, 1 << 60, 2 << 60], np.uint64), count=counts)
    for compressed in (False, True):
        out = tmp_path / ("z" if compressed else "plain")
        out.mkdir()
        swz.bin_persist_nodes_image(str(out), nodes, np.frombuffer(image, np.uint8), names, compressed)
        ext = ".binz" if compressed else ".bin"
        assert sorted(os.listdir(str(out))) == sorted(n + ext for n in ("r", "r1", "r2"))
        at = 0
        for k, name in enumerate(("r", "r0", "r1", "r2")):
            c = int(counts[k])
            if not c:
                continue
            path = str(out / (name + ext))
            if not compressed:
                assert open(path, "rb").read() == files[k]
            got_xyz, got = swz.bin_read_node(path, compressed)
            assert np.array_equal(got_xyz, xyz[at:at + c]) and sorted(got) == sorted(names)
            for a in names:
                assert np.array_equal(got[a], cols[a][at:at + c]), a
            at += c


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def source():
    import torch
    rng = np.random.default_rng(77)
    src = 2 * N
    xyz = (rng.random((src, 3)) - 0.5) * 1e6
    cols = _columns(rng, src)
    dev = torch.device("cuda:0")
    d = {"xyz": torch.from_numpy(xyz).to(dev)}
    for name, arr in cols.items():
        d[name] = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to(dev)
    torch.cuda.synchronize()
    perm = rng.permutation(src).astype(np.uint32)[:N]          # stored rows are any rows of the source
    order = rng.permutation(N).astype(np.uint32)
    return dict(xyz=xyz, cols=cols, d=d, perm=perm, order=order)


def _pack(ctx, S, off, cnt, names, with_order):
    import torch
    import schwarzwald_amd as swz
    total = swz.bin_layout(cnt, names)["total"]
    d_perm = torch.from_numpy(S["perm"].view(np.int32)).to("cuda:0")
    d_order = torch.from_numpy(S["order"].view(np.int32)).to("cuda:0") if with_order else None
    buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    attrs = {a: S["d"][a].data_ptr() for a in names}
    ctx.bin_pack_device(d_perm.data_ptr(), d_order.data_ptr() if with_order else None, N, S["d"]["xyz"].data_ptr(), attrs,
                        dict(offset=off, count=cnt), buf.data_ptr() + GUARD, total, attrs=names)
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + total:] == 0xA5), "a guard was touched"
    return got[GUARD:GUARD + total]


@pytest.mark.gpu
@pytest.mark.parametrize("with_order", [True, False])
@pytest.mark.parametrize("names", MASKS)
@pytest.mark.parametrize("table", [0, 1])
def test_gpu_pack_bodies_are_the_written_files(tmp_path, source, table, names, with_order):
    import schwarzwald_amd as swz
    S = source
    off, cnt = _tables()[table]
    rows = S["perm"][S["order"]] if with_order else S["perm"]
    lay = swz.bin_layout(cnt, names)
    with swz.Context(0) as ctx:
        image = _pack(ctx, S, off, cnt, names, with_order)
    for k in range(len(cnt)):
        c, o, at = int(cnt[k]), int(off[k]), int(lay["offset"][k])
        want = _written_file(tmp_path, S["xyz"], S["cols"], names, rows[o:o + c]) if c else b""
        assert int(lay["file_size"][k]) == len(want)
        got = image[at:at + len(want)].tobytes()
        if got != want:
            bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
            pytest.fail("mask %s, node %d (rows %d + %d): %d bytes differ, first at %d" % (names, k, o, c, len(bad), bad[0]))
        assert not image[at + len(want):at + int(lay["size"][k])].any(), "padding of node %d" % k


@pytest.mark.gpu
@pytest.mark.parametrize("compressed", [False, True])
def test_gpu_persist_nodes_image(tmp_path, source, compressed):
    import schwarzwald_amd as swz
    S = source
    names = ("rgb", "normal", "gps_time")
    off, cnt = _tables()[1]
    rows = S["perm"][S["order"]]
    m = len(cnt)
    nodes = dict(level=np.array([-1] + [0] * (m - 1), np.int8), key=np.array([0] + [(k - 1) << 60 for k in range(1, m)], np.uint64),
                 offset=off, count=cnt)
    out = tmp_path / "out"
    out.mkdir()
    with swz.Context(0) as ctx:
        image = _pack(ctx, S, off, cnt, names, True)
        ctx.bin_persist_nodes_image(str(out), nodes, image, names, compressed)
    ext = ".binz" if compressed else ".bin"
    want_names = [swz.node_name(int(nodes["level"][k]), int(nodes["key"][k])) + ext for k in range(m) if cnt[k]]
    assert sorted(os.listdir(str(out))) == sorted(want_names)
    for k in range(m):
        c, o = int(cnt[k]), int(off[k])
        if not c:
            continue
        path = str(out / (swz.node_name(int(nodes["level"][k]), int(nodes["key"][k])) + ext))
        if not compressed:
            assert open(path, "rb").read() == _written_file(tmp_path, S["xyz"], S["cols"], names, rows[o:o + c])
        got_xyz, got = swz.bin_read_node(path, compressed)
        assert np.array_equal(got_xyz, S["xyz"][rows[o:o + c]]) and sorted(got) == sorted(names)
        for a in names:
            assert np.array_equal(got[a], S["cols"][a][rows[o:o + c]]), a


@pytest.mark.gpu
def test_gpu_pack_refuses_before_anything_is_launched(source):
    import torch
    import schwarzwald_amd as swz
    S = source
    d = S["d"]
    u = lambda *v: np.array(v, np.uint64)
    good = dict(offset=u(0, 10), count=u(10, 10))
    both = {"rgb": d["rgb"].data_ptr(), "gps_time": d["gps_time"].data_ptr()}
    perm = torch.arange(N, dtype=torch.int32, device="cuda:0")
    cases = [
        ("offsets descend", dict(offset=u(10, 0), count=u(5, 5)), both, ("rgb",), N),
        ("ranges overlap", dict(offset=u(0, 5), count=u(10, 5)), both, ("rgb",), N),
        ("a range passes n", dict(offset=u(0, N - 3), count=u(10, 4)), both, ("rgb",), N),
        ("mask names absent rgb", good, {"gps_time": d["gps_time"].data_ptr()}, ("rgb",), N),
        ("mask names no columns at all", good, None, ("intensity",), N),
        ("a mask bit that does not exist", good, both, 1 << 12, N),
        ("too many rows", good, both, ("rgb",), 2 ** 32 - 65535),
    ]
    with swz.Context(0) as ctx:
        buf = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        for what, nodes, attrs, names, rows in cases:
            with pytest.raises(swz.SwzError) as e:
                ctx.bin_pack_device(perm.data_ptr(), None, rows, d["xyz"].data_ptr(), attrs, nodes, buf.data_ptr(), 1 << 16, attrs=names)
            assert e.value.code == ERR_BAD_ARG, what
        with pytest.raises(swz.SwzError):  # the image is smaller than the layout
            ctx.bin_pack_device(perm.data_ptr(), None, N, d["xyz"].data_ptr(), both, good, buf.data_ptr(), 100, attrs=("rgb",))
        with pytest.raises(swz.SwzError):  # ... or not 8-byte aligned
            ctx.bin_pack_device(perm.data_ptr(), None, N, d["xyz"].data_ptr(), both, good, buf.data_ptr() + 4, 1 << 15, attrs=("rgb",))
        with pytest.raises(swz.SwzError):  # NULL rows
            ctx.bin_pack_device(None, None, N, d["xyz"].data_ptr(), both, good, buf.data_ptr(), 1 << 16, attrs=("rgb",))
        # no nodes, and only empty ones: valid, nothing is launched
        empty = dict(offset=np.empty(0, np.uint64), count=np.empty(0, np.uint64))
        ctx.bin_pack_device(perm.data_ptr(), None, N, d["xyz"].data_ptr(), both, empty, buf.data_ptr(), 1 << 16, attrs=("rgb",))
        ctx.bin_pack_device(perm.data_ptr(), None, N, d["xyz"].data_ptr(), both, dict(offset=u(5, 9), count=u(0, 0)), buf.data_ptr(), 1 << 16,
                            attrs=("rgb",))
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), "a refused or empty call wrote into the image"
