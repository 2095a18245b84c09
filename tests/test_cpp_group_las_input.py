"""swz_group_add_las_files, driven by tests/cpp/test_group_las_input.cpp: six LAS files (formats 1, 3 and 7, so the common
mask loses rgb -- and gps_time, which format 7 does not report --, different scales and UTM-sized offsets, an odd record
length from extra bytes, a file of one point, an empty file) are read by a group of 2 or 8 shards (all on device 0) in one
call and by a single tiler in one call (swz_tiler_add_las_files: the yardstick); after finalize both data sets are written
as LAS and as BIN and must be the same directories, byte for byte.  batch_points 9 000: batches span files, slices start
in the middle of a file.  The files hold no two points with equal Morton keys (asserted here from the records), so the
order inside every node file is defined by the keys alone.  The refusals run in the program's mode "acc".  Mode "tail" cuts
batches of 13 333 points, which leaves a last batch of 3 points for 8 shards (most shards read, copy and decode nothing of a
batch that is not empty); mode "one" reads the whole data set as one batch (one raw image per shard)."""
import os
import subprocess

import numpy as np
import pytest

from las_input_util import LasTile, make_cubic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTM = (412345.678, 5401234.321, 287.125)
CASES = [(2, "acc"), (8, "acc"), (2, "fast"), (8, "fast"), (8, "shift"), (8, "tail"), (8, "one")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build") / "test_group_las_input")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_group_las_input.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def _tiles():
    rng = np.random.default_rng(23)
    off = lambda dx, dy, dz: (UTM[0] + dx, UTM[1] + dy, UTM[2] + dz)
    return [LasTile(rng, 15000, 1, scale=(1e-3, 1e-3, 1e-3), offset=off(0, 0, 0), lo=0, hi=1000000),
            LasTile(rng, 9000, 3, scale=(0.01, 0.01, 0.01), offset=off(100.5, 50.25, 10.125), lo=0, hi=80000),
            LasTile(rng, 1, 1, scale=(1e-3, 1e-3, 1e-3), offset=off(3, 4, 5), lo=1000, hi=2000),
            LasTile(rng, 0, 3, scale=(1e-3, 1e-3, 1e-3), offset=off(0, 0, 0), lo=0, hi=1000),
            LasTile(rng, 9000, 7, extra=3, scale=(1e-3, 1e-3, 0.005), offset=off(-20.75, 10, 0), lo=0, hi=900000),   # 39-byte records
            LasTile(rng, 7001, 3, extra=1, scale=(2e-3, 2e-3, 2e-3), offset=off(0, 0, 0), lo=200000, hi=210000)]    # a dense clump


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    top = tmp_path_factory.mktemp("las")
    tiles = _tiles()
    paths = [t.write(top / ("tile%d.las" % i)) for i, t in enumerate(tiles)]
    assert sum(t.n for t in tiles) == 40002 and tiles[4].record_bytes % 2 == 1 and tiles[5].record_bytes % 2 == 1
    # a LAZ-flagged copy of the first file
    data = bytearray(open(paths[0], "rb").read())
    data[104] |= 0x80
    laz = str(top / "flagged.las")
    with open(laz, "wb") as f:
        f.write(bytes(data))
    # no two points share a Morton cell of the root box, as read and as shifted to the centre (float32)
    xyz = np.concatenate([np.stack([t.records[ax].astype(np.float64) * t.scale[k] + t.offset[k] for k, ax in enumerate("XYZ")], axis=1)
                          for t in tiles])
    tmin = np.min([t.bmin for t in tiles], axis=0)
    tmax = np.max([t.bmax for t in tiles], axis=0)
    (cmin, cmax), (omin, omax), center = make_cubic(tmin, tmax)
    for pos, lo, hi in ((xyz, cmin, cmax), ((xyz - center).astype(np.float32).astype(np.float64), omin, omax)):
        cells = np.minimum(np.floor((pos - lo) * (2.0 ** 21 / (hi - lo))), 2 ** 21 - 1).astype(np.int64)
        assert len(np.unique(cells, axis=0)) == len(cells)
    return laz, paths


def _tree(top):
    out = {}
    for base, _, files in os.walk(top):
        for f in files:
            path = os.path.join(base, f)
            out[os.path.relpath(path, top)] = path
    return out


def test_group_las_input_test_compiles_against_the_abi(exe):
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    assert os.path.exists(exe)


@pytest.mark.gpu
@pytest.mark.parametrize("shards,mode", CASES)
def test_group_las_input_gives_the_single_tilers_data_set(tmp_path, exe, dataset, shards, mode):
    laz, paths = dataset
    r = subprocess.run([exe, str(tmp_path), str(shards), mode, laz] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    pairs = [line.split()[1:] for line in r.stdout.splitlines() if line.startswith("pair ")]
    assert len(pairs) == 2 and "pairs 2" in r.stdout, r.stdout
    assert r.stdout.count("refused: ") == (3 if mode == "acc" else 0), r.stdout
    for want_dir, got_dir in pairs:
        want, got = _tree(want_dir), _tree(got_dir)
        assert sorted(got) == sorted(want), (got_dir, sorted(set(got) ^ set(want))[:10])
        assert len(want) > 50  # a real tree, not a root alone
        for rel in sorted(want):
            with open(want[rel], "rb") as a, open(got[rel], "rb") as b:
                assert a.read() == b.read(), (got_dir, rel)
