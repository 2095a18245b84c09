"""swz_group_set_source_srs, driven by tests/cpp/test_group_srs.cpp: two LAS files in UTM 32N (formats 3 and 7, one 600 m tile
with 40 m of relief, 20 000 points, batches of 9 000 so that one spans the file boundary) are read with the projection by a
group of 2 shards (both on device 0) and by a single tiler (swz_tiler_set_source_srs: tiler A, the yardstick), shifted to the
centre of the data set's ECEF box; after finalize both data sets are written as BIN and must be the same directory, byte for
byte: the merged node table and every stored position.  The files hold no two points in one Morton cell of the root box
(asserted here from the host map), so the order inside every node file is defined by the keys alone.  The refusals -- a set
before the open and after the first batch, the source CRS's box -- run in the program."""
import os
import subprocess

import numpy as np
import pytest

from las_input_util import LasTile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTM32 = "+proj=utm +zone=32 +datum=WGS84"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    out = str(tmp_path_factory.mktemp("build") / "test_group_srs")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_group_srs.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    import schwarzwald_amd as swz
    top = tmp_path_factory.mktemp("las")
    rng = np.random.default_rng(31)
    kw = dict(scale=(1e-3, 1.1e-3, 40.0 / 600000), offset=(499700.0, 1105000.0, 250.0), lo=0, hi=600000)
    tiles = [LasTile(rng, 12000, 3, **kw), LasTile(rng, 8000, 7, extra=1, **kw)]
    paths = [t.write(top / ("tile%d.las" % i)) for i, t in enumerate(tiles)]
    # no two points share a Morton cell of the root box once projected and shifted to the centre (float32)
    _, ds = swz.las_scan_files(paths, srs=UTM32)
    xyz = np.concatenate([np.stack([t.records[ax].astype(np.float64) * t.scale[k] + t.offset[k] for k, ax in enumerate("XYZ")], axis=1)
                          for t in tiles])
    pos = (swz.srs_transform(UTM32, xyz) - ds["center"]).astype(np.float32).astype(np.float64)
    lo, hi = ds["origin"]
    cells = np.clip(np.floor((pos - lo) * (2.0 ** 21 / (hi - lo))), 0, 2 ** 21 - 1).astype(np.int64)
    assert len(np.unique(cells, axis=0)) == len(cells)
    return paths


def _tree(top):
    out = {}
    for base, _, files in os.walk(top):
        for f in files:
            path = os.path.join(base, f)
            out[os.path.relpath(path, top)] = path
    return out


def test_group_srs_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,refusals", [("abi", 3), ("adapter", 1)])
def test_group_with_a_projection_gives_the_single_tilers_data_set(tmp_path, exe, dataset, mode, refusals):
    r = subprocess.run([exe, str(tmp_path), "2", mode, UTM32] + dataset, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    pairs = [line.split()[1:] for line in r.stdout.splitlines() if line.startswith("pair ")]
    assert len(pairs) == 1 and r.stdout.count("refused: ") == refusals, r.stdout
    want, got = _tree(pairs[0][0]), _tree(pairs[0][1])
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))[:10]
    assert len(want) > 20  # a real tree, not a root alone
    for rel in sorted(want):
        with open(want[rel], "rb") as a, open(got[rel], "rb") as b:
            assert a.read() == b.read(), rel
