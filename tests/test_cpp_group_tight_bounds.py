"""SWZ_OUT_TIGHT_BOUNDS on a group, driven by tests/cpp/test_group_tight_bounds.cpp: a thin, tilted sheet tiled on eight shards
(all on device 0) and on a single tiler fed the same batches in the same process.  With the flag, the 3DTILES, ENTWINE_LAS and
LAS directories swz_group_write_output writes must be the single tiler's -- the same relative paths, every file byte for byte,
tileset JSON, LAS headers and ept.json included --, and swz_group_node_boxes must equal swz_tiler_node_boxes node by node
(the program checks that, the alignment of the two tables, and that the root's box is the min / max of the shards' parts).

This has never run on more than one device: every shard of the group lies on device 0."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the program, built once"""
    out = str(tmp_path_factory.mktemp("build") / "test_group_tight_bounds")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_group_tight_bounds.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def _tree(top):
    out = {}
    for base, _, files in os.walk(top):
        for f in files:
            path = os.path.join(base, f)
            out[os.path.relpath(path, top)] = path
    return out


def test_group_tight_bounds_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_group_output_with_tight_bounds_is_the_single_tilers(tmp_path, exe):
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work), "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    pairs = [line.split()[1:] for line in r.stdout.splitlines() if line.startswith("pair ")]
    assert len(pairs) == PAIRS and "pairs %d" % PAIRS in r.stdout and "boxes " in r.stdout, r.stdout
    assert not (work / "refused").exists()
    for want_dir, got_dir in pairs:
        want, got = _tree(want_dir), _tree(got_dir)
        assert sorted(got) == sorted(want), (got_dir, sorted(set(got) ^ set(want))[:10])
        assert len(want) >= 50
        for rel in sorted(want):
            with open(want[rel], "rb") as a, open(got[rel], "rb") as b:
                assert a.read() == b.read(), (got_dir, rel)
    # the flag reached the metadata: the root tile is written with half-axes of a sheet, not the unit cube's extent
    root = json.loads((work / "group_3dtiles" / "r.json").read_text())["root"]["boundingVolume"]["box"]
    assert root[11] < 0.4 and root[3] < 0.51 and abs(root[0] - 1001.0) < 0.01
    ept = json.loads((work / "group_ept" / "ept.json").read_text())
    assert ept["bounds"] == [0, 0, 0, 1, 1, 1] and ept["boundsConforming"][2] > 0.2 and ept["boundsConforming"][5] < 0.95
