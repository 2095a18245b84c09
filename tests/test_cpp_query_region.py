"""swz_host::query_dataset_region and swz_host::frustum_planes of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp),
driven by tests/cpp/test_query_region.cpp: a BIN data set written by TilingAlgorithmGPU::write_output (+ write_properties) is
queried by an L-shaped outline and by the frustum of a fixed camera; the dumped rows must be the filter of tests/region_ref.py
over every node file in scan order, exactly; the helper's planes must be numpy's; a refusal surfaces as the adapter's
exception with the library's text."""
import os
import subprocess

import numpy as np
import pytest

import region_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build") / "test_query_region")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_query_region.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def test_query_region_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_queried_outline_and_frustum_are_numpys(tmp_path, exe):
    import schwarzwald_amd as swz
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "region query ok: " in r.stdout, r.stdout
    assert "refused: swz_dataset_query_region_nodes: a polygon region holds 3 to 1024 vertices" in r.stdout, r.stdout
    # the helper against numpy: the same planes to rounding, and the doubles it returned are what the query took
    matrix = np.fromfile(str(tmp_path / "matrix.f64"), np.float64).reshape(4, 4)
    planes = np.fromfile(str(tmp_path / "planes.f64"), np.float64).reshape(6, 4)
    assert np.allclose(planes, swz.frustum_planes(matrix), rtol=1e-14, atol=0)
    outline = np.fromfile(str(tmp_path / "outline.f64"), np.float64).reshape(6, 2)
    src = str(tmp_path / "bin")
    scan = swz.dataset_scan(src)
    rows = [swz.bin_read_node(os.path.join(src, swz.node_name(int(l), int(k)) + ".bin")) for l, k in zip(scan["nodes"]["level"], scan["nodes"]["key"])]
    xyz = np.concatenate([x for x, _ in rows])
    intensity = np.concatenate([c["intensity"] for _, c in rows])
    assert len(xyz) == 9000
    for stem, region in (("l", ("polygon", outline)), ("frustum", ("planes", planes))):
        sel = R.region_mask(xyz, UNIT, region)
        assert 500 < sel.sum() < len(xyz)
        assert np.fromfile(str(tmp_path / (stem + "_xyz.f64")), np.float64).tobytes() == xyz[sel].tobytes(), stem
        assert np.fromfile(str(tmp_path / (stem + "_intensity.u16")), np.uint16).tobytes() == intensity[sel].tobytes(), stem
        kept = swz.dataset_query_region_nodes(src, UNIT[0], UNIT[1], R.as_region(swz, region))
        index = {(int(l), int(k)): i for i, (l, k) in enumerate(zip(kept["level"], kept["key"]))}
        node = np.concatenate([np.full(len(x), index.get((int(l), int(k)), -1)) for (x, _), l, k in zip(rows, scan["nodes"]["level"], scan["nodes"]["key"])])
        assert np.array_equal(np.fromfile(str(tmp_path / (stem + "_nodes.u32")), np.uint32), node[sel].astype(np.uint32)), stem
