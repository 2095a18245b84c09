"""swz_host::query_dataset of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp), driven by tests/cpp/test_query.cpp: a
BIN data set written by TilingAlgorithmGPU::write_output (+ write_properties) is queried by an octant; the dumped rows must be
numpy's filter over every node file in scan order, exactly; a refusal surfaces as the adapter's exception with the library's
text."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build") / "test_query")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_query.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def test_query_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_queried_octant_is_numpys(tmp_path, exe):
    import schwarzwald_amd as swz
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "query ok: " in r.stdout and "refused: swz_dataset_query_nodes: box_min > box_max" in r.stdout, r.stdout
    src = str(tmp_path / "bin")
    scan = swz.dataset_scan(src)
    rows = [swz.bin_read_node(os.path.join(src, swz.node_name(int(l), int(k)) + ".bin")) for l, k in zip(scan["nodes"]["level"], scan["nodes"]["key"])]
    xyz = np.concatenate([x for x, _ in rows])
    sel = ((xyz >= 0.0) & (xyz <= 0.5)).all(axis=1)
    assert 500 < sel.sum() < len(xyz) == 9000
    assert np.fromfile(str(tmp_path / "xyz.f64"), np.float64).tobytes() == xyz[sel].tobytes()
    assert np.fromfile(str(tmp_path / "intensity.u16"), np.uint16).tobytes() == np.concatenate([c["intensity"] for _, c in rows])[sel].tobytes()
    assert np.fromfile(str(tmp_path / "gps.f64"), np.float64).tobytes() == np.concatenate([c["gps_time"] for _, c in rows])[sel].tobytes()
    kept = swz.dataset_query_nodes(src, [0, 0, 0], [0.5, 0.5, 0.5])
    index = {(int(l), int(k)): i for i, (l, k) in enumerate(zip(kept["level"], kept["key"]))}
    node = np.concatenate([np.full(len(x), index.get((int(l), int(k)), -1)) for (x, _), l, k in zip(rows, scan["nodes"]["level"], scan["nodes"]["key"])])
    assert np.array_equal(np.fromfile(str(tmp_path / "nodes.u32"), np.uint32), node[sel].astype(np.uint32))
