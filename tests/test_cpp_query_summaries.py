"""swz_host::summarize_dataset and swz_host::query_dataset_filtered_nodes of the C++ host adapter
(schwarzwald_amd/host/swz_tiling.hpp), driven by tests/cpp/test_query_summaries.cpp: a BIN data set written by
TilingAlgorithmGPU::write_output is queried by range(intensity) and any_of(classification), summarised and queried again.  The
program itself checks that both queries return the same rows and that the second reads fewer nodes; the dumped rows must be
the filter of tests/filter_ref.py over every node file in scan order, exactly."""
import os
import subprocess

import numpy as np
import pytest

import filter_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build") / "test_query_summaries")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_query_summaries.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def test_query_summaries_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_the_same_rows_with_fewer_nodes_read(tmp_path, exe):
    import schwarzwald_amd as swz
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "summaries ok: " in r.stdout, r.stdout
    src = str(tmp_path / "bin")
    assert swz.dataset_summaries_read(src)["attrs"] == ["intensity", "classification"]
    scan = swz.dataset_scan(src)
    rows = [swz.bin_read_node(os.path.join(src, swz.node_name(int(l), int(k)) + ".bin")) for l, k in zip(scan["nodes"]["level"], scan["nodes"]["key"])]
    xyz = np.concatenate([x for x, _ in rows])
    cols = {name: np.concatenate([c[name] for _, c in rows]) for name in ("intensity", "classification")}
    assert len(xyz) == 9000
    sel = F.select_mask(xyz, cols, UNIT, None, [("range", "intensity", 10000.0, 14999.0), ("any_of", "classification", [2])])
    assert 0.01 * len(xyz) < sel.sum() < 0.2 * len(xyz)
    assert np.fromfile(str(tmp_path / "s_xyz.f64"), np.float64).tobytes() == xyz[sel].tobytes()
    assert np.fromfile(str(tmp_path / "s_intensity.u16"), np.uint16).tobytes() == cols["intensity"][sel].tobytes()
    node = np.concatenate([np.full(len(x), k) for k, (x, _) in enumerate(rows)])
    assert np.array_equal(np.fromfile(str(tmp_path / "s_nodes.u32"), np.uint32), node[sel].astype(np.uint32))
