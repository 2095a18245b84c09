"""swz_host::query_dataset_filtered and swz_host::Filter of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp), driven
by tests/cpp/test_query_filter.cpp: a BIN data set written by TilingAlgorithmGPU::write_output (+ write_properties) is queried
by an L-shaped outline with any_of(classification, {2, 9}) and range(intensity, 1000, 40000.5); the dumped rows must be the
filter of tests/filter_ref.py over every node file in scan order, exactly; a refusal surfaces as the adapter's exception with
the library's text."""
import os
import subprocess

import numpy as np
import pytest

import filter_ref as F
import region_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build") / "test_query_filter")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_query_filter.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def test_query_filter_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_filtered_outline_is_numpys(tmp_path, exe):
    import schwarzwald_amd as swz
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "filtered query ok: " in r.stdout, r.stdout
    assert "refused: swz_filter_check: clause 1: a SET on SWZ_ATTR_INTENSITY, a column wider than a byte" in r.stdout, r.stdout
    assert "refused: swz_dataset_query_filtered: the filter names SWZ_ATTR_GPS_TIME, which the source does not hold" in r.stdout, r.stdout
    outline = np.fromfile(str(tmp_path / "outline.f64"), np.float64).reshape(6, 2)
    src = str(tmp_path / "bin")
    scan = swz.dataset_scan(src)
    rows = [swz.bin_read_node(os.path.join(src, swz.node_name(int(l), int(k)) + ".bin")) for l, k in zip(scan["nodes"]["level"], scan["nodes"]["key"])]
    xyz = np.concatenate([x for x, _ in rows])
    cols = {name: np.concatenate([c[name] for _, c in rows]) for name in ("intensity", "classification")}
    assert len(xyz) == 9000
    region = ("polygon", outline)
    sel = F.select_mask(xyz, cols, UNIT, region, [("any_of", "classification", [2, 9]), ("range", "intensity", 1000.0, 40000.5)])
    assert 0.05 * R.region_mask(xyz, UNIT, region).sum() < sel.sum() < 0.5 * R.region_mask(xyz, UNIT, region).sum()
    assert np.fromfile(str(tmp_path / "f_xyz.f64"), np.float64).tobytes() == xyz[sel].tobytes()
    assert np.fromfile(str(tmp_path / "f_intensity.u16"), np.uint16).tobytes() == cols["intensity"][sel].tobytes()
    kept = swz.dataset_query_region_nodes(src, UNIT[0], UNIT[1], R.as_region(swz, region))
    index = {(int(l), int(k)): i for i, (l, k) in enumerate(zip(kept["level"], kept["key"]))}
    node = np.concatenate([np.full(len(x), index.get((int(l), int(k)), -1)) for (x, _), l, k in zip(rows, scan["nodes"]["level"], scan["nodes"]["key"])])
    assert np.array_equal(np.fromfile(str(tmp_path / "f_nodes.u32"), np.uint32), node[sel].astype(np.uint32))
