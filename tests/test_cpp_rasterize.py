"""swz_host::rasterize_dataset of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp), driven by
tests/cpp/test_rasterize.cpp: a BIN data set written by TilingAlgorithmGPU::write_output (+ write_properties) is rastered on a
9 x 5 grid over a sub-box -- z of the box alone, z and intensity of an L-shaped outline with any_of(classification, {2, 9}).
The program itself compares every table with a direct call of swz_dataset_rasterize; the dumped tables must be
tests/raster_ref.py over every node file in scan order, exactly; a refusal surfaces as the adapter's exception with the
library's text."""
import os
import subprocess

import numpy as np
import pytest

import filter_ref as F
import raster_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build") / "test_rasterize")
    lib_dir = os.path.join(ROOT, "schwarzwald_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "test_rasterize.cpp"), "-o", out,
                    "-L" + lib_dir, "-lswz_gpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return out


def test_rasterize_test_compiles_against_the_abi(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_rasters_are_numpys(tmp_path, exe):
    import schwarzwald_amd as swz
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "raster ok: " in r.stdout, r.stdout
    assert "refused: swz_raster_frame_of: SWZ_ATTR_GPS_TIME is not a value the raster takes" in r.stdout, r.stdout
    assert "refused: swz_dataset_rasterize: the value is SWZ_ATTR_USER_DATA, which the source does not hold (its attribute mask is 0xc)" in r.stdout, r.stdout
    outline = np.fromfile(str(tmp_path / "outline.f64"), np.float64).reshape(6, 2)
    box = np.fromfile(str(tmp_path / "box.f64"), np.float64).reshape(2, 3)
    box = (box[0].tolist(), box[1].tolist())
    src = str(tmp_path / "bin")
    scan = swz.dataset_scan(src)
    rows = [swz.bin_read_node(os.path.join(src, swz.node_name(int(l), int(k)) + ".bin")) for l, k in zip(scan["nodes"]["level"], scan["nodes"]["key"])]
    xyz = np.concatenate([x for x, _ in rows])
    cols = {name: np.concatenate([c[name] for _, c in rows]) for name in ("intensity", "classification")}
    assert len(xyz) == 9000
    sel = F.select_mask(xyz, cols, box, ("polygon", outline), [("any_of", "classification", [2, 9])])
    assert 0 < sel.sum() < 0.5 * len(xyz)
    for name, value, keep in (("z_box", "z", None), ("z_sel", "z", sel), ("i_sel", "intensity", sel)):
        frame, table = RR.raster(box, 9, 5, xyz, value, cols["intensity"] if value == "intensity" else None, keep)
        cells = np.fromfile(str(tmp_path / (name + ".cells")), swz.RASTER_CELL_DTYPE)
        lib_frame = swz.raster_frame_of(box[0], box[1], 9, 5, value)
        got = swz.raster_finish(lib_frame, cells)
        got["sum"] = cells["sum"].reshape(5, 9)
        assert RR.same_table(got, frame, table), name
        mean = np.fromfile(str(tmp_path / (name + ".mean")), np.float64).reshape(5, 9)
        assert np.array_equal(mean, RR.finish(frame, table)["mean"], equal_nan=True), name
        assert int(table["count"].sum()) > 0, name
