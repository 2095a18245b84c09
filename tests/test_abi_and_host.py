"""CPU-side checks (no GPU): the C-ABI library builds, loads and exports every symbol that include/swz_gpu.h
declares; it refuses to work without a device instead of falling back to the CPU; host-side bookkeeping
(node lists) that needs no device behaves; the product never reaches into oracle/."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-C", os.path.join(ROOT, "schwarzwald_amd", "csrc"), "-j", "4", "-s"], check=True)
    import schwarzwald_amd as swz
    return swz.load_library()


def test_library_exports_every_declared_symbol(lib):
    header = open(os.path.join(ROOT, "include", "swz_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(swz_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 20
    for name in sorted(declared):
        assert hasattr(lib, name), "libswz_gpu.so does not export %s" % name
    import schwarzwald_amd.api as api
    assert lib.swz_abi_version() == 3 == api.ABI_VERSION


def test_no_cpu_fallback_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import schwarzwald_amd as swz
    with pytest.raises(swz.SwzError) as e:
        swz.Context(0)
    assert "no CPU fallback" in str(e.value)


def test_product_does_not_use_the_oracle():
    pkg = os.path.join(ROOT, "schwarzwald_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".inc", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in text.lower() or f == "jitter_tables.inc", os.path.join(dirpath, f)


def test_jitter_tables_are_identical_in_product_and_checker():
    a = open(os.path.join(ROOT, "schwarzwald_amd", "csrc", "jitter_tables.inc")).read()
    b = open(os.path.join(ROOT, "oracle", "jitter_tables.inc")).read()
    assert a == b
    nums = [int(x) for x in re.findall(r"\b\d+\b", a.split("SWZ_JITTER_TABLE(64)")[1])]
    assert len(nums) == 16 * 64
    for r in range(16):
        assert sorted(nums[r * 64:(r + 1) * 64]) == list(range(1, 65))


def test_makefile_lists_every_source_and_header():
    """bench.py's source hash globs csrc/ while the build reads the Makefile's lists: a .hip missing from SRCS is not
    compiled (at best the link fails), a header missing from HDRS silently drops out of the rebuild dependencies."""
    csrc = os.path.join(ROOT, "schwarzwald_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()

    def listed(var):
        m = re.search(r"^%s\s*:=\s*(.*)$" % var, make, flags=re.M)
        assert m, "the Makefile sets no %s" % var
        return sorted(m.group(1).split())

    on_disk = sorted(os.listdir(csrc))
    assert listed("SRCS") == [f for f in on_disk if f.endswith(".hip")]
    assert len(listed("SRCS")) >= 10
    headers = [f for f in on_disk if f.endswith((".h", ".inc"))]
    assert sorted(h for h in listed("HDRS") if "/" not in h) == headers
    assert "../../include/swz_gpu.h" in listed("HDRS")


def test_spacing_from_diagonal_matches_reference_value():
    import schwarzwald_amd as swz
    s = swz.spacing_from_diagonal([0, 0, 0], [1, 1, 1], 250)
    assert np.float32(s).view(np.uint32) == 0x3BE305FB


# SWZ_* names only Python reads (bench.py, the suite, the sharded driver): they never reach the library
PYTHON_ONLY_OPTIONS = ("SWZ_SHARD_JOINT_ROOT", "SWZ_GPU_LIBRARY", "SWZ_TEST_QUEUE_TIMEOUT")
PYTHON_ONLY_PREFIXES = ("SWZ_BENCH_", "SWZ_FULLSIZE_")


def _options_read_by_the_library():
    csrc = os.path.join(ROOT, "schwarzwald_amd", "csrc")
    names = set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            names |= set(re.findall(r'\bopt(?:_int|_num|_on)?\("(SWZ_\w+)"', open(os.path.join(csrc, f)).read()))
    return names


def _unknown_options(text, known):
    """SWZ_* names that `text` sets -- quoted (set_option / setenv arguments, keys of option or environment dicts) or
    assigned on a command line (NAME=value) -- and the library does not read."""
    named = set(re.findall(r"[\"'](SWZ_\w+)[\"']", text)) | set(re.findall(r"\b(SWZ_\w+)=(?!=)", text))
    return sorted(n for n in named
                  if n not in known and n not in PYTHON_ONLY_OPTIONS and not n.startswith(PYTHON_ONLY_PREFIXES))


def test_tests_and_tools_set_only_options_the_library_reads():
    """swz_set_option accepts any name: a test mode that sets a switch the library no longer reads would pass without
    testing anything."""
    known = _options_read_by_the_library()
    assert len(known) > 50
    bad = {}
    for sub in ("tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith((".py", ".sh", ".txt", ".cpp", ".hip", ".h")):
                    path = os.path.join(dirpath, f)
                    unknown = _unknown_options(open(path, errors="ignore").read(), known)
                    if unknown:
                        bad[os.path.relpath(path, ROOT)] = unknown
    assert not bad, bad
    # ... and a mode that still sets a switch the library has dropped is caught, in every form
    gone = "_".join(["SWZ", "MD", "PERSISTENT"])  # (spelt out it would be one of the names this test finds)
    assert _unknown_options('{"SWZ_MD_LAZY": "0", "%s": "1"}' % gone, known) == [gone]
    assert _unknown_options('ctx.set_option("%s", "1")' % gone, known) == [gone]
    assert _unknown_options("SWZ_DEBUG=1 %s=1 python bench.py" % gone, known) == [gone]


def test_every_option_the_library_reads_is_documented():
    header = open(os.path.join(ROOT, "include", "swz_gpu.h")).read()
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int swz_set_option\(", header, re.S).group(1)
    missing = sorted(n for n in _options_read_by_the_library() if not re.search(r"\b%s\b" % n, doc))
    assert not missing, "not described at swz_set_option in include/swz_gpu.h: %s" % missing
