"""Duplicate sets, the host layers: the two entry points in the header, the
binding and the library, the Engine methods, the measurement tool's model, and
the C++ mirror's shaping through its test program (tests/cpp/test_dupsets.cpp).
The GPU side is tests/test_gpu_dupsets.py."""
import ctypes
import json
import os
import re
import subprocess
import sys

from spacedrive_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
SYMBOLS = ("sdcas_duplicate_sets", "sdcas_dev_duplicate_sets")


def _bin(name):
    path = os.path.join(BUILD, name)
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "dupsets.mk"], check=True)
    return path


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    lib = ctypes.CDLL(N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sdcas_\w+)", out))
    for name in SYMBOLS:
        assert name in N.ABI_SYMBOLS
        assert re.search(r"\bint %s\(sdcas_ctx \*ctx," % name, hdr), name
        assert name in exported and getattr(lib, name) is not None
        assert getattr(N.load(), name).argtypes is not None
    assert len(N.load().sdcas_duplicate_sets.argtypes) == 10
    assert len(N.load().sdcas_dev_duplicate_sets.argtypes) == 11


def test_constants_and_counts_layout():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    for name, value in (("BY_REP", 0), ("BY_RECLAIMABLE", 1)):
        assert re.search(r"#define SDCAS_SETS_%s\s+%du\b" % (name, value), hdr), name
        assert getattr(N, "SDCAS_SETS_" + name) == value
    body = re.search(r"typedef struct sdcas_sets_counts \{(.*?)\} sdcas_sets_counts;", hdr, re.S).group(1)
    fields = re.findall(r"uint64_t (\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["files", "sets", "members", "duplicate_files", "reclaimable_bytes", "largest_set"]
    assert [f for f, _ in N.SetsCounts._fields_] == fields
    assert ctypes.sizeof(N.SetsCounts) == 48
    assert N.SetsCounts(1, 2, 3, 4, 5, 6).as_dict() == dict(zip(fields, range(1, 7)))


def test_abi_version_is_still_7():
    """new symbols alone are a compatible change: callers probe for them"""
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    assert "#define SDCAS_ABI_VERSION 7" in hdr
    assert N.SDCAS_ABI_VERSION == 7 and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("duplicate sets: members, sizes and reclaimable bytes"):]
    assert "added after abi 7; probe for the symbol" in section[:400].lower()


def test_engine_methods_exist():
    from spacedrive_amd import Engine
    for name in ("duplicate_sets", "dev_duplicate_sets", "identify_duplicate_sets"):
        assert callable(getattr(Engine, name)), name


def test_argument_checks_need_no_device():
    """a null context is refused before anything touches the GPU"""
    L = N.load()
    assert L.sdcas_duplicate_sets(None, None, None, 0, 0, None, None, None, None, None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_duplicate_sets(None, None, None, 0, 0, None, None, None, None, None, None) == N.SDCAS_E_INVALID


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_ds_count", "k_ds_head_write", "k_ds_hist", "k_ds_scatter", "k_ds_scan_apply", "k_ds_final",
              "k_ds_mem_write", "k_ds_members_out"):
        assert k in out, k


def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_sets.py"), "--count-only", "--files", "20000"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = json.loads(r.stdout.strip().splitlines()[-1])["model"]
    assert m["files"] == 20000 and m["participating"] == 20000
    assert 0 < m["sets"] <= 10000 and 2 * m["sets"] <= m["members"] <= 20000
    by_rep = m["bytes_by_rep"]
    assert by_rep["clear"] == 8 * 20000 and by_rep["count"] == 16 * 20000
    assert by_rep["out"] == 12 * m["members"] and m["member_sort_passes"] == 2
    assert m["bytes_per_file"]["by_reclaimable"] > m["bytes_per_file"]["by_rep"] > 0


def test_reclaim_report_shaping_without_gpu():
    """reclaim_report_from on hand-made arrays: the mapping of indices to
    file_path ids, the sets' order, the totals, empty input, arrays that do
    not fit together"""
    r = subprocess.run([_bin("test_dupsets")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
