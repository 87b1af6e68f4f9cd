"""The family bytes, the host layers: the entry points in the header, the
binding and the library, the GPU-free plan and its ranges, the Python methods
and the tool's model. The kernels' tests are tests/test_gpu_family_bytes.py and
tests/test_gpu_similar_family_bytes.py."""
import ctypes
import importlib.util
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from spacedrive_amd import _native as N
from tests import _family_bytes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_family_bytes_plan": 3, "sdcas_family_bytes": 16, "sdcas_dev_family_bytes": 17}
KERNELS = ("k_fb_insert", "k_fb_classify", "k_fb_rows", "k_fb_heads", "k_fb_merge", "k_fb_write", "k_fb_totals")


def plan(m, n):
    ws = ctypes.c_uint64(0)
    rc = N.load().sdcas_family_bytes_plan(m, n, ctypes.byref(ws))
    return rc, ws.value


def load_tool():
    spec = importlib.util.spec_from_file_location("ab_family_bytes", os.path.join(ROOT, "tools", "ab_family_bytes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sdcas_\w+)", out))
    for name, nargs in SYMBOLS.items():
        assert name in N.ABI_SYMBOLS and name in exported, name
        assert len(getattr(N.load(), name).argtypes) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
    assert "#define SDCAS_ABI_VERSION 7" in hdr and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("family bytes: what a family's versions store and give back"):]
    assert "added after abi 7; probe for the symbol (sdcas_abi_version stays 7)" in section[:300].lower()
    fields = re.findall(r"uint64_t (\w+);", section[section.index("typedef struct sdcas_family_bytes_counts"):
                                                    section.index("} sdcas_family_bytes_counts;")])
    assert fields == list(R.COUNTS) == [name for name, _ in N.FamilyBytesCounts._fields_]
    assert fields == ["files", "chunks", "classes", "total_bytes", "stored_bytes", "sets", "members",
                      "set_reclaimable_bytes", "largest_reclaimable"]
    assert ctypes.sizeof(N.FamilyBytesCounts) == 72


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in KERNELS:
        assert k in out, k


def test_plan_ranges_and_bytes():
    assert plan(1 << 30, 1 << 30)[0] == N.SDCAS_OK
    assert plan((1 << 30) + 1, 4)[0] == N.SDCAS_E_CAPACITY
    assert plan(4, (1 << 30) + 1)[0] == N.SDCAS_E_CAPACITY
    assert plan(0, 0)[0] == N.SDCAS_OK
    assert N.load().sdcas_family_bytes_plan(5, 1, None) == N.SDCAS_OK  # a NULL output is taken
    sizes = (0, 1, 2, 255, 256, 257, 65536, 70000, 1 << 20, (1 << 24) + 1, 1 << 30)
    last = 0
    for m in sizes:  # monotone in m: a table of at least 2 m u32 slots and 4 bytes per chunk
        rc, ws = plan(m, 1000)
        assert rc == N.SDCAS_OK and ws >= last and ws >= 12 * m and ws <= 20 * m + 65 * 1000 + 4096, m
        last = ws
    last = 0
    for n in sizes:  # monotone in n_files: 65 bytes per row
        rc, ws = plan(1000, n)
        assert rc == N.SDCAS_OK and ws >= last and ws >= 65 * n and ws <= 65 * n + 20 * 1000 + 4096, n
        last = ws


def test_a_null_context_is_refused_without_a_device():
    L = N.load()
    assert L.sdcas_family_bytes(None, None, None, None, 0, None, 0, *([None] * 9)) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_family_bytes(None, None, None, None, 0, None, 0, *([None] * 10)) == N.SDCAS_E_INVALID


def test_engine_agrees_with_the_plan_and_the_methods_exist():
    from spacedrive_amd import Engine
    for m, n in ((0, 0), (1, 1), (12345, 77), (1 << 30, 1 << 30)):
        assert Engine.family_bytes_plan(m, n) == plan(m, n)[1]
    for bad in (((1 << 30) + 1, 4), (4, (1 << 30) + 1)):
        with pytest.raises(N.SdcasError) as ei:
            Engine.family_bytes_plan(*bad)
        assert ei.value.code == N.SDCAS_E_CAPACITY
    for name in ("family_bytes_plan", "family_bytes", "dev_family_bytes", "family_bytes_of", "similar_families"):
        assert callable(getattr(Engine, name)), name
    sig = inspect.signature(Engine.family_bytes).parameters
    assert list(sig) == ["self", "chunk_file", "chunk_len", "rep", "family", "sets"] and sig["sets"].default is False
    sig = inspect.signature(Engine.dev_family_bytes).parameters
    assert list(sig) == ["self", "chunk_file", "chunk_len", "rep", "m", "family", "n_files", "file_bytes", "delta_bytes",
                         "self_bytes", "inherited_bytes", "set_rep", "set_files", "set_total", "set_stored", "counts",
                         "stream"]
    assert all(sig[name].default == 0 for name in list(sig)[7:])
    sig = inspect.signature(Engine.family_bytes_of).parameters
    assert list(sig) == ["self", "results", "file_ids", "num", "den"] and (sig["num"].default, sig["den"].default) == (1, 2)
    sig = inspect.signature(Engine.similar_families).parameters
    assert list(sig) == ["self", "paths", "k", "max_holders", "num", "den", "params", "window_bytes"]
    assert [sig[name].default for name in list(sig)[2:]] == [4, 64, 1, 2, None, 256 << 20]
    # families_of's signature stays; similar_files_indexed gains a trailing keyword
    sig = inspect.signature(Engine.families_of).parameters
    assert list(sig) == ["self", "results", "file_ids", "num", "den"] and (sig["num"].default, sig["den"].default) == (1, 2)
    sig = inspect.signature(Engine.similar_files_indexed).parameters
    assert list(sig) == ["self", "paths", "file_ids", "index", "params", "window_bytes", "peers", "max_holders", "chunks"]
    assert sig["chunks"].default is False


def test_makefile_and_documents_name_the_feature():
    mk = open(os.path.join(ROOT, "spacedrive_amd", "csrc", "Makefile")).read()
    assert "family_bytes.hip" in mk
    assert "ab_family_bytes.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "tools/ab_family_bytes.py" in readme and "family_bytes.hip" in readme and "similar_families" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.11" in design and all(k in design for k in KERNELS)


def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_family_bytes.py"), "--count-only"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    models = json.loads(lines[0])["model"]
    assert [c["m"] for c in models] == [1 << 20, 1 << 22]
    for c in models:
        m, n = c["m"], c["m"] // 64
        assert c["n_files"] == n and c["workspace_bytes"] == plan(m, n)[1]
        assert c["table_slots"] == 2 * m and c["workspace_bytes"] >= 4 * c["table_slots"] + 4 * m + 65 * n
        assert c["merge_launches"] == (n - 1).bit_length() and c["launches"] == 6 + c["merge_launches"]
        assert c["bytes_in"] == m * 20 + n * 8 and c["bytes_out"] == n * 32 + (n // 2) * 28 + 72


def test_the_tools_reference_is_the_tests_reference():
    """the numpy reference the tool checks the device against, on its own three corpora at small sizes"""
    tool = load_tool()
    for kind in tool.KINDS:
        for m in (1, 64, 130, 64 * 40 + 5):
            g = tool.corpus(kind, m)
            got, want = tool.reference(*g), R.family_bytes(*g)
            for name in R.ROWS + R.SETS:
                assert np.array_equal(got[name], want[name]) and got[name].dtype == want[name].dtype, (kind, m, name)
            assert got["counts"] == want["counts"], (kind, m)
    # and on inputs with rows, chunks and reps outside their ranges, zero and wrapping lengths
    rng = np.random.default_rng(5)
    for _ in range(30):
        m, n = int(rng.integers(0, 50)), int(rng.integers(1, 9))
        g = (rng.integers(0, n + 2, m).astype(np.uint32), rng.choice(np.array([0, 3, 1 << 63], np.uint64), m),
             rng.integers(-2, m + 2, m).astype(np.int64), rng.integers(-1, n + 1, n).astype(np.int64))
        got, want = tool.reference(*g), R.family_bytes(*g)
        for name in R.ROWS + R.SETS:
            assert np.array_equal(got[name], want[name]), name
        assert got["counts"] == want["counts"]
    c = tool.reference(*tool.corpus("random", 1 << 14))["counts"]
    assert c["sets"] > 10 and c["chunks"] == 1 << 14 and c["chunks"] // 4 < c["classes"] < 3 * c["chunks"] // 4
    c = tool.reference(*tool.corpus("one_class", 1 << 12))["counts"]
    assert c["classes"] == 1 and c["sets"] == 1 and c["members"] == 64
    c = tool.reference(*tool.corpus("one_file", 1 << 12))["counts"]
    assert c["classes"] == 1 << 12 and c["stored_bytes"] == c["total_bytes"] and c["set_reclaimable_bytes"] == 0
