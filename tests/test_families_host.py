"""The file families, the host layers: the entry points in the header, the
binding and the library, the GPU-free plan and its ranges, the Python methods
and the tool's model. The kernels' tests are tests/test_gpu_file_families.py and
tests/test_gpu_similar_families.py."""
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
from tests import _families_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_file_families_plan": 3, "sdcas_file_families": 13, "sdcas_dev_file_families": 14}
KERNELS = ("k_ff_init", "k_ff_union", "k_ff_jump", "k_ff_sizes", "k_ff_write")


def plan(n, k):
    ws = ctypes.c_uint64(0)
    rc = N.load().sdcas_file_families_plan(n, k, ctypes.byref(ws))
    return rc, ws.value


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
    section = hdr[hdr.index("file families: the files that are versions of one another"):]
    assert "added after abi 7; probe for the symbol (sdcas_abi_version stays 7)" in section[:300].lower()
    assert "sdcas_families_counts" in section
    fields = re.findall(r"uint64_t (\w+);", section[section.index("typedef struct sdcas_families_counts"):
                                                    section.index("} sdcas_families_counts;")])
    assert fields == list(F.COUNTS) == [name for name, _ in N.FamiliesCounts._fields_]
    assert fields == ["files", "slots", "missing", "self_slots", "weak", "links", "families", "members", "largest",
                      "unsorted"]
    assert ctypes.sizeof(N.FamiliesCounts) == 80


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in KERNELS:
        assert k in out, k


def test_plan_ranges_and_bytes():
    for k in (0, 65):
        assert plan(10, k)[0] == N.SDCAS_E_INVALID
    assert plan(10, 1)[0] == plan(10, 64)[0] == N.SDCAS_OK
    assert plan(1 << 30, 4)[0] == N.SDCAS_OK
    assert plan((1 << 30) + 1, 4)[0] == N.SDCAS_E_CAPACITY
    assert N.load().sdcas_file_families_plan(5, 1, None) == N.SDCAS_OK  # a NULL output is taken
    last = 0
    for n in (0, 1, 2, 255, 256, 257, 65536, 70000, 1 << 20, (1 << 24) + 1, 1 << 30):
        rc, ws = plan(n, 4)
        assert rc == N.SDCAS_OK and ws >= 8 * n and ws >= last and ws <= 8 * n + 4096, n
        last = ws
    assert plan(1000, 1)[1] == plan(1000, 64)[1]  # the workspace does not depend on k


def test_a_null_context_is_refused_without_a_device():
    L = N.load()
    assert L.sdcas_file_families(*([None] * 6), 0, 4, 1, 2, None, None, None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_file_families(*([None] * 6), 0, 4, 1, 2, None, None, None, None) == N.SDCAS_E_INVALID


def test_engine_agrees_with_the_plan_and_the_methods_exist():
    from spacedrive_amd import Engine
    for n in (0, 1, 12345, 1 << 30):
        assert Engine.file_families_plan(n, 4) == plan(n, 4)[1]
    for bad, code in (((1, 0), N.SDCAS_E_INVALID), ((1, 65), N.SDCAS_E_INVALID), (((1 << 30) + 1, 4), N.SDCAS_E_CAPACITY)):
        with pytest.raises(N.SdcasError) as ei:
            Engine.file_families_plan(*bad)
        assert ei.value.code == code
    for name in ("file_families_plan", "file_families", "dev_file_families", "families_of"):
        assert callable(getattr(Engine, name)), name
    sig = inspect.signature(Engine.file_families).parameters
    assert list(sig) == ["self", "ids", "sizes", "peer_count", "peers", "peer_bytes", "num", "den", "sets"]
    assert (sig["num"].default, sig["den"].default, sig["sets"].default) == (1, 2, False)
    sig = inspect.signature(Engine.families_of).parameters
    assert list(sig) == ["self", "results", "file_ids", "num", "den"] and (sig["num"].default, sig["den"].default) == (1, 2)
    sig = inspect.signature(Engine.dev_file_families).parameters
    assert list(sig)[:8] == ["self", "ids", "sizes", "peer_count", "peers", "peer_bytes", "n", "k"]


def test_makefile_and_documents_name_the_feature():
    mk = open(os.path.join(ROOT, "spacedrive_amd", "csrc", "Makefile")).read()
    assert "families.hip" in mk
    assert "ab_families.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "tools/ab_families.py" in readme and "families.hip" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.10" in design and "k_ff_union" in design


def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_families.py"), "--count-only"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    models = json.loads(lines[0])["model"]
    assert [c["n"] for c in models] == [1 << 20, 1 << 22]
    for c in models:
        assert c["k"] == 4 and c["workspace_bytes"] == plan(c["n"], 4)[1]
        assert c["jump_launches"] == (c["n"] - 1).bit_length() and c["halvings_per_slot"] == 1
        assert c["bytes_in"] == c["n"] * (8 + 8 + 4 + 16 * 4)


def test_the_tools_reference_is_the_tests_reference():
    """the numpy reference the tool checks the device against, on its own three graphs at a small n"""
    spec = importlib.util.spec_from_file_location("ab_families", os.path.join(ROOT, "tools", "ab_families.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for kind in ("random", "chain", "star"):
        for n in (1, 2, 777):
            g = tool.graph(kind, n)
            family, size, counts = tool.reference(*g)
            want = F.families(*g, tool.NUM, tool.DEN)
            assert np.array_equal(family, want["family"]) and np.array_equal(size, want["family_size"]), (kind, n)
            assert counts == want["counts"], (kind, n)
    c = tool.reference(*tool.graph("random", 4096))[2]
    assert c["families"] > 50 and c["missing"] > 0 and c["weak"] > 0 and c["self_slots"] > 0
    assert tool.reference(*tool.graph("chain", 500))[2]["largest"] == 500
    assert tool.reference(*tool.graph("star", 500))[2]["largest"] == 500
