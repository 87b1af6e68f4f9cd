"""The family recipes, the host layers: the entry points in the header, the
binding and the library, the GPU-free plan and its ranges, the Python methods'
argument checks and the tool's model. The kernels' tests are
tests/test_gpu_family_recipes.py and tests/test_gpu_similar_recipes.py."""
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
from tests import _family_recipes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_family_recipes_plan": 3, "sdcas_family_recipes": 19, "sdcas_dev_family_recipes": 20}
KERNELS = ("k_fr_insert", "k_fr_source", "k_fr_scan", "k_fr_emit", "k_fr_close", "k_fr_rows", "k_fr_totals")
BYTES_KERNELS = ("k_fb_insert", "k_fb_classify", "k_fb_rows", "k_fb_heads", "k_fb_merge", "k_fb_write", "k_fb_totals")


def plan(m, n):
    ws = ctypes.c_uint64(0)
    rc = N.load().sdcas_family_recipes_plan(m, n, ctypes.byref(ws))
    return rc, ws.value


def load_tool():
    spec = importlib.util.spec_from_file_location("ab_family_recipes",
                                                  os.path.join(ROOT, "tools", "ab_family_recipes.py"))
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
    section = hdr[hdr.index("family recipes: rebuild every file from its family's stored bytes"):]
    assert "added after abi 7; probe for the symbol (sdcas_abi_version stays 7)" in section[:300].lower()
    fields = re.findall(r"uint64_t (\w+);", section[section.index("typedef struct sdcas_family_recipes_counts"):
                                                    section.index("} sdcas_family_recipes_counts;")])
    assert fields == list(R.COUNTS) == [name for name, _ in N.FamilyRecipesCounts._fields_]
    assert fields == ["files", "chunks", "ops", "literal_ops", "copy_ops", "literal_bytes", "copy_bytes", "longest_op"]
    assert ctypes.sizeof(N.FamilyRecipesCounts) == 64
    # the header's worked example is the reference's
    for key in ("chunk_file", "chunk_off", "chunk_len", "rep"):
        assert str(R.EXAMPLE[key]).replace(" ", "") in section.replace(" ", ""), key


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in KERNELS + BYTES_KERNELS:  # family_bytes.hip's kernels keep their names beside the new ones
        assert k in out, k


def test_plan_ranges_and_bytes():
    assert plan(1 << 30, 1 << 30)[0] == N.SDCAS_OK
    assert plan((1 << 30) + 1, 4)[0] == N.SDCAS_E_CAPACITY
    assert plan(4, (1 << 30) + 1)[0] == N.SDCAS_E_CAPACITY
    assert plan(0, 0)[0] == N.SDCAS_OK
    assert N.load().sdcas_family_recipes_plan(5, 1, None) == N.SDCAS_OK  # a NULL output is taken
    sizes = (0, 1, 2, 255, 256, 257, 65536, 70000, 1 << 20, (1 << 24) + 1, 1 << 30)
    last = 0
    # monotone in m: a table of at least 2 m u32 slots (below 4 m), 17 bytes per chunk, 8 KiB of counters and a bit
    for m in sizes:
        rc, ws = plan(m, 1000)
        assert rc == N.SDCAS_OK and ws >= last and ws >= 25 * m and ws <= 34 * m + 8 * 1000 + 12288, m
        last = ws
    last = 0
    for n in sizes:  # monotone in n_files: 8 bytes per row
        rc, ws = plan(1000, n)
        assert rc == N.SDCAS_OK and ws >= last and ws >= 8 * n and ws <= 8 * n + 34 * 1000 + 12288, n
        last = ws


def test_a_null_context_is_refused_without_a_device():
    L = N.load()
    assert L.sdcas_family_recipes(None, None, None, None, None, 0, None, 0, *([None] * 11)) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_family_recipes(None, None, None, None, None, 0, None, 0, *([None] * 12)) == N.SDCAS_E_INVALID


def test_engine_agrees_with_the_plan_and_the_methods_exist():
    from spacedrive_amd import Engine
    for m, n in ((0, 0), (1, 1), (12345, 77), (1 << 30, 1 << 30)):
        assert Engine.family_recipes_plan(m, n) == plan(m, n)[1]
    for bad in (((1 << 30) + 1, 4), (4, (1 << 30) + 1)):
        with pytest.raises(N.SdcasError) as ei:
            Engine.family_recipes_plan(*bad)
        assert ei.value.code == N.SDCAS_E_CAPACITY
    for name in ("family_recipes_plan", "family_recipes", "dev_family_recipes", "family_recipes_of", "similar_recipes"):
        assert callable(getattr(Engine, name)), name
    sig = inspect.signature(Engine.family_recipes).parameters
    assert list(sig) == ["self", "chunk_file", "chunk_len", "rep", "family", "chunk_off"]
    assert sig["chunk_off"].default is None
    sig = inspect.signature(Engine.dev_family_recipes).parameters
    assert list(sig) == ["self", "chunk_file", "chunk_off", "chunk_len", "rep", "m", "family", "n_files", "op_chunk",
                         "op_src_chunk", "op_row", "op_src_row", "op_dst_off", "op_src_off", "op_len", "chunk_op",
                         "row_ops", "row_first_op", "counts", "stream"]
    assert all(sig[name].default == 0 for name in list(sig)[8:])
    sig = inspect.signature(Engine.family_recipes_of).parameters
    assert list(sig) == ["self", "results", "file_ids", "num", "den"] and (sig["num"].default, sig["den"].default) == (1, 2)
    sig = inspect.signature(Engine.similar_recipes).parameters
    assert list(sig) == ["self", "paths", "k", "max_holders", "num", "den", "params", "window_bytes"]
    assert [sig[name].default for name in list(sig)[2:]] == [4, 64, 1, 2, None, 256 << 20]
    # what was there stays as it was
    sig = inspect.signature(Engine.family_bytes_of).parameters
    assert list(sig) == ["self", "results", "file_ids", "num", "den"] and (sig["num"].default, sig["den"].default) == (1, 2)
    sig = inspect.signature(Engine.similar_families).parameters
    assert list(sig) == ["self", "paths", "k", "max_holders", "num", "den", "params", "window_bytes"]


class _NoDevice:
    """an Engine whose argument checks run and whose library is never reached"""
    def __getattr__(self, name):
        raise AssertionError(f"the call reached {name}")


def test_the_methods_check_their_arguments_before_any_call():
    from spacedrive_amd import Engine
    e = _NoDevice()
    with pytest.raises(ValueError, match="3 chunk files, 2 lengths, 3 reps"):
        Engine.family_recipes(e, [0, 0, 0], [1, 2], [0, 1, 2], [0])
    with pytest.raises(ValueError, match="3 chunk files, 3 lengths, 1 reps"):
        Engine.family_recipes(e, [0, 0, 0], [1, 2, 3], [0], [0])
    with pytest.raises(ValueError, match="running_offsets: 2 chunk files, 1 lengths"):
        Engine.running_offsets([0, 0], [1])

    class Sums:
        running_offsets = staticmethod(Engine.running_offsets)

        def __getattr__(self, name):
            raise AssertionError(f"the call reached {name}")
    with pytest.raises(ValueError, match="3 chunk files, 2 offsets"):
        Engine.family_recipes(Sums(), [0, 0, 0], [1, 2, 3], [0, 1, 2], [0], chunk_off=[0, 1])

    class Inputs:
        _family_inputs = Engine._family_inputs

        def __getattr__(self, name):
            raise AssertionError(f"the call reached {name}")
    with pytest.raises(ValueError, match="family_recipes_of: 1 results, 2 id arrays"):
        Engine.family_recipes_of(Inputs(), [{}], [[0], [1]])
    with pytest.raises(ValueError, match="family_recipes_of: a result has no chunk_file"):
        Engine.family_recipes_of(Inputs(), [{"sizes": [1]}], [[0]])
    r = {"sizes": [1], "chunk_file": [0, 1], "chunk_len": [1, 1], "chunk_keys": [0, 0],
         "chunk_digests": np.zeros((2, 32), np.uint8)}
    with pytest.raises(ValueError, match="family_recipes_of: a result's rows do not match its ids"):
        Engine.family_recipes_of(Inputs(), [r], [[7]])
    with pytest.raises(ValueError, match="family_bytes_of: 1 results, 2 id arrays"):  # its messages keep its name
        Engine.family_bytes_of(Inputs(), [{}], [[0], [1]])


def test_running_offsets():
    from spacedrive_amd import Engine
    assert Engine.running_offsets([], []).tolist() == []
    assert Engine.running_offsets(R.EXAMPLE["chunk_file"], R.EXAMPLE["chunk_len"]).tolist() == R.EXAMPLE["chunk_off"]
    rng = np.random.default_rng(4)
    for m in (1, 2, 65, 700):  # interleaved files too: position order inside each file
        cf = rng.integers(0, 9, m).astype(np.uint32)
        ln = rng.choice(np.array([0, 1, 77, 1 << 63], np.uint64), m)
        got = Engine.running_offsets(cf, ln)
        assert got.dtype == np.uint64 and np.array_equal(got, R.running_offsets(cf, ln))


def test_makefile_and_documents_name_the_feature():
    mk = open(os.path.join(ROOT, "spacedrive_amd", "csrc", "Makefile")).read()
    assert "family_recipes.hip" in mk and "family_bytes.hip" in mk
    assert "ab_family_recipes.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "tools/ab_family_recipes.py" in readme and "family_recipes.hip" in readme
    assert "similar_recipes" in readme and "rebuild_files" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.12" in design and all(k in design for k in KERNELS)


def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_family_recipes.py"), "--count-only"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    models = json.loads(lines[0])["model"]
    assert [c["m"] for c in models] == [1 << 20, 1 << 22]
    for c in models:
        m, n = c["m"], c["m"] // 64
        assert c["n_files"] == n and c["workspace_bytes"] == plan(m, n)[1]
        assert c["table_slots"] == 2 * m
        assert c["workspace_bytes"] >= 4 * c["table_slots"] + 17 * m + 4 * c["scan_counts"] + 8 * n
        assert c["scan_counts"] == m // 256 and c["scan_passes"] == m // 256 // 1024
        assert c["launches"] == 7 and c["fills"] == 2
        assert c["bytes_in"] == m * 28 + n * 8 and c["bytes_out_most"] == m * 44 + n * 8 + 64


def test_the_tools_reference_is_the_tests_reference():
    """the numpy reference the tool checks the device against, on its own four corpora at small sizes"""
    tool = load_tool()
    names = R.OPS + ("chunk_op",) + R.ROWS
    for kind in tool.KINDS:
        for m in (1, 64, 130, 64 * 40 + 5):
            g = tool.corpus(kind, m)
            got, want = tool.reference(*g), R.family_recipes(*g)
            for name in names:
                assert np.array_equal(got[name], want[name]) and got[name].dtype == want[name].dtype, (kind, m, name)
            assert got["counts"] == want["counts"], (kind, m)
    # and on inputs with rows, chunks and reps outside their ranges, zero and wrapping lengths, any offsets
    rng = np.random.default_rng(5)
    for _ in range(40):
        m, n = int(rng.integers(0, 50)), int(rng.integers(1, 9))
        g = (rng.integers(0, n + 2, m).astype(np.uint32), rng.choice(np.array([0, 3, 6, 1 << 63], np.uint64), m),
             rng.choice(np.array([0, 3, 1 << 63], np.uint64), m), rng.integers(-2, m + 2, m).astype(np.int64),
             rng.integers(-1, n + 1, n).astype(np.int64))
        got, want = tool.reference(*g), R.family_recipes(*g)
        for name in names:
            assert np.array_equal(got[name], want[name]), name
        assert got["counts"] == want["counts"]
    m = 1 << 12
    c = tool.reference(*tool.corpus("random", 1 << 14))["counts"]
    assert c["chunks"] == 1 << 14 and 0 < c["copy_ops"] and c["ops"] < c["chunks"]
    c = tool.reference(*tool.corpus("one_run", m))["counts"]
    assert c["ops"] == 1 and c["literal_ops"] == 1 and c["longest_op"] == c["literal_bytes"] and c["copy_bytes"] == 0
    c = tool.reference(*tool.corpus("no_runs", m))["counts"]
    assert c["ops"] == m and c["literal_ops"] == c["copy_ops"] == m // 2
    c = tool.reference(*tool.corpus("one_class", m))["counts"]
    assert c["ops"] == m and c["literal_ops"] == 1 and c["copy_ops"] == m - 1
