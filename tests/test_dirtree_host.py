"""Duplicate directories, the host layers: the five entry points in the header,
the binding and the library, the Engine methods, and sdcas_tree_plan (which
needs no GPU) against tests/_tree_ref.py. The GPU side is
tests/test_gpu_dirtree.py."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from spacedrive_amd import _native as N
from tests import _tree_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_tree_plan": 6, "sdcas_tree_digests": 13, "sdcas_dev_tree_digests": 14, "sdcas_tree_top": 7,
           "sdcas_dev_tree_top": 8}


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    lib = ctypes.CDLL(N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sdcas_\w+)", out))
    for name, nargs in SYMBOLS.items():
        assert name in N.ABI_SYMBOLS
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in exported and getattr(lib, name) is not None
        assert len(getattr(N.load(), name).argtypes) == nargs, name
    for name in SYMBOLS:
        if name != "sdcas_tree_plan":
            assert re.search(r"\bint %s\(sdcas_ctx \*ctx," % name, hdr), name


def test_constants_and_counts_layouts():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    for name, value in (("TREE_DIR", 1), ("TREE_INCOMPLETE", 2), ("TREE_EMPTY", 4), ("TOP_DUP", 1),
                        ("TOP_NESTED", 2)):
        assert re.search(r"#define SDCAS_%s\s+%du\b" % (name, value), hdr), name
        assert getattr(N, "SDCAS_" + name) == value
    assert re.search(r"#define SDCAS_TREE_MAX_DEPTH\s+4096\b", hdr) and N.SDCAS_TREE_MAX_DEPTH == 4096
    for struct, cls, want in (("sdcas_tree_counts", N.TreeCounts, list(R.TREE_COUNTS)),
                              ("sdcas_top_counts", N.TopCounts, list(R.TOP_COUNTS))):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        fields = re.findall(r"uint64_t (\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == want and [f for f, _ in cls._fields_] == want
        assert ctypes.sizeof(cls) == 48
        assert cls(1, 2, 3, 4, 5, 6).as_dict() == dict(zip(want, range(1, 7)))


def test_abi_version_is_still_7():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    assert "#define SDCAS_ABI_VERSION 7" in hdr
    assert N.SDCAS_ABI_VERSION == 7 and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("duplicate directories: tree digests and top-most sets"):]
    assert "added after abi 7; probe for the symbol" in section[:400].lower()


def test_engine_methods_exist():
    from spacedrive_amd import Engine
    for name in ("tree_plan", "tree_digests", "dev_tree_digests", "tree_top", "dev_tree_top",
                 "identify_duplicate_trees"):
        assert callable(getattr(Engine, name)), name


def test_a_null_context_is_refused_without_a_device():
    L = N.load()
    assert L.sdcas_tree_digests(None, None, None, None, None, 0, None, None, None, None, None, None,
                                None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_tree_digests(None, None, None, None, None, 0, None, None, None, None, None, None, None,
                                    None) == N.SDCAS_E_INVALID
    assert L.sdcas_tree_top(None, None, None, 0, None, None, None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_tree_top(None, None, None, 0, None, None, None, None) == N.SDCAS_E_INVALID


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_dt_keys", "k_dt_pkeys", "k_dt_fix", "k_dt_gate", "k_dt_wkeys", "k_dt_select", "k_dt_files", "k_dt_gather", "k_dt_head", "k_dt_finish",
              "k_tt_mark", "k_tt_write"):
        assert k in out, k


# ---- sdcas_tree_plan ---------------------------------------------------------------

def plan(parent, is_dir, outputs=(True, True, True)):
    """the C call -> (rc, depth, children, levels); outputs: which are passed"""
    parent = np.ascontiguousarray(parent, np.int64)
    is_dir = np.ascontiguousarray(is_dir, np.uint8)
    n = parent.size
    depth = np.full(n, 0xEEEEEEEE, np.uint32)
    children = np.full(n, 0xEEEEEEEE, np.uint64)
    levels = ctypes.c_uint64(0xEEEEEEEE)
    ptr = lambda a: a.ctypes.data if a.size else None
    rc = N.load().sdcas_tree_plan(ptr(parent), ptr(is_dir), n, ptr(depth) if outputs[0] else None,
                                  ptr(children) if outputs[1] else None,
                                  ctypes.byref(levels) if outputs[2] else None)
    return rc, depth, children, int(levels.value)


def agree(parent, is_dir):
    rc, depth, children, levels = plan(parent, is_dir)
    try:
        want = R.tree_plan(parent, is_dir)
    except R.ShapeError as e:
        assert rc == e.code, (rc, e.code, str(e))
        return rc
    assert rc == N.SDCAS_OK
    assert (depth == want[0]).all() and (children == want[1]).all() and levels == want[2]
    return rc


def chain(n):
    """n directories, each inside the one before"""
    return np.arange(-1, n - 1, dtype=np.int64), np.ones(n, np.uint8)


def test_plan_smallest():
    rc, _, _, levels = plan([], [])
    assert rc == N.SDCAS_OK and levels == 0
    assert agree([-1], [0]) == N.SDCAS_OK and agree([-1], [1]) == N.SDCAS_OK
    assert agree([-1, 0, 0, -1, 3, 0], [1, 0, 0, 1, 0, 1]) == N.SDCAS_OK


def test_plan_depth_limit():
    assert agree(*chain(4096)) == N.SDCAS_OK
    assert plan(*chain(4096))[3] == 4096
    assert agree(*chain(4097)) == N.SDCAS_E_CAPACITY
    # a file at the bottom counts as a level
    parent, is_dir = chain(4096)
    assert agree(np.r_[parent, 4095], np.r_[is_dir, 0].astype(np.uint8)) == N.SDCAS_E_CAPACITY


def test_plan_refuses_bad_shapes():
    assert agree([-1, 0], [0, 0]) == N.SDCAS_E_INVALID  # a file as parent
    assert agree([-1, 2], [1, 1]) == N.SDCAS_E_INVALID  # parent == n
    assert agree([-2, 0], [1, 1]) == N.SDCAS_E_INVALID
    assert agree([0], [1]) == N.SDCAS_E_INVALID  # a 1-cycle
    assert agree([2, 0, 1, -1], [1, 1, 1, 1]) == N.SDCAS_E_INVALID  # a 3-cycle beside a root
    assert agree([-1, 3, 1, 2, 0], [1, 1, 1, 1, 0]) == N.SDCAS_E_INVALID  # a cycle with a tree beside it


def test_plan_children_before_parents_and_null_outputs():
    is_dir = np.ones(300, np.uint8)
    parent = np.where(np.arange(300) == 299, -1, np.arange(1, 301))  # entry i lies inside entry i + 1
    assert agree(parent, is_dir) == N.SDCAS_OK
    assert plan(parent, is_dir)[1][0] == 299
    full = plan(parent, is_dir)
    for j in range(3):
        outputs = [k != j for k in range(3)]
        got = plan(parent, is_dir, outputs)
        assert got[0] == N.SDCAS_OK
        for k in range(3):
            if outputs[k]:
                assert np.array_equal(got[1 + k], full[1 + k])
            else:
                assert np.all(np.asarray(got[1 + k]) == 0xEEEEEEEE), "a null output was written"


def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_tree.py"), "--count-only", "--entries",
                        "20000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = json.loads(r.stdout.strip().splitlines()[-1])["model"]
    n, dirs, roots = m["entries"], m["dirs"], m["roots"]
    assert 17000 <= n <= 23000 and m["files"] + dirs == n and 0 < roots < dirs
    assert m["levels"] <= 12 and m["dir_levels"] <= 11 and m["largest_dir"] == 5000
    assert m["message_bytes"] == 16 * dirs + 72 * (n - roots)
    b = m["bytes_tree_digests"]
    assert b["clear"] == 16 * n and b["hash"] == m["message_bytes"] + 32 * dirs and b["head"] == 48 * dirs
    assert b["name_sort"] == 8 * (32 * n + 4096 * -(-n // 4096)) and m["parent_sort_passes"] == 2
    assert m["bytes_tree_top"]["clear"] == 12 * n and m["shape_upload_bytes"] == 5 * n + 16 * dirs
    assert m["bytes_per_entry"]["tree_digests"] > m["bytes_per_entry"]["tree_top"] > 0


def test_tree_shape_and_report_shaping_without_gpu():
    """tree_shape_from and tree_report_from on hand-made rows
    (tests/cpp/test_dirtree.cpp without arguments)"""
    path = os.path.join(ROOT, "tests", "cpp", "build", "test_dirtree")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "dirtree.mk"], check=True)
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    hpp = open(os.path.join(ROOT, "include", "sdcore.hpp")).read()
    for name in ("tree_shape_from", "tree_report_from", "tree_report(", "file_paths_in_location", "TreeDigests tree_digests",
                 "TreeTop tree_top"):
        assert name in hpp, name


def test_plan_random_entries():
    parent, is_dir = R.random_tree(100000, 7)
    assert agree(parent, is_dir) == N.SDCAS_OK
    from spacedrive_amd import Engine
    depth, children, levels = Engine.tree_plan(parent, is_dir)
    want = R.tree_plan(parent, is_dir)
    assert (depth == want[0]).all() and (children == want[1]).all() and levels == want[2] and levels > 3
    with pytest.raises(N.SdcasError) as e:
        Engine.tree_plan([0], [1])
    assert e.value.code == N.SDCAS_E_INVALID
