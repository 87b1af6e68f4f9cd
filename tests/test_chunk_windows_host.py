"""Chunk windows, the host layers: the entry points in the header, the binding
and the library, sdcas_chunk_seg_bytes (which needs no GPU), the window
planners of the Python and the C++ layer and the C++ merge. The GPU side is
tests/test_gpu_chunk_windows.py and tests/test_gpu_similar_streamed.py."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from spacedrive_amd import _native as N
from tests import _cdc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_chunk_seg_bytes": 1, "sdcas_chunk_windows": 15, "sdcas_dev_chunk_windows": 18}


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    lib = ctypes.CDLL(N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sdcas_\w+)", out))
    for name, nargs in SYMBOLS.items():
        assert name in N.ABI_SYMBOLS
        assert name in exported and getattr(lib, name) is not None
        assert len(getattr(N.load(), name).argtypes) == nargs, name
    assert re.search(r"\buint64_t sdcas_chunk_seg_bytes\(const sdcas_chunk_params \*params\);", hdr)
    for name in ("sdcas_chunk_windows", "sdcas_dev_chunk_windows"):
        assert re.search(r"\bint %s\(sdcas_ctx \*ctx," % name, hdr), name
    assert N.load().sdcas_chunk_seg_bytes.restype is ctypes.c_uint64


def test_abi_version_is_still_7_and_the_section_says_so():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    assert "#define SDCAS_ABI_VERSION 7" in hdr and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("chunk windows: a file chunked piece by piece"):]
    assert "added after abi 7; probe for the symbol" in section[:300].lower()


def test_a_null_context_is_refused_without_a_device():
    L = N.load()
    assert L.sdcas_chunk_windows(None, None, None, None, None, 0, None, None, None, None, None, None, None, None,
                                 None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_chunk_windows(None, None, None, None, None, 0, None, 0, 0, None, None, None, None, None, None,
                                     None, None, None) == N.SDCAS_E_INVALID


def test_library_holds_the_kernels_and_keeps_the_old_ones():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_cdc_cut_seg", "k_cdc_cut_win", "k_cdc_stitch", "k_cdc_gather", "k_cdc_win_sizes", "k_cdc_cut(", "k_cdc_gear",
              "k_cdc_emit"):
        assert k in out, k


def test_engine_methods_exist():
    from spacedrive_amd import Engine
    for name in ("chunk_seg_bytes", "chunk_windows", "dev_chunk_windows", "plan_windows", "chunk_stream",
                 "similar_files_streamed"):
        assert callable(getattr(Engine, name)), name


# ---- sdcas_chunk_seg_bytes -----------------------------------------------------------------

def seg(params):
    cp = N.ChunkParams(*params, 0) if params is not None else None
    return int(N.load().sdcas_chunk_seg_bytes(ctypes.byref(cp) if cp is not None else None))


def test_seg_bytes(monkeypatch):
    from spacedrive_amd import Engine
    monkeypatch.delenv("SDCAS_CHUNK_SEG_BYTES", raising=False)
    assert seg(None) == seg(R.DEFAULT_PARAMS) == seg(R.TEST_PARAMS) == 1 << 20 == Engine.chunk_seg_bytes()
    # the floor of 2 * max_len, itself rounded up to a multiple of 64
    assert seg((1 << 20, 21, 1 << 22)) == 1 << 23
    assert seg((1 << 20, 21, (1 << 22) + 1)) == (1 << 23) + 64
    # the environment, read per call
    monkeypatch.setenv("SDCAS_CHUNK_SEG_BYTES", "2112")
    assert seg(R.TEST_PARAMS) == 2112 == Engine.chunk_seg_bytes(R.TEST_PARAMS)
    assert seg(R.DEFAULT_PARAMS) == 2 * 65536
    for asked, got in ((2048, 2048), (2049, 2112), (2111, 2112), (2113, 2176), (1, 2048), (4160, 4160)):
        monkeypatch.setenv("SDCAS_CHUNK_SEG_BYTES", str(asked))
        assert seg(R.TEST_PARAMS) == got, asked
    monkeypatch.setenv("SDCAS_CHUNK_SEG_BYTES", "2112")
    assert seg((64, 8, 1025)) == 2112 and seg((64, 8, 1057)) == 2176  # 2114 rounds up
    monkeypatch.setenv("SDCAS_CHUNK_SEG_BYTES", "0")
    assert seg(R.TEST_PARAMS) == 1 << 20
    monkeypatch.setenv("SDCAS_CHUNK_SEG_BYTES", "nonsense")
    assert seg(R.TEST_PARAMS) == 1 << 20
    # invalid parameters
    for bad in ((31, 8, 1024), (64, 5, 1024), (64, 8, 256), (64, 8, (1 << 28) + 1)):
        assert seg(bad) == 0 == Engine.chunk_seg_bytes(bad), bad


# ---- the window planners and the C++ merge ---------------------------------------------------

def test_plan_windows():
    from spacedrive_amd import Engine
    plan = Engine.plan_windows
    assert plan([], 100) == []
    assert plan([10, 20, 30], 100) == [(0, 3, False)]
    assert plan([60, 40, 1], 100) == [(0, 2, False), (2, 1, False)]
    assert plan([60, 41], 100) == [(0, 1, False), (1, 1, False)]
    assert plan([100], 100) == [(0, 1, False)] and plan([101], 100) == [(0, 1, True)]
    assert plan([10, 500, 20, 30, 700, 0], 100) == [(0, 1, False), (1, 1, True), (2, 2, False), (4, 1, True),
                                                     (5, 1, False)]
    assert plan([0, 0, 0], 1) == [(0, 3, False)]
    assert plan([500, 600], 100) == [(0, 1, True), (1, 1, True)]
    assert plan(np.array([5, 5], np.uint64), np.int64(10)) == [(0, 2, False)]
    with pytest.raises(ValueError):
        plan([1], 0)
    # every file in exactly one entry, in order
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 3000, 300).tolist()
    p = plan(lens, 1000)
    assert [f for first, n, _ in p for f in range(first, first + n)] == list(range(300))
    for first, n, streamed in p:
        assert (n == 1 and lens[first] > 1000) if streamed else sum(lens[first:first + n]) <= 1000


def windows_program():
    path = os.path.join(ROOT, "tests", "cpp", "build", "test_chunk_windows")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "chunkwin.mk"], check=True)
    return path


def test_cpp_planner_and_merge_without_gpu():
    """plan_chunk_windows on the lists above and merge_chunk_windows on
    hand-made windows (tests/cpp/test_chunk_windows.cpp without arguments)"""
    r = subprocess.run([windows_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    hpp = open(os.path.join(ROOT, "include", "sdcore.hpp")).read()
    for name in ("WindowChunks chunk_windows", "plan_chunk_windows(", "merge_chunk_windows(",
                 "similarity_report_streamed("):
        assert name in hpp, name


def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_chunk_windows.py"), "--count-only"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = json.loads(r.stdout.strip().splitlines()[-1])["model"]
    assert m["file_bytes"] == 1 << 30 and m["seg_bytes"] == 1 << 20 and m["segments"] == 1024
    assert m["windows"] == 5 and m["window_bytes"] == 256 << 20  # four windows and the tail behind their consumed
    assert m["max_chunks"] == (1 << 30) // 2048 and m["spec_bytes"] >= 8 * m["max_chunks"]


@pytest.mark.gpu
def test_cpp_streamed_report_equals_the_resident_one(tmp_path, monkeypatch):
    """test_chunk_windows --gpu DIR W: similarity_report_streamed in windows of
    W bytes against similarity_report over files made here"""
    monkeypatch.setenv("SDCAS_CHUNK_SEG_BYTES", str(2 * 65536))
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, 700000, dtype=np.uint8)
    files = {"a.bin": a, "b.bin": np.concatenate([a[:1000], np.array([0x42], np.uint8), a[1000:]]),
             "c.bin": rng.integers(0, 256, 30000, dtype=np.uint8), "d.bin": rng.integers(0, 256, 5000, dtype=np.uint8),
             "empty.bin": np.zeros(0, np.uint8)}
    files["sub/e.bin"] = np.concatenate([files["c.bin"], a[:300000]])
    (tmp_path / "loc" / "sub").mkdir(parents=True)
    for name, data in files.items():
        (tmp_path / "loc" / name).write_bytes(data.tobytes())
    r = subprocess.run([windows_program(), "--gpu", str(tmp_path), "200000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert int(re.search(r"pairs (\d+)", r.stdout).group(1)) >= 2
