"""The chunk peers, the host layers: the entry points in the header, the binding
and the library, the GPU-free plan and its ranges, the Python methods and the
tool's model. The kernels' tests are tests/test_gpu_chunk_peers.py and
tests/test_gpu_similar_peers.py."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

from spacedrive_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_chunk_peers_plan": 6, "sdcas_chunk_peers": 26, "sdcas_dev_chunk_peers": 27}


def plan(m, n_files, k, h):
    pairs, ws = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = N.load().sdcas_chunk_peers_plan(m, n_files, k, h, ctypes.byref(pairs), ctypes.byref(ws))
    return rc, pairs.value, ws.value


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sdcas_\w+)", out))
    for name, nargs in SYMBOLS.items():
        assert name in N.ABI_SYMBOLS and name in exported, name
        assert len(getattr(N.load(), name).argtypes) == nargs, name
        assert re.search(r"\bint %s\(" % name, hdr), name
    assert "#define SDCAS_ABI_VERSION 7" in hdr and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("chunk peers: the files that hold most of a file's bytes"):]
    assert "added after abi 7; probe for the symbol" in section[:300].lower()
    assert "sdcas_peers_counts" in section and "SDCAS_PEERS_EARLIER" in section and "SDCAS_PEERS_ALL" in section
    assert [name for name, _ in N.PeersCounts._fields_] == ["files", "chunks", "common_chunks", "pairs", "edges",
                                                            "files_with_peer", "overflow"]
    assert ctypes.sizeof(N.PeersCounts) == 56
    assert (N.SDCAS_PEERS_EARLIER, N.SDCAS_PEERS_ALL) == (0, 1)


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_cp_runs", "k_cp_offsets", "k_cp_expand", "k_cp_merge", "k_cp_heads", "k_cp_scan64", "k_cp_edges",
              "k_cp_write", "k_ch_scan"):
        assert k in out, k


def test_plan_is_the_bound_that_cannot_overflow():
    for m, h, want in ((0, 1, 0), (1, 1, 1), (1 << 30, 1, 1 << 30), (1 << 20, 1 << 20, 1 << 30), (1000, 64, 64000)):
        rc, pairs, ws = plan(m, 10, 4, h)
        assert (rc, pairs) == (N.SDCAS_OK, want), (m, h)
        assert ws >= 16 * m + 57 * pairs  # the per-chunk and per-pair arrays, and the scans' levels
    assert plan(1 << 20, 10, 4, 1 << 20)[1] < (1 << 40)  # capped
    # NULL outputs are taken
    assert N.load().sdcas_chunk_peers_plan(5, 1, 1, 1, None, None) == N.SDCAS_OK


def test_plan_is_non_decreasing_in_m():
    last = (0, 0)
    for m in (0, 1, 2, 255, 256, 257, 65536, 65537, 1 << 20, 1 << 24, (1 << 24) + 1, 1 << 30):
        rc, pairs, ws = plan(m, 3, 4, 16)
        assert rc == N.SDCAS_OK and pairs >= last[0] and ws >= last[1], m
        last = (pairs, ws)


def test_ranges():
    for k in (0, 65):
        assert plan(10, 1, k, 4)[0] == N.SDCAS_E_INVALID
    for h in (0, (1 << 20) + 1):
        assert plan(10, 1, 4, h)[0] == N.SDCAS_E_INVALID
    assert plan(10, 1, 1, 1)[0] == plan(10, 1, 64, 1 << 20)[0] == N.SDCAS_OK
    assert plan((1 << 30) + 1, 1, 4, 4)[0] == N.SDCAS_E_CAPACITY
    assert plan(10, (1 << 32) - 1, 4, 4)[0] == N.SDCAS_E_CAPACITY


def test_a_null_context_and_an_unknown_mode_are_refused_without_a_device():
    L = N.load()
    for mode in (0, 1, 2):
        assert L.sdcas_chunk_peers(*([None] * 5), 0, 0, *([None] * 5), 0, None, 0, 4, 64, mode, 0, *([None] * 7)) \
            == N.SDCAS_E_INVALID
        assert L.sdcas_dev_chunk_peers(*([None] * 5), 0, 0, *([None] * 5), 0, None, 0, 4, 64, mode, 0,
                                       *([None] * 8)) == N.SDCAS_E_INVALID


def test_engine_agrees_with_the_plan_and_the_methods_exist():
    from spacedrive_amd import ChunkHolders, ChunkIndex, Engine
    for m, h in ((0, 1), (1, 1), (12345, 64), (1 << 20, 1 << 20)):
        assert Engine.chunk_peers_plan(m, 7, 4, h) == plan(m, 7, 4, h)[1:]
    for bad in ((1, 1, 0, 4), (1, 1, 65, 4), (1, 1, 4, 0), (1, 1, 4, (1 << 20) + 1), ((1 << 30) + 1, 1, 4, 4)):
        with pytest.raises(N.SdcasError) as ei:
            Engine.chunk_peers_plan(*bad)
        assert ei.value.code == (N.SDCAS_E_CAPACITY if bad[0] > (1 << 30) else N.SDCAS_E_INVALID)
    for name in ("chunk_peers_plan", "chunk_peers", "dev_chunk_peers"):
        assert callable(getattr(Engine, name)), name
    assert callable(ChunkHolders.peers) and not hasattr(ChunkIndex, "peers")
    sig = inspect.signature(ChunkHolders.peers).parameters
    assert (sig["k"].default, sig["max_holders"].default, sig["mode"].default) == (4, 64, "earlier")
    sig = inspect.signature(Engine.similar_files_indexed).parameters
    assert sig["peers"].default == 0 and sig["max_holders"].default == 64
    assert list(sig)[:6] == ["self", "paths", "file_ids", "index", "params", "window_bytes"]


def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_chunk_peers.py"), "--count-only"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    models = json.loads(r.stdout.strip().splitlines()[-1])["model"]
    assert [(c["n"], c["max_holders"]) for c in models] == [(1 << 22, 16), (1 << 22, 64), (1 << 24, 16), (1 << 24, 64)]
    for c in models:
        assert c["m"] == 1 << 20 and c["plan_max_pairs"] == min(c["m"] * c["max_holders"], 1 << 30)
        assert c["merge_passes_at_plan_bound"] == (c["plan_max_pairs"] - 1).bit_length()
        assert c["workspace_bytes_at_plan_bound"] == plan(c["m"], c["n_files"], c["k"], c["max_holders"])[2]
        assert c["halvings_per_chunk"] == 3
