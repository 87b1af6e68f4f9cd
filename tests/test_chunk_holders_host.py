"""The holders index, the host layers: the entry points in the header, the
binding and the library, the GPU-free check, the tool's model, and — on the
GPU, where a context exists — the host calls' refusals that come before the
device is touched. The kernels' tests are tests/test_gpu_chunk_holders.py and
tests/test_gpu_similar_holders.py."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from spacedrive_amd import _native as N
from tests import _chunk_holders_ref as H
from tests import _chunk_index_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_chunk_holders_check": 7, "sdcas_chunk_holders_match": 15, "sdcas_dev_chunk_holders_match": 16,
           "sdcas_chunk_holders_add": 20, "sdcas_dev_chunk_holders_add": 21, "sdcas_chunk_holders_remove": 15,
           "sdcas_dev_chunk_holders_remove": 16}
U64_MAX = (1 << 64) - 1


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sdcas_\w+)", out))
    for name, nargs in SYMBOLS.items():
        assert name in N.ABI_SYMBOLS and name in exported, name
        assert len(getattr(N.load(), name).argtypes) == nargs, name
        assert re.search(r"\bint %s\(" % name, hdr), name
    assert "#define SDCAS_ABI_VERSION 7" in hdr and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("holders index: a chunk index that can forget files"):]
    assert "added after abi 7; probe for the symbol" in section[:300].lower()
    assert "every valid chunk index is a valid" in " ".join(section[:2500].lower().split())
    assert "sdcas_holders_remove_counts" in section
    assert [name for name, _ in N.HoldersRemoveCounts._fields_] == ["entries_old", "removed", "entries_new", "values"]
    assert ctypes.sizeof(N.HoldersRemoveCounts) == 32


def test_a_null_context_is_refused_without_a_device():
    L = N.load()
    assert L.sdcas_chunk_holders_match(*([None] * 5), 0, 0, None, None, None, 0, None, None, None,
                                       None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_chunk_holders_match(*([None] * 5), 0, 0, None, None, None, 0, None, None, None, None,
                                           None) == N.SDCAS_E_INVALID
    assert L.sdcas_chunk_holders_add(*([None] * 5), 0, 0, None, None, None, None, 0, None, None, None, None, 0, None,
                                     None, None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_chunk_holders_add(*([None] * 5), 0, 0, None, None, None, None, 0, None, None, None, None, 0,
                                         None, None, None, None) == N.SDCAS_E_INVALID
    assert L.sdcas_chunk_holders_remove(*([None] * 5), 0, 0, None, 0, None, None, None, None, 0,
                                        None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_chunk_holders_remove(*([None] * 5), 0, 0, None, 0, None, None, None, None, 0, None,
                                            None) == N.SDCAS_E_INVALID


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_ch_match", "k_ch_merge", "k_ch_head", "k_ch_scan", "k_ch_place", "k_ix_place_old", "k_ix_dir",
              "k_ch_rm_mark", "k_ch_rm_scatter"):
        assert k in out, k


def test_engine_and_index_methods_exist():
    from spacedrive_amd import ChunkHolders, ChunkIndex, Engine
    for name in ("chunk_holders_check", "chunk_holders_match", "dev_chunk_holders_match", "chunk_holders_add",
                 "dev_chunk_holders_add", "chunk_holders_remove", "dev_chunk_holders_remove"):
        assert callable(getattr(Engine, name)), name
    for name in ("match", "add", "remove", "arrays", "save", "load", "from_index", "_upload", "_match_dev", "_add_dev"):
        assert callable(getattr(ChunkHolders, name)), name
    assert issubclass(ChunkHolders, ChunkIndex)


def small_index():
    keys, dig = R.random_pairs(np.random.default_rng(5), 12)
    return sorted((int(k), d.tobytes(), v) for i, (k, d) in enumerate(zip(keys, dig)) for v in (3, 9, U64_MAX)[:1 + i % 3])


def test_check_without_gpu():
    from spacedrive_amd import Engine
    entries = small_index()
    n = len(entries)
    for bits in (0, 2, 5):
        k, d, v, dr, _ = H.arrays(entries, bits)
        assert Engine.chunk_holders_check(k, d, v, dr, bits) == (N.SDCAS_OK, None)  # equal pairs, ascending values
    k, d, v, dr, _ = H.arrays(entries, 2)
    run = next(i for i in range(1, n) if entries[i][:2] == entries[i - 1][:2])
    # an equal triple
    bad = v.copy()
    bad[run] = bad[run - 1]
    assert Engine.chunk_holders_check(k, d, bad, dr, 2) == (N.SDCAS_E_INVALID, run)
    # a descending value: only in the unsigned order is 2^64 - 1 above 9
    last = next(i for i in range(n) if entries[i][2] == U64_MAX)
    assert entries[last - 1][:2] == entries[last][:2] and entries[last - 1][2] == 9
    bad = v.copy()
    bad[last - 1], bad[last] = bad[last], bad[last - 1]
    assert Engine.chunk_holders_check(k, d, bad, dr, 2) == (N.SDCAS_E_INVALID, last)
    # values NULL stand for all 0: a repeated pair is then an equal triple
    assert Engine.chunk_holders_check(k, d, None, dr, 2) == (N.SDCAS_E_INVALID, run)
    # a wrong directory slot, the last one too
    for slot in (1, 4):
        bad = dr.copy()
        bad[slot] += 1
        assert Engine.chunk_holders_check(k, d, v, bad, 2) == (N.SDCAS_E_INVALID, slot)
    # the limits, before any array is touched
    L = N.load()
    assert L.sdcas_chunk_holders_check(None, None, None, None, (1 << 30) + 1, 0, None) == N.SDCAS_E_CAPACITY
    assert L.sdcas_chunk_holders_check(None, None, None, None, 0, 29, None) == N.SDCAS_E_CAPACITY
    assert L.sdcas_chunk_holders_check(None, None, None, None, 0, 0, None) == N.SDCAS_E_INVALID
    empty = np.zeros(2, np.uint32)
    assert L.sdcas_chunk_holders_check(None, None, None, empty.ctypes.data, 0, 0, None) == N.SDCAS_OK


def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_chunk_holders.py"), "--count-only"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    models = json.loads(r.stdout.strip().splitlines()[-1])["model"]
    assert [m["n"] for m in models] == [1 << 22, 1 << 24, 1 << 26] and [m["bits"] for m in models] == [20, 22, 24]
    m = models[1]
    assert m["copy_bytes_each_way"] == 48 << 24 and len(m["remove"]) == 6
    for leg in m["remove"]:
        assert leg["bytes_read"] == 48 << 24 and leg["bytes_written"] == 48 * leg["rebuild_triples"]
        assert leg["requests_into_removed_per_entry"] == {1 << 10: 11, 1 << 20: 21}[leg["r"]]
    assert sorted({leg["fraction"] for leg in m["remove"]}) == [0.01, 0.1, 0.5]
    steps = m["match_dependent_requests_per_query"]
    assert steps["key_steps_first"] == steps["key_steps_last"] == 3


@pytest.mark.gpu
def test_host_calls_refuse_overlap_and_unsorted_removed():
    """SDCAS_E_INVALID from pointers and sizes, and from a `removed` that does
    not ascend, with the context's message"""
    from spacedrive_amd import Engine
    eng = Engine()
    try:
        entries = small_index()
        n = len(entries)
        k, d, v, dr, _ = H.arrays(entries, 2)
        removed = np.array([3, 9], np.uint64)
        nd, nv, ndr = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint64), np.zeros(5, np.uint32)
        L, vp = eng.L, lambda a: a.ctypes.data

        def call(new_keys, rem=removed, new_vals=nv):
            return L.sdcas_chunk_holders_remove(eng.ctx, vp(k), vp(d), vp(v), vp(dr), n, 2, vp(rem), rem.size, new_keys,
                                                vp(nd), vp(new_vals), vp(ndr), 2, None)

        assert call(vp(k)) == N.SDCAS_E_INVALID  # the new keys are the old ones
        assert call(vp(k) + 8 * (n - 1)) == N.SDCAS_E_INVALID
        nk = np.zeros(n, np.uint64)
        both = np.zeros(n + 2, np.uint64)  # `removed` and the new values in one allocation
        both[:2] = removed
        assert call(vp(nk), rem=both[:2], new_vals=both[1:1 + n]) == N.SDCAS_E_INVALID
        for rem in ([9, 3], [3, 3], [3, 9, 9]):
            with pytest.raises(N.SdcasError) as ei:
                eng.chunk_holders_remove((k, d, v, dr, 2), np.array(rem, np.uint64))
            assert ei.value.code == N.SDCAS_E_INVALID and "ascend" in str(ei.value)
        # and the same arguments in order are taken
        (nk, _, nvv, _, _), counts = eng.chunk_holders_remove((k, d, v, dr, 2), removed)
        assert counts["entries_new"] == int((v == U64_MAX).sum()) == nk.size and (nvv == U64_MAX).all()
    finally:
        eng.close()
