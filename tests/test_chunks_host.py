"""Content-defined chunks, the host layers: the entry points in the header, the
binding and the library, the Engine methods, and sdcas_chunk_plan (which needs
no GPU) against tests/_cdc_ref.py. The GPU side is tests/test_gpu_chunks.py and
tests/test_gpu_chunk_sharing.py."""
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
SYMBOLS = {"sdcas_chunk_plan": 5, "sdcas_chunk_messages": 13, "sdcas_dev_chunk": 16, "sdcas_chunk_sharing": 12,
           "sdcas_dev_chunk_sharing": 13}
CHUNK_COUNTS = ["files", "chunks", "total_bytes", "hash_cuts", "max_cuts", "end_chunks"]
SHARING_COUNTS = ["files", "chunks", "distinct_chunks", "total_bytes", "stored_bytes", "files_with_peer"]


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
        if name != "sdcas_chunk_plan":
            assert re.search(r"\bint %s\(sdcas_ctx \*ctx," % name, hdr), name


def test_constants_and_counts_layouts():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    assert re.search(r"#define SDCAS_CHUNK_PARAMS_DEFAULT \{2048u, 13u, 65536u, 0u\}", hdr)
    assert N.SDCAS_CHUNK_PARAMS_DEFAULT == R.DEFAULT_PARAMS == (2048, 13, 65536)
    assert re.search(r"#define SDCAS_CHUNK_MAX_CHUNKS \(1ull << 30\)", hdr) and N.SDCAS_CHUNK_MAX_CHUNKS == 1 << 30
    assert re.search(r"#define SDCAS_CHUNK_GEAR_TILE %du\b" % N.SDCAS_CHUNK_GEAR_TILE, hdr)
    assert re.search(r"#define SDCAS_CHUNK_GEAR_STRIP %du\b" % N.SDCAS_CHUNK_GEAR_STRIP, hdr)
    assert N.SDCAS_CHUNK_GEAR_TILE % N.SDCAS_CHUNK_GEAR_STRIP == 0 and N.SDCAS_CHUNK_GEAR_STRIP >= 32
    body = re.search(r"typedef struct sdcas_chunk_params \{(.*?)\} sdcas_chunk_params;", hdr, re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", body) == ["min_len", "avg_bits", "max_len", "reserved"]
    assert [f for f, _ in N.ChunkParams._fields_] == ["min_len", "avg_bits", "max_len", "reserved"]
    assert ctypes.sizeof(N.ChunkParams) == 16
    for struct, cls, want in (("sdcas_chunk_counts", N.ChunkCounts, CHUNK_COUNTS),
                              ("sdcas_sharing_counts", N.SharingCounts, SHARING_COUNTS)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        fields = re.findall(r"uint64_t (\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == want and [f for f, _ in cls._fields_] == want
        assert ctypes.sizeof(cls) == 48
        assert cls(1, 2, 3, 4, 5, 6).as_dict() == dict(zip(want, range(1, 7)))


def test_abi_version_is_still_7():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    assert "#define SDCAS_ABI_VERSION 7" in hdr
    assert N.SDCAS_ABI_VERSION == 7 and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("content-defined chunks: files that share most of their bytes"):]
    assert "added after abi 7; probe for the symbol" in section[:400].lower()


def test_engine_methods_exist():
    from spacedrive_amd import Engine
    for name in ("chunk_plan", "chunk_messages", "dev_chunk", "chunk_sharing", "dev_chunk_sharing", "similar_files"):
        assert callable(getattr(Engine, name)), name


def test_a_null_context_is_refused_without_a_device():
    L = N.load()
    assert L.sdcas_chunk_messages(None, None, None, None, 0, None, None, None, None, None, None, None,
                                  None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_chunk(None, None, None, None, 0, None, 0, 0, None, None, None, None, None, None, None,
                             None) == N.SDCAS_E_INVALID
    assert L.sdcas_chunk_sharing(None, None, None, None, 0, 0, None, None, None, None, None, None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_chunk_sharing(None, None, None, None, 0, 0, None, None, None, None, None, None,
                                     None) == N.SDCAS_E_INVALID


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_cdc_sizes", "k_cdc_scan", "k_cdc_gear", "k_cdc_cut", "k_cdc_emit", "k_cdc_pack", "k_cs_accum",
              "k_cs_max", "k_cs_min", "k_cs_write"):
        assert k in out, k


# ---- sdcas_chunk_plan ---------------------------------------------------------------

def plan(lens, params, outputs=(True, True)):
    lens = np.ascontiguousarray(lens, np.uint64)
    mc, ms = ctypes.c_uint64(0xEEEEEEEE), ctypes.c_uint64(0xEEEEEEEE)
    cp = N.ChunkParams(*params, 0) if params is not None else None
    rc = N.load().sdcas_chunk_plan(lens.ctypes.data if lens.size else None, lens.size,
                                   ctypes.byref(cp) if cp is not None else None,
                                   ctypes.byref(mc) if outputs[0] else None, ctypes.byref(ms) if outputs[1] else None)
    return rc, int(mc.value), int(ms.value)


def test_plan_against_the_reference():
    rng = np.random.default_rng(11)
    cases = [[], [0], [1], [0, 0, 0], [63, 64, 65], [1023, 1024, 1025], list(rng.integers(0, 200000, 500)),
             [1 << 33, 5]]
    for lens in cases:
        for params in (R.TEST_PARAMS, R.DEFAULT_PARAMS, (32, 6, 65), (1 << 23, 24, 1 << 28)):
            assert plan(lens, params) == (N.SDCAS_OK,) + R.chunk_plan(lens, params), (lens[:4], params)
    # a null parameter set is the default one; either output may be null
    lens = [5000, 70000]
    assert plan(lens, None) == (N.SDCAS_OK,) + R.chunk_plan(lens, R.DEFAULT_PARAMS)
    assert plan(lens, None, (False, True))[2] == R.chunk_plan(lens)[1]
    assert plan(lens, None, (True, False))[1] == R.chunk_plan(lens)[0]


def test_plan_refuses_invalid_parameters():
    bad = [(31, 8, 1024), (0, 8, 1024), (64, 5, 1024), (64, 25, 1 << 27), (256, 8, 1024), (300, 8, 1024),
           (64, 8, 256), (64, 8, 255), (64, 8, (1 << 28) + 1), (64, 0, 1024), (1 << 24, 24, 1 << 28)]
    for params in bad:
        assert not R.params_valid(params), params
        assert plan([100, 200], params)[0] == N.SDCAS_E_INVALID, params
        assert plan([], params)[0] == N.SDCAS_E_INVALID, params
    for params in ((32, 6, 65), (63, 6, 1 << 28), ((1 << 24) - 1, 24, (1 << 24) + 1)):
        assert R.params_valid(params) and plan([100], params)[0] == N.SDCAS_OK, params


def test_plan_capacity_without_data():
    # 2^30 chunks exactly is taken, one more is not: lengths alone, no content
    p = (32, 6, 65)
    assert plan([32 << 30], p) == (N.SDCAS_OK, 1 << 30, (1 << 25) + (1 << 30))
    assert plan([32 << 30, 1], p)[0] == N.SDCAS_E_CAPACITY
    assert plan([(32 << 30) + 1], p)[0] == N.SDCAS_E_CAPACITY
    assert plan([1 << 62] * 4, p)[0] == N.SDCAS_E_CAPACITY
    assert plan([(1 << 64) - 1] * 64, R.DEFAULT_PARAMS)[0] == N.SDCAS_E_CAPACITY
    from spacedrive_amd import Engine
    assert Engine.chunk_plan([5000, 70000], R.TEST_PARAMS) == R.chunk_plan([5000, 70000], R.TEST_PARAMS)
    for lens, params, code in (([32 << 30, 1], p, N.SDCAS_E_CAPACITY), ([1], (31, 8, 1024), N.SDCAS_E_INVALID)):
        try:
            Engine.chunk_plan(lens, params)
        except N.SdcasError as e:
            assert e.code == code
        else:
            raise AssertionError("chunk_plan accepted what it must refuse")


# ---- the tool and the C++ mirror ----------------------------------------------------------

def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_chunks.py"), "--count-only", "--files", "2000"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = json.loads(r.stdout.strip().splitlines()[-1])["model"]
    assert m["files"] == 2000 and m["max_chunks"] >= m["chunks"] > 2000
    b = m["bytes_chunk"]
    # at least four passes over the content: the gear read, the pack read and write, the hash read
    assert b["gear"] >= m["content_bytes"] and b["pack"] >= 2 * m["content_bytes"] and b["hash"] >= m["content_bytes"]
    assert m["passes_over_content"] >= 4 and m["ms_at_hbm_peak"]["chunk"] > m["ms_at_hbm_peak"]["hash"] > 0


def chunks_program():
    path = os.path.join(ROOT, "tests", "cpp", "build", "test_chunks")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "chunks.mk"], check=True)
    return path


def test_similarity_report_shaping_without_gpu():
    """similarity_report_from on hand-made rows, and what it refuses
    (tests/cpp/test_chunks.cpp without arguments)"""
    r = subprocess.run([chunks_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    hpp = open(os.path.join(ROOT, "include", "sdcore.hpp")).read()
    for name in ("Chunks chunk_messages", "Sharing chunk_sharing", "similarity_report_from", "similarity_report("):
        assert name in hpp, name


@pytest.mark.gpu
def test_similarity_report_on_both_libraries(tmp_path):
    """test_chunks --gpu DIR: similarity_report on a MemoryLibrary and a
    SqliteLibrary over files made here; the program checks that the two agree
    and that nothing is written, this test that the printed report is the
    checker's"""
    from tests._oracle import content, content_key
    a = content("synth", 0, 300000, content_key(0xCDC2, 1))
    files = {"a.bin": a,
             "b.bin": np.concatenate([a[:1000], np.array([0x42], np.uint8), a[1000:]]),
             "sub/c.bin": np.concatenate([a[:150000], content("synth", 0, 4000, content_key(0xCDC2, 2)), a[154000:]]),
             "sub/d.bin": content("synth", 0, 90000, content_key(0xCDC2, 3)),
             "empty.bin": np.zeros(0, np.uint8)}
    files["sub/e.bin"] = np.concatenate([a, files["sub/d.bin"]])
    (tmp_path / "loc" / "sub").mkdir(parents=True)
    for name, data in files.items():
        (tmp_path / "loc" / name).write_bytes(data.tobytes())
    r = subprocess.run([chunks_program(), "--gpu", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    pairs = {}
    for ln in lines:
        if ln.startswith("pair "):
            _, path, peer, shared, size = ln.split(" ")
            pairs[path] = (peer, int(shared), int(size))
    counts = [int(x) for x in [ln for ln in lines if ln.startswith("counts ")][0].split()[1:]]
    # the checker over the same contents in the rows' order (the walk's: a directory's entries by name,
    # directories after their own level): the first occurrence of a chunk is the lowest row's
    order = sorted(files)
    data = [files[k] for k in order]
    offs = np.r_[0, np.cumsum([d.size for d in data])[:-1]]
    w = R.chunk_files(data, offs, R.DEFAULT_PARAMS)
    rep = R.chunk_reps(np.concatenate(data), w["chunk_off"], w["chunk_len"])
    s = R.sharing(w["chunk_file"], w["chunk_len"], rep, len(data))
    assert counts == [w["counts"]["chunks"], s["counts"]["distinct_chunks"], s["counts"]["stored_bytes"],
                      s["counts"]["files_with_peer"]]
    want = {order[i]: (order[int(s["peer"][i])], int(s["peer_bytes"][i]), data[i].size)
            for i in range(len(order)) if s["peer"][i] >= 0}
    assert pairs == want and len(want) >= 3
    assert want["b.bin"][0] == "a.bin" and want["b.bin"][1] >= 0.9 * a.size
    # most shared bytes first, ties by the row's id
    listed = [ln.split(" ")[1] for ln in lines if ln.startswith("pair ")]
    assert listed == sorted(want, key=lambda k: (-want[k][1], order.index(k)))
