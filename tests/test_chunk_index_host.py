"""The chunk index, the host layers: the entry points in the header, the binding
and the library, the C++ mirror's SQLite tables (no GPU), the tool's model, and
— on the GPU — similarity_report_indexed over files that arrive in three steps.
The kernels' tests are tests/test_gpu_chunk_index.py and
tests/test_gpu_similar_indexed.py."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from spacedrive_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_chunk_index_dir_bits": 1, "sdcas_chunk_index_check": 6, "sdcas_chunk_index_match": 14,
           "sdcas_dev_chunk_index_match": 15, "sdcas_chunk_index_add": 20, "sdcas_dev_chunk_index_add": 21}


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sdcas_\w+)", out))
    for name, nargs in SYMBOLS.items():
        assert name in N.ABI_SYMBOLS and name in exported
        assert len(getattr(N.load(), name).argtypes) == nargs, name
        assert re.search(r"\b(int|uint32_t) %s\(" % name, hdr), name
    assert "#define SDCAS_ABI_VERSION 7" in hdr and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("chunk index: a batch's chunks against the chunks stored before"):]
    assert "added after abi 7; probe for the symbol" in section[:300].lower()
    assert (N.SDCAS_INDEX_HIT, N.SDCAS_INDEX_ADDED, N.SDCAS_INDEX_SKIPPED) == (1, 2, 4)
    for name, v in (("SDCAS_INDEX_HIT", 1), ("SDCAS_INDEX_ADDED", 2), ("SDCAS_INDEX_SKIPPED", 4)):
        assert re.search(r"#define %s\s+%du" % (name, v), hdr), name


def test_a_null_context_is_refused_without_a_device():
    L = N.load()
    assert L.sdcas_chunk_index_match(*([None] * 5), 0, 0, None, None, None, 0, None, None, None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_chunk_index_match(*([None] * 5), 0, 0, None, None, None, 0, None, None, None,
                                         None) == N.SDCAS_E_INVALID
    assert L.sdcas_chunk_index_add(*([None] * 5), 0, 0, None, None, None, None, 0, None, None, None, None, 0, None,
                                   None, None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_chunk_index_add(*([None] * 5), 0, 0, None, None, None, None, 0, None, None, None, None, 0, None,
                                       None, None, None) == N.SDCAS_E_INVALID


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_ci_match", "k_ci_select", "k_ci_fix", "k_ci_place_new", "k_ix_place_old", "k_ci_add_out", "k_ix_dir"):
        assert k in out, k


def test_engine_and_index_methods_exist():
    from spacedrive_amd import ChunkIndex, Engine
    for name in ("chunk_index_dir_bits", "chunk_index_check", "chunk_index_match", "dev_chunk_index_match",
                 "chunk_index_add", "dev_chunk_index_add", "similar_files_indexed"):
        assert callable(getattr(Engine, name)), name
    for name in ("match", "add", "arrays", "save", "load"):
        assert callable(getattr(ChunkIndex, name)), name


def index_program():
    path = os.path.join(ROOT, "tests", "cpp", "build", "test_chunk_index")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "chunkindex.mk"], check=True)
    return path


def test_cpp_tables_without_gpu():
    """SqliteLibrary's chunk_index / chunk_indexed_file: the round trip, the
    order of digests from 0x00.. to 0xff.., refused appends, a spoiled table
    (tests/cpp/test_chunk_index.cpp without arguments)"""
    r = subprocess.run([index_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    hpp = open(os.path.join(ROOT, "include", "sdcore.hpp")).read()
    for name in ("struct ChunkIndexData", "IndexMatch chunk_index_match(", "IndexAdd chunk_index_add(",
                 "load_chunk_index()", "append_chunk_index(", "similarity_report_indexed("):
        assert name in hpp, name


def test_tool_prints_its_model_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_chunk_index.py"), "--count-only"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    models = json.loads(r.stdout.strip().splitlines()[-1])["model"]
    assert [m["n"] for m in models] == [1 << 22, 1 << 24, 1 << 26] and all(m["m"] == 1 << 20 for m in models)
    assert [m["bits"] for m in models] == [20, 22, 24] and all(m["entries_per_bucket"] == 4 for m in models)
    assert models[2]["copy_bytes_each_way"] == 48 << 26 and models[0]["confirm_pairs"] == (1 << 22) + (1 << 20)


@pytest.mark.gpu
def test_cpp_indexed_report_over_three_steps(tmp_path):
    """test_chunk_index --gpu DIR: the files of step1, step2 and step3 arrive
    one step at a time; the union of similarity_report_indexed's reports equals
    similarity_report_streamed over all of them, and a further run is idle"""
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, 500000, dtype=np.uint8)
    c = rng.integers(0, 256, 60000, dtype=np.uint8)
    steps = {
        "step1": {"a.bin": a, "c.bin": c, "empty.bin": np.zeros(0, np.uint8)},
        "step2": {"b.bin": np.concatenate([a[:1000], np.array([0x42], np.uint8), a[1000:]]),  # a, one byte inserted
                  "d.bin": rng.integers(0, 256, 5000, dtype=np.uint8), "a_copy.bin": a},
        "step3": {"e.bin": np.concatenate([c, a[:250000]]),  # the whole of c, half of a
                  "f.bin": np.concatenate([rng.integers(0, 256, 20000, dtype=np.uint8), c[10000:]])},
    }
    (tmp_path / "loc").mkdir()
    for step, files in steps.items():
        (tmp_path / step).mkdir()
        for name, data in files.items():
            (tmp_path / step / name).write_bytes(data.tobytes())
    r = subprocess.run([index_program(), "--gpu", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert int(re.search(r"^pairs (\d+)", r.stdout, re.M).group(1)) >= 4
