"""Duplicates confirmed by checksum, the host layers: the two entry points in
the header, the binding and the library, and the C++ mirror through its test
program (tests/cpp/test_confirm.cpp): the report's shaping and
Library::file_paths_with_checksum without a GPU, and on the GPU the
identifier job with checksums followed by confirm_duplicates on a
MemoryLibrary and a SqliteLibrary."""
import ctypes
import os
import re
import subprocess

import pytest

from spacedrive_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
SYMBOLS = ("sdcas_confirm_duplicates", "sdcas_dev_confirm_duplicates")


def _bin(name):
    path = os.path.join(BUILD, name)
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "confirm.mk"], check=True)
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


def test_constants_and_counts_layout():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    for name, value in (("DUPLICATE", 1), ("COLLISION", 2), ("SKIPPED", 4)):
        assert re.search(r"#define SDCAS_CONFIRM_%s\s+%du\b" % (name, value), hdr), name
        assert getattr(N, "SDCAS_CONFIRM_" + name) == value
    body = re.search(r"typedef struct sdcas_confirm_counts \{(.*?)\} sdcas_confirm_counts;", hdr, re.S).group(1)
    fields = re.findall(r"uint64_t (\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["files", "classes", "keys", "collided_keys", "collided_files", "duplicate_files"]
    assert [f for f, _ in N.ConfirmCounts._fields_] == fields
    assert ctypes.sizeof(N.ConfirmCounts) == 48


def test_abi_version_is_still_7():
    """new symbols alone are a compatible change: callers probe for them"""
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    assert "#define SDCAS_ABI_VERSION 7" in hdr
    assert N.SDCAS_ABI_VERSION == 7 and N.load().sdcas_abi_version() == 7
    assert "added after abi 7; probe for the symbol" in hdr.lower()


def test_engine_methods_exist():
    from spacedrive_amd import Engine
    for name in ("confirm_duplicates", "dev_confirm_duplicates", "identify_confirmed"):
        assert callable(getattr(Engine, name)), name


def test_argument_checks_need_no_device():
    """a null context is refused before anything touches the GPU"""
    L = N.load()
    assert L.sdcas_confirm_duplicates(None, None, None, None, 0, None, None, None, None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_confirm_duplicates(None, None, None, None, 0, None, None, None, None, None) == N.SDCAS_E_INVALID


def test_report_and_library_query_without_gpu():
    """duplicate_report_from against a std::map group-by, and
    file_paths_with_checksum on a MemoryLibrary and a SqliteLibrary(":memory:")
    over 31 hand-built rows"""
    r = subprocess.run([_bin("test_confirm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_job_links_the_collision_and_the_report_names_it(tmp_path):
    """real files: the identifier job with checksums links the pair that
    shares a cas_id to ONE Object; confirm_duplicates lists it under
    collisions with that Object and two classes, the identical sets under
    confirmed, on both libraries, and leaves every row as it was"""
    r = subprocess.run([_bin("test_confirm"), "--gpu", str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
