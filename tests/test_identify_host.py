"""The host layers of the one-pass cas_id + checksum through their C++ test
programs: sdcas_identify_checksums' GPU-free open helper, which never opens a
FIFO (tests/cpp/test_identify_io.cpp), the identifier job's `checksums` flag
over synthetic metadata (tests/cpp/test_identify_job.cpp, no GPU), and on the
GPU the job with the flag against the job followed by the object validator."""
import ctypes
import os
import subprocess

import pytest

from spacedrive_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")


def _bin(name):
    path = os.path.join(BUILD, name)
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "identify.mk"], check=True)
    return path


def test_new_entry_points_are_exported_and_bound():
    assert N.SDCAS_ABI_VERSION == 7 and N.SDCAS_META_HAS_CHECKSUM == 4
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ("sdcas_dev_identify", "sdcas_identify_checksums"):
        assert name in N.ABI_SYMBOLS
        assert getattr(lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    assert "#define SDCAS_ABI_VERSION 7" in hdr and "#define SDCAS_META_HAS_CHECKSUM 4u" in hdr
    from spacedrive_amd import Engine
    assert callable(Engine.identify_checksums) and callable(Engine.dev_identify)


def test_open_helper_never_opens_a_fifo(tmp_path):
    """a FIFO without a writer: size 0, status 0, no kind of file to read —
    and the call returns (the program gives it 5 s on a worker thread)"""
    r = subprocess.run([_bin("test_identify_io"), str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_job_flag_without_gpu():
    """FileIdentifierJobInit::checksums over a synthetic MetadataFn: set, exactly
    the rows the steps read get the checksum (the reread row too); clear, the
    library ends as it does today"""
    r = subprocess.run([_bin("test_identify_job")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_job_with_checksums_equals_job_then_validator(tmp_path):
    """~300 small files with duplicates and empty files: every file_path row
    (cas_id, object_id, integrity_checksum) and the Object count identical"""
    r = subprocess.run([_bin("test_identify_job"), "--gpu", str(tmp_path)], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
