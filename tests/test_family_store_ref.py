"""The family store's plain reference (tests/_family_store_ref.py) against
rebuild_files and the header's worked example, and spacedrive_amd.recipes'
GPU-free store functions against both. No GPU."""
import numpy as np
import pytest

from spacedrive_amd.recipes import pack_store, rebuild_files, restore_from_store, store_layout
from tests import _family_recipes_ref as R
from tests import _family_store_ref as S


@pytest.fixture(scope="module")
def corpus():
    contents, fl, off, ln, rep, fam = R.versions(11, n_families=40, max_versions=6, blocks=30)
    rec = R.family_recipes(fl, off, ln, rep, fam)
    read = lambda row, at, n: contents[row][at:at + n]
    return contents, rec, read, rebuild_files(rec, read)


def test_worked_example():
    rec = R.family_recipes(**R.EXAMPLE)
    lay = S.layout(rec)
    assert [int(x) for x in lay["op_store_off"]] == S.EXAMPLE_STORE_OFF == [0, 0, 60, 30]
    assert lay["counts"]["store_bytes"] == S.EXAMPLE_STORE_BYTES == 65
    assert lay["counts"] == dict(ops=4, literal_ops=2, copy_ops=2, uncovered_ops=0, store_bytes=65, uncovered_bytes=0)
    got = store_layout(rec)
    assert np.array_equal(got["op_store_off"], lay["op_store_off"]) and got["counts"] == lay["counts"]


def test_reference_gives_every_file_back(corpus):
    contents, rec, read, rebuilt = corpus
    lay = S.layout(rec)
    total = sum(len(rebuilt[r]) for r in rebuilt)
    assert lay["counts"]["uncovered_ops"] == 0 and lay["counts"]["uncovered_bytes"] == 0
    assert lay["counts"]["store_bytes"] == rec["counts"]["literal_bytes"] < total
    store = S.pack_all(rec, lay, contents)
    assert len(store) == rec["counts"]["literal_bytes"]
    back = S.restore_all(rec, lay, store, [len(rebuilt[r]) for r in range(len(contents))])
    assert back == rebuilt
    assert all(back[r] == contents[r] for r in back if rec["row_ops"][r])


def test_recipes_functions_against_rebuild_files(corpus):
    contents, rec, read, rebuilt = corpus
    lay = store_layout(rec)
    want = S.layout(rec)
    assert np.array_equal(lay["op_store_off"], want["op_store_off"]) and lay["counts"] == want["counts"]
    assert lay["counts"]["uncovered_ops"] == 0
    assert lay["counts"]["store_bytes"] == rec["counts"]["literal_bytes"] < sum(len(b) for b in rebuilt.values())
    store = pack_store(rec, lay, read)
    assert store.tobytes() == bytes(S.pack_all(rec, want, contents))
    assert restore_from_store(rec, lay, store) == rebuilt
    some = [r for r in range(len(contents)) if rec["row_ops"][r]][3:9:2]
    assert restore_from_store(rec, lay, store, rows=some) == {r: rebuilt[r] for r in some}


def test_windows_and_pieces_in_the_reference(corpus):
    contents, rec, read, rebuilt = corpus
    lay = S.layout(rec)
    whole = S.pack_all(rec, lay, contents)
    n = len(contents)
    store = bytearray(len(whole))
    for first in range(0, n, 3):  # windows of three rows
        blob, at, ln = S.whole_rows(contents, range(first, min(first + 3, n)), gap=5)
        S.move(rec, lay["op_store_off"], at, None, ln, blob, store, False, 8192)
    assert store == whole
    store = bytearray(len(whole))
    for pos in range(0, max(len(c) for c in contents), 1000):  # every row in pieces of 1000 bytes
        pieces = [c[pos:pos + 1000] for c in contents]
        blob, at, ln = S.whole_rows(pieces)
        S.move(rec, lay["op_store_off"], at, np.full(n, pos, np.uint64), ln, blob, store, False, 8192)
    assert store == whole


def test_uncovered_and_bad_ops_in_the_reference():
    rec = {k: np.array(v) for k, v in R.EXAMPLE_OPS.items()}
    rec["chunk_op"] = np.array(R.EXAMPLE_REST["chunk_op"])
    rec["op_src_off"] = np.array([0, 40, 30, 30], np.uint64)  # op 1 now reads [40, 70) of a literal of 60
    lay = S.layout(rec)
    assert [int(x) for x in lay["op_store_off"]] == [0, S.NONE, 60, 30]
    assert lay["counts"]["uncovered_ops"] == 1 and lay["counts"]["uncovered_bytes"] == 30
    got = store_layout(rec)
    assert np.array_equal(got["op_store_off"], lay["op_store_off"]) and got["counts"] == lay["counts"]
    # a row out of range and a store range past the store are bad; the other ops move
    rec["op_row"] = np.array([0, 1, 7, 1], np.uint32)
    blob, store = bytearray(200), bytearray(b"\x11" * 65)
    c = S.move(rec, lay["op_store_off"], [0, 100], None, [60, 65], blob, store, True, 8192, store_bytes=50)
    assert c == dict(ops_moved=0, bytes_moved=0, bad_ops=3, tiles=0)
    c = S.move(rec, lay["op_store_off"], [0, 100], None, [60, 65], blob, store, True, 8192)
    assert c == dict(ops_moved=2, bytes_moved=90, bad_ops=1, tiles=2)
    assert blob[:60] == b"\x11" * 60 and blob[135:165] == b"\x11" * 30 and blob[100:135] == bytes(35)
