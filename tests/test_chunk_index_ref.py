"""CPU tests of the chunk index's definition: the Python reference
(tests/_chunk_index_ref.py) against brute force, and the library's GPU-free
helpers sdcas_chunk_index_dir_bits / sdcas_chunk_index_check against it."""
import ctypes

import numpy as np
import pytest

from spacedrive_amd import Engine, _native as N
from tests import _chunk_index_ref as R


def small_batch(rng, m, distinct):
    """m pairs drawn from `distinct` random ones, a few keys forged to collide"""
    keys, dig = R.random_pairs(rng, distinct)
    keys[: distinct // 4] = keys[0]  # one key, several digests
    pick = rng.integers(0, distinct, m)
    return keys[pick], dig[pick]


def test_reference_against_brute_force():
    rng = np.random.default_rng(1)
    keys, dig = small_batch(rng, 200, 60)
    values = np.arange(1000, 1200, dtype=np.uint64)
    valid = (rng.random(200) > 0.2).astype(np.uint8)
    half = R.build(keys[:100], dig[:100], values[:100], valid[:100])
    new, pos, flags, counts = R.add(half, keys[100:], dig[100:], values[100:], valid[100:])
    # brute force: every valid pair, the first position that holds it
    first = {}
    ps = R.pairs(keys, dig)
    for c, p in enumerate(ps):
        if valid[c] and p not in first:
            first[p] = c
    want = sorted((k, d, 1000 + c) for (k, d), c in first.items())
    assert new == want
    assert all(new[i][:2] < new[i + 1][:2] for i in range(len(new) - 1))
    for c in range(100, 200):
        j = c - 100
        if not valid[c]:
            assert (pos[j], flags[j]) == (-1, R.SKIPPED)
            continue
        assert new[pos[j]][:2] == ps[c]
        f = first[ps[c]]
        assert flags[j] == (R.HIT if f < 100 else R.ADDED if f == c else 0)
    assert counts["queries"] == counts["hits"] + counts["added"] + counts["batch_duplicates"] == int(valid[100:].sum())
    assert (counts["entries_old"], counts["entries_new"]) == (len(half), len(want))
    # match: a linear scan
    mpos, mval, mcounts = R.match(half, keys, dig, valid)
    for c, p in enumerate(ps):
        hit = [i for i, e in enumerate(half) if e[:2] == p]
        if not valid[c]:
            assert (mpos[c], mval[c]) == (-1, 0)
        elif hit:
            assert mpos[c] == hit[0] and mval[c] == half[hit[0]][2]
        else:
            assert (mpos[c], mval[c]) == (-1, 0)
    assert mcounts["queries"] + mcounts["skipped"] == 200 and mcounts["hits"] + mcounts["misses"] == mcounts["queries"]
    # the directory: a count per slot
    for bits in (0, 1, 3, 6):
        d = R.directory(new, bits)
        assert len(d) == (1 << bits) + 1 and d[-1] == len(new)
        for j in range(1 << bits):
            assert d[j] == sum(1 for e in new if bits and (e[0] >> (64 - bits)) < j)


def test_dir_bits():
    want = {0: 0, 1: 0, 7: 0, 8: 1, 9: 2, 16: 2, 17: 3, 1000: 8, 1024: 8, 1025: 9, 1 << 20: 18, (1 << 20) + 1: 19,
            1 << 30: 28, 1 << 40: 28}
    for n, b in want.items():
        assert R.dir_bits(n) == b, n
        assert Engine.chunk_index_dir_bits(n) == b, n


def ref_index(n, seed=2):
    rng = np.random.default_rng(seed)
    keys, dig = R.random_pairs(rng, n)
    if n >= 3:
        keys[:3] = keys[0]  # a run of one key ordered by the digests
    return R.build(keys, dig, np.arange(n, dtype=np.uint64))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 8, 9, 1000])
def test_check_accepts_reference_indexes(n):
    entries = ref_index(n)
    assert len(entries) == n
    for bits in sorted({0, R.dir_bits(n), 3}):
        keys, dig, _, d, _ = R.arrays(entries, bits)
        assert Engine.chunk_index_check(keys, dig, d, bits) == (N.SDCAS_OK, None), bits


def check(keys, dig, d, bits):
    return Engine.chunk_index_check(keys, dig, d, bits)


def test_check_rejects_and_names_the_place():
    entries = ref_index(100)
    bits = 3
    keys, dig, _, d, _ = R.arrays(entries, bits)
    # two entries swapped: entry 41 no longer orders after entry 40
    k2, d2 = keys.copy(), dig.copy()
    k2[[40, 41]], d2[[40, 41]] = keys[[41, 40]], dig[[41, 40]]
    assert check(k2, d2, d, bits) == (N.SDCAS_E_INVALID, 41)
    # a pair twice
    k2, d2 = keys.copy(), dig.copy()
    k2[60], d2[60] = keys[59], dig[59]
    assert check(k2, d2, d, bits) == (N.SDCAS_E_INVALID, 60)
    # a directory slot off by one, and a last slot that is not n
    for slot in (1, 5):
        e = d.copy()
        e[slot] += 1
        assert check(keys, dig, e, bits) == (N.SDCAS_E_INVALID, slot)
    e = d.copy()
    e[-1] -= 1
    assert check(keys, dig, e, bits) == (N.SDCAS_E_INVALID, 1 << bits)
    assert check(keys, dig, d, bits) == (N.SDCAS_OK, None)


def test_check_orders_digests_by_bytes_not_by_words():
    """bytes 0..3 = 00 00 00 01 order before 01 00 00 00 (memcmp); as
    little-endian words they are 0x01000000 and 0x00000001, the other way round"""
    a = np.zeros(32, np.uint8)
    b = np.zeros(32, np.uint8)
    a[3], b[0] = 1, 1
    keys = np.array([5, 5], np.uint64)
    d = np.array([0, 2], np.uint32)
    assert check(keys, np.stack([a, b]), d, 0) == (N.SDCAS_OK, None)
    assert check(keys, np.stack([b, a]), d, 0) == (N.SDCAS_E_INVALID, 1)
    assert R.build(keys, np.stack([b, a]), [7, 8]) == [(5, a.tobytes(), 8), (5, b.tobytes(), 7)]


def test_check_capacity_before_any_array_is_touched():
    L = N.load()
    bad = ctypes.c_uint64(123)
    assert L.sdcas_chunk_index_check(None, None, None, 0, 29, ctypes.byref(bad)) == N.SDCAS_E_CAPACITY
    assert L.sdcas_chunk_index_check(None, None, None, (1 << 30) + 1, 0, ctypes.byref(bad)) == N.SDCAS_E_CAPACITY
    assert bad.value == 123
    # a NULL array that is needed
    assert L.sdcas_chunk_index_check(None, None, None, 0, 0, None) == N.SDCAS_E_INVALID
