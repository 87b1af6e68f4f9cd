"""The holders index's reference (tests/_chunk_holders_ref.py) held to its own
laws on random and forged inputs, and the GPU-free check of the library held to
the reference, so that the GPU tests rest on something checked here."""
import numpy as np
import pytest

from spacedrive_amd import Engine, _native as N
from tests import _chunk_holders_ref as H
from tests import _chunk_index_ref as R


def corpus(seed, n_files=12, n_chunks=60, forged=False):
    """file id -> list of (key, digest) with heavy sharing: a few chunks are in
    almost every file (the all-zero chunk, a template header), most in two or
    three, some twice in one file"""
    rng = np.random.default_rng(seed)
    keys, dig = R.random_pairs(rng, n_chunks, forged_key=0xF00D if forged else None)
    files = {}
    for f in range(n_files):
        pick = list(rng.integers(0, n_chunks, rng.integers(0, 25)))
        if rng.random() < 0.8:
            pick += [0, 1, 0]
        files[10 + 3 * f] = [(int(keys[c]), dig[c].tobytes()) for c in pick]
    return files


def batch_of(files, ids):
    ts = [(k, d, f) for f in ids for k, d in files[f]]
    return H.batch_arrays(ts)


def build_from(files, ids):
    return H.build(*batch_of(files, ids))


@pytest.mark.parametrize("seed", range(6))
def test_remove_equals_the_index_of_the_files_that_remain(seed):
    """law (a), and law (e): match after the remove as on the rebuilt index"""
    files = corpus(seed, forged=seed % 3 == 2)
    ids = sorted(files)
    full = build_from(files, ids)
    assert H.check(full) == (0, None)
    rng = np.random.default_rng(100 + seed)
    gone = sorted(int(x) for x in rng.permutation(ids)[:rng.integers(0, len(ids) + 1)])
    left, counts = H.remove(full, gone + [5, 10 ** 9])  # ids nobody holds change nothing
    rebuilt = build_from(files, [f for f in ids if f not in gone])
    assert left == rebuilt and H.check(left) == (0, None)
    assert counts == dict(entries_old=len(full), removed=len(full) - len(rebuilt), entries_new=len(rebuilt),
                          values=len(gone) + 2)
    qk, qd, _ = batch_of(files, ids)
    a, b = H.match(left, qk, qd), H.match(rebuilt, qk, qd)
    assert all((x == y).all() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    for (k, d, f), p, v, h in zip(H.triples(*batch_of(files, ids)), *a[:3]):
        holders = sorted(g for g in ids if g not in gone and (k, d) in files[g])
        assert h == len(holders) and v == (holders[0] if holders else 0) and (p >= 0) == bool(holders)
        if holders:
            assert left[p][:2] == (k, d) and (p == 0 or left[p - 1][:2] != (k, d))


@pytest.mark.parametrize("seed", range(4))
def test_add_then_remove_is_the_identity(seed):
    """law (b)"""
    files = corpus(seed)
    ids = sorted(files)
    base = build_from(files, ids[:-1])
    new, pos, flags, counts = H.add(base, *batch_of(files, ids[-1:]))
    assert counts["hits"] == 0 and counts["added"] == len(set(files[ids[-1]]))
    assert H.remove(new, ids[-1:])[0] == base
    # adding it again: every triple is a hit, nothing changes
    again, _, flags, counts = H.add(new, *batch_of(files, ids[-1:]))
    assert again == new and (flags == H.HIT).all() and counts["hits"] == counts["queries"]


@pytest.mark.parametrize("seed", range(4))
def test_any_split_and_any_order_give_one_index(seed):
    """law (c)"""
    files = corpus(seed, forged=seed == 3)
    ids = sorted(files)
    keys, dig, vals = batch_of(files, ids)
    want = H.build(keys, dig, vals)
    rng = np.random.default_rng(200 + seed)
    m = len(keys)
    for trial in range(4):
        p = rng.permutation(m) if trial % 2 else np.arange(m)
        cuts = [0] + sorted(int(c) for c in rng.integers(0, m + 1, 3)) + [m]
        ix = []
        for lo, hi in zip(cuts, cuts[1:]):
            before = len(ix)
            ix, pos, flags, counts = H.add(ix, keys[p[lo:hi]], dig[p[lo:hi]], vals[p[lo:hi]])
            assert counts["entries_new"] == before + counts["added"] == len(ix)
            assert counts["queries"] == counts["hits"] + counts["added"] + counts["batch_duplicates"]
            ts = H.triples(keys[p[lo:hi]], dig[p[lo:hi]], vals[p[lo:hi]])
            assert all(ix[q] == t for q, t in zip(pos, ts))
            first = {}
            for c, t in enumerate(ts):
                first.setdefault(t, c)
            assert all((flags[c] == H.ADDED) == (first[t] == c) for c, t in enumerate(ts) if flags[c] != H.HIT)
        assert ix == want


def test_a_chunk_index_is_a_holders_index():
    """law (d): strict in the pair implies strict in the triple, for the
    reference and for the library's GPU-free check"""
    rng = np.random.default_rng(7)
    keys, dig = R.random_pairs(rng, 300)
    keys[:40] = keys[0]  # one key, many digests
    pick = rng.integers(0, 300, 700)
    entries = R.build(keys[pick], dig[pick], rng.integers(0, 50, 700).astype(np.uint64))
    assert H.check(entries) == (0, None)
    for bits in (0, 3, R.dir_bits(len(entries))):
        k, d, v, dr, _ = R.arrays(entries, bits)
        assert Engine.chunk_index_check(k, d, dr, bits) == (N.SDCAS_OK, None)
        assert Engine.chunk_holders_check(k, d, v, dr, bits) == (N.SDCAS_OK, None)
    # a holders index with a repeated pair is no chunk index
    files = corpus(1)
    full = build_from(files, sorted(files))
    k, d, v, dr, _ = H.arrays(full, 2)
    assert Engine.chunk_holders_check(k, d, v, dr, 2) == (N.SDCAS_OK, None)
    assert Engine.chunk_index_check(k, d, dr, 2)[0] == N.SDCAS_E_INVALID


def test_the_library_check_agrees_with_the_reference_on_spoiled_indexes():
    rng = np.random.default_rng(8)
    files = corpus(2)
    full = build_from(files, sorted(files))
    for _ in range(30):
        bad = list(full)
        i, j = (int(x) for x in rng.integers(0, len(bad), 2))
        bad[i], bad[j] = bad[j], bad[i]
        k, d, v, _, _ = H.arrays(bad, 0)
        dr = np.array(H.directory(full, 3), np.uint32)
        if rng.random() < 0.3:
            dr[int(rng.integers(0, 9))] += 1
        rc, where = H.check(bad, dr, 3)
        got = Engine.chunk_holders_check(k, d, v, dr, 3)
        assert got == ((N.SDCAS_OK, None) if rc == 0 else (N.SDCAS_E_INVALID, where))
