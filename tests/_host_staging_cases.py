"""The inputs of tests/test_gpu_host_staging.py and what the suites' CPU
references make of them. One case per host-array entry point, built once and
shared: read, never written. The references are the checkers the other suites
use: the oracle (the identifier job, BLAKE3), tests/_tree_ref.py,
tests/_cdc_ref.py, tests/_chunk_index_ref.py, tests/_chunk_holders_ref.py, and
the dict-based group-bys of tests/test_gpu_confirm.py and
tests/test_gpu_dupsets.py."""
import functools

import numpy as np

from tests import _cdc_ref as C
from tests import _chunk_holders_ref as H
from tests import _chunk_index_ref as R
from tests import _tree_ref as T
from tests._oracle import mix64
from tests.test_gpu_confirm import digests_of, group_by, shuffled_classes
from tests.test_gpu_dupsets import group_sets

FILE_SIZES = (0, 31, 32, 4096, 70000, 32)
EDGES = (1, 2, 15, 16, 17)  # byte-sized parts end off a 16-byte boundary; n / 2 set slots is 0 or odd
REMOVED = np.array([3], np.uint64)  # the holders index forgets file 2 (its chunks carry the value file + 1)


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def confirm_case(n):
    """-> (keys, digests [n, 32], valid, group_by's answer): pairs of equal
    files; from three files on the first is not valid"""
    ids = np.arange(n, dtype=np.uint64) // np.uint64(2)
    keys, dig = mix64(ids + np.uint64(77)), digests_of(ids + np.uint64(900))
    valid = np.ones(n, np.uint8)
    if n > 2:
        valid[0] = 0
    _ro(keys, dig, valid)
    return keys, dig, valid, group_by(keys, dig, valid)


@functools.lru_cache(maxsize=None)
def big_confirm_case():
    """5000 files over 700 keys, up to three digests per key, no valid array"""
    keys, dig = shuffled_classes(5000, 700, 5)
    _ro(keys, dig)
    return keys, dig, None, group_by(keys, dig)


@functools.lru_cache(maxsize=None)
def sets_case(n):
    """-> (rep, sizes, group_sets' answer in the order by rep): confirm_case's rep"""
    rep = confirm_case(n)[3][0].copy()
    sizes = np.arange(n, dtype=np.uint64) * np.uint64(10) + np.uint64(7)
    _ro(rep, sizes)
    return rep, sizes, group_sets(rep, sizes)


@functools.lru_cache(maxsize=None)
def top_case(n):
    """-> (parent, rep, tree_top's answer). n == 1000: a random tree with
    labels from a small pool; else entry 0 above all others, confirm_case's rep"""
    if n == 1000:
        parent, _ = T.random_tree(n, 11)
        rep = np.random.default_rng(12).integers(-1, 300, n).astype(np.int64)
    else:
        parent = np.r_[-1, np.zeros(n - 1, np.int64)].astype(np.int64)
        rep = confirm_case(n)[3][0].copy()
    _ro(parent, rep)
    return parent, rep, T.tree_top(parent, rep)


@functools.lru_cache(maxsize=None)
def tree_case(oracle):
    """seven entries: a root with the directories 1 and 4, which hold equal
    files under equal names -> (parent, is_dir, name32, digests, valid, sizes,
    keys, tree_digests' answer with the three optional arrays, and without)"""
    parent = np.array([-1, 0, 1, 1, 0, 4, 4], np.int64)
    is_dir = np.array([1, 1, 0, 0, 1, 0, 0], np.uint8)
    name32 = digests_of(np.array([50, 51, 60, 61, 52, 60, 61], np.uint64)).reshape(-1).copy()
    digests = digests_of(np.array([0, 0, 70, 71, 0, 70, 71], np.uint64)).copy()
    digests[is_dir != 0] = 0
    valid = np.array([0, 0, 1, 1, 0, 1, 1], np.uint8)
    sizes = np.array([0, 0, 100, 2000, 0, 100, 2000], np.uint64)
    keys = np.where(is_dir != 0, 0, mix64(np.arange(7, dtype=np.uint64) % np.uint64(3))).astype(np.uint64)
    _ro(parent, is_dir, name32, digests, valid, sizes, keys)
    return (parent, is_dir, name32, digests, valid, sizes, keys,
            T.tree_digests(oracle, parent, is_dir, name32, digests, valid, sizes, keys),
            T.tree_digests(oracle, parent, is_dir, name32, digests))


@functools.lru_cache(maxsize=None)
def dedup_case(oracle):
    """17 orphans, 3 existing Objects -> (keys, has_key, status, existing,
    the identifier job's (link, created, linked, window))"""
    pool = mix64(np.arange(6, dtype=np.uint64) + np.uint64(1234))
    keys = pool[np.array([0, 1, 0, 2, 3, 1, 4, 4, 5, 0, 2, 2, 3, 5, 1, 4, 0])]
    has = np.ones(17, np.uint8)
    has[6] = 0
    status = np.zeros(17, np.int32)
    status[12] = 5
    existing = np.r_[pool[1], pool[5], mix64(np.uint64(99))].astype(np.uint64)
    _ro(keys, has, status, existing)
    return keys, has, status, existing, oracle.identifier_job(keys, has, status, 100, existing)


@functools.lru_cache(maxsize=None)
def files():
    """six files of FILE_SIZES bytes. The last equals the third; the 70000
    bytes are 25000 random ones twice and 20000 more, so its cuts repeat"""
    rng = np.random.default_rng(2024)
    out = [rng.integers(0, 256, s, dtype=np.uint8) for s in FILE_SIZES[:4]]
    a = rng.integers(0, 256, 25000, dtype=np.uint8)
    out.append(np.concatenate([a, a, rng.integers(0, 256, 20000, dtype=np.uint8)]))
    out.append(out[2].copy())
    assert tuple(f.size for f in out) == FILE_SIZES
    return tuple(_ro(*out))


@functools.lru_cache(maxsize=None)
def chunk_case(oracle):
    """the files three bytes apart in one blob -> dict: blob, offsets, lens,
    chunk_files' answer ("chunks"), the chunks' keys and digests (BLAKE3 of
    their bytes, the key its first eight bytes), their rep and sharing's answer"""
    fs = files()
    lens = np.array([f.size for f in fs], np.uint64)
    offs = (np.r_[0, np.cumsum(lens[:-1])] + 3 * np.arange(1, len(fs) + 1)).astype(np.uint64)
    blob = np.full(int(offs[-1] + lens[-1]) + 5, 0xA5, np.uint8)
    for f, o in zip(fs, offs):
        blob[int(o):int(o) + f.size] = f
    ch = C.chunk_files(fs, offs)
    m = ch["counts"]["chunks"]
    dig = np.zeros((m, 32), np.uint8)
    for c, (o, n) in enumerate(zip(ch["chunk_off"], ch["chunk_len"])):
        dig[c] = np.frombuffer(bytes.fromhex(oracle.hash(blob[int(o):int(o) + int(n)].tobytes())), np.uint8)
    keys = np.array([R.real_key(d) for d in dig], np.uint64)
    rep = C.chunk_reps(blob, ch["chunk_off"], ch["chunk_len"])
    _ro(blob, offs, lens, dig, keys, rep)
    return {"blob": blob, "offsets": offs, "lens": lens, "chunks": ch, "keys": keys, "digests": dig, "rep": rep,
            "sharing": C.sharing(ch["chunk_file"], ch["chunk_len"], rep, len(fs))}


@functools.lru_cache(maxsize=None)
def index_case(oracle):
    """the chunk index of the first five chunks (into an empty index), all
    chunks matched against it; the holders index of all chunks with the value
    file + 1, all chunks matched against it, REMOVED taken out -> dict"""
    c = chunk_case(oracle)
    keys, dig = c["keys"], c["digests"]
    values = c["chunks"]["chunk_file"].astype(np.uint64) + np.uint64(1)
    _ro(values)
    m = keys.size
    first = R.add([], keys[:5], dig[:5], values[:5])
    held = H.add([], keys, dig, values)
    return {"keys": keys, "digests": dig, "values": values,
            "empty": R.arrays([], 0), "bits5": R.dir_bits(5), "add5": first,
            "match": R.match(first[0], keys, dig),
            "bits_held": R.dir_bits(m), "held": held, "held_match": H.match(held[0], keys, dig),
            "removed": H.remove(held[0], REMOVED)}
