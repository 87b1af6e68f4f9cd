"""Test infrastructure: the chunk index (include/sdcas.h) in plain Python. An
index is a list of (key, digest bytes, value) tuples, strictly ascending in
(key, digest) — Python compares ints as unsigned and bytes as memcmp does — and
everything is a dict or a bisect over it. Every comparison against the library
is exact equality."""
import bisect

import numpy as np

HIT, ADDED, SKIPPED = 1, 2, 4


def dir_bits(n):
    """the recommended directory width: 0 below 8 entries, else
    min(28, ceil_log2(n) - 2)"""
    if n < 8:
        return 0
    return min(28, (n - 1).bit_length() - 2)


def pairs(keys, digests):
    """[(key, digest bytes)] of a batch"""
    dig = np.ascontiguousarray(digests, np.uint8).reshape(-1, 32)
    return [(int(k), dig[i].tobytes()) for i, k in enumerate(np.asarray(keys, np.uint64))]


def build(keys, digests, values, valid=None):
    """the index of a batch alone: its distinct valid pairs, sorted, each with
    the value of the lowest position that holds it"""
    return add([], keys, digests, values, valid)[0]


def directory(entries, bits):
    """dir[j] = the entries whose key's top `bits` bits are below j"""
    ks = [e[0] for e in entries]
    out = [bisect.bisect_left(ks, j << (64 - bits)) if bits else 0 for j in range(1 << bits)]
    return out + [len(entries)]


def match(entries, keys, digests, valid=None):
    """-> (pos, value, counts)"""
    where = {(k, d): i for i, (k, d, _) in enumerate(entries)}
    pos, value = [], []
    counts = dict(queries=0, hits=0, misses=0, skipped=0)
    for c, p in enumerate(pairs(keys, digests)):
        if valid is not None and not valid[c]:
            pos.append(-1), value.append(0)
            counts["skipped"] += 1
            continue
        counts["queries"] += 1
        i = where.get(p, -1)
        counts["hits" if i >= 0 else "misses"] += 1
        pos.append(i), value.append(entries[i][2] if i >= 0 else 0)
    return np.array(pos, np.int64).reshape(-1), np.array(value, np.uint64).reshape(-1), counts


def add(entries, keys, digests, values, valid=None):
    """-> (new entries, pos, flags, counts)"""
    old = {(k, d): v for k, d, v in entries}
    new, flags = dict(old), []
    counts = dict(queries=0, hits=0, added=0, batch_duplicates=0, entries_old=len(entries), entries_new=0)
    ps = pairs(keys, digests)
    for c, p in enumerate(ps):
        if valid is not None and not valid[c]:
            flags.append(SKIPPED)
            continue
        counts["queries"] += 1
        if p in old:
            flags.append(HIT)
            counts["hits"] += 1
        elif p in new:
            flags.append(0)
            counts["batch_duplicates"] += 1
        else:
            new[p] = int(values[c]) if values is not None else 0
            flags.append(ADDED)
            counts["added"] += 1
    out = sorted((k, d, v) for (k, d), v in new.items())
    counts["entries_new"] = len(out)
    where = {(k, d): i for i, (k, d, _) in enumerate(out)}
    pos = [where[p] if flags[c] != SKIPPED else -1 for c, p in enumerate(ps)]
    return out, np.array(pos, np.int64).reshape(-1), np.array(flags, np.uint8).reshape(-1), counts


def arrays(entries, bits):
    """the tuple the engine takes: (keys, digests [n, 32], values, dir, bits)"""
    n = len(entries)
    keys = np.array([e[0] for e in entries], np.uint64).reshape(-1)
    dig = np.frombuffer(b"".join(e[1] for e in entries), np.uint8).reshape(n, 32).copy()
    values = np.array([e[2] for e in entries], np.uint64).reshape(-1)
    return keys, dig, values, np.array(directory(entries, bits), np.uint32), bits


def from_arrays(keys, digests, values):
    dig = np.ascontiguousarray(digests, np.uint8).reshape(-1, 32)
    return [(int(k), dig[i].tobytes(), int(v)) for i, (k, v) in enumerate(zip(keys, values))]


def real_key(digest):
    """a real chunk's key: the digest's bytes 0..8 big-endian"""
    return int.from_bytes(bytes(digest[:8]), "big")


def random_pairs(rng, n, forged_key=None):
    """n distinct random digests with their real keys (or one forged key)"""
    dig = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    dig = np.unique(dig, axis=0)
    while dig.shape[0] < n:  # never, at 32 random bytes
        dig = np.unique(np.concatenate([dig, rng.integers(0, 256, (n, 32), dtype=np.uint8)]), axis=0)
    dig = dig[rng.permutation(dig.shape[0])[:n]]
    if forged_key is None:
        keys = np.array([real_key(d) for d in dig], np.uint64)
    else:
        keys = np.full(n, forged_key, np.uint64)
    return keys, dig
