"""Test infrastructure: the holders index (include/sdcas.h) in plain Python. An
index is a list of (key, digest bytes, value) tuples, strictly ascending as
tuples — Python compares ints as unsigned and bytes as memcmp does — so a pair
may repeat, once per distinct value, lowest value first. Everything is a set, a
dict or a bisect over that list. Every comparison against the library is exact
equality."""
import bisect

import numpy as np

from tests._chunk_index_ref import arrays, dir_bits, directory, from_arrays, pairs, random_pairs, real_key  # noqa: F401

HIT, ADDED, SKIPPED = 1, 2, 4
U64_MAX = (1 << 64) - 1


def triples(keys, digests, values):
    """[(key, digest bytes, value)] of a batch (values None: 0)"""
    ps = pairs(keys, digests)
    vs = [0] * len(ps) if values is None else [int(v) for v in np.asarray(values, np.uint64)]
    return [(k, d, v) for (k, d), v in zip(ps, vs)]


def check(entries, dir=None, bits=0):
    """-> (0, None) for a holders index, (1, the first entry that does not order
    after the one before) or (2, the first directory slot that is wrong)"""
    for i in range(1, len(entries)):
        if not entries[i - 1] < entries[i]:
            return 1, i
    if dir is not None:
        want = directory(entries, bits)
        for j, w in enumerate(want):
            if int(dir[j]) != w:
                return 2, j
    return 0, None


def build(keys, digests, values, valid=None):
    """the index of a batch alone: its distinct valid triples, sorted"""
    return add([], keys, digests, values, valid)[0]


def match(entries, keys, digests, valid=None):
    """-> (pos: the pair's first entry or -1, value: the lowest holder or 0,
    holders: the entries with the pair, counts)"""
    pos, value, holders = [], [], []
    counts = dict(queries=0, hits=0, misses=0, skipped=0)
    for c, (k, d) in enumerate(pairs(keys, digests)):
        if valid is not None and not valid[c]:
            pos.append(-1), value.append(0), holders.append(0)
            counts["skipped"] += 1
            continue
        counts["queries"] += 1
        lo = bisect.bisect_left(entries, (k, d, 0))
        hi = bisect.bisect_right(entries, (k, d, U64_MAX))
        counts["hits" if hi > lo else "misses"] += 1
        pos.append(lo if hi > lo else -1), value.append(entries[lo][2] if hi > lo else 0), holders.append(hi - lo)
    return (np.array(pos, np.int64).reshape(-1), np.array(value, np.uint64).reshape(-1),
            np.array(holders, np.uint32).reshape(-1), counts)


def add(entries, keys, digests, values, valid=None):
    """-> (new entries, pos, flags, counts), read per triple"""
    old = set(entries)
    new, flags = set(old), []
    counts = dict(queries=0, hits=0, added=0, batch_duplicates=0, entries_old=len(entries), entries_new=0)
    ts = triples(keys, digests, values)
    for c, t in enumerate(ts):
        if valid is not None and not valid[c]:
            flags.append(SKIPPED)
            continue
        counts["queries"] += 1
        if t in old:
            flags.append(HIT)
            counts["hits"] += 1
        elif t in new:
            flags.append(0)
            counts["batch_duplicates"] += 1
        else:
            new.add(t)
            flags.append(ADDED)
            counts["added"] += 1
    out = sorted(new)
    counts["entries_new"] = len(out)
    where = {t: i for i, t in enumerate(out)}
    pos = [where[t] if flags[c] != SKIPPED else -1 for c, t in enumerate(ts)]
    return out, np.array(pos, np.int64).reshape(-1), np.array(flags, np.uint8).reshape(-1), counts


def remove(entries, removed):
    """-> (the entries whose value is not in `removed`, in their order, counts)"""
    gone = {int(v) for v in removed}
    out = [e for e in entries if e[2] not in gone]
    return out, dict(entries_old=len(entries), removed=len(entries) - len(out), entries_new=len(out),
                     values=len(removed))


def batch_arrays(ts):
    """a list of triples as the (keys, digests [m, 32], values) a call takes"""
    m = len(ts)
    keys = np.array([t[0] for t in ts], np.uint64).reshape(-1)
    dig = np.frombuffer(b"".join(t[1] for t in ts), np.uint8).reshape(m, 32).copy()
    return keys, dig, np.array([t[2] for t in ts], np.uint64).reshape(-1)
