"""Test infrastructure: the chunk peers (include/sdcas.h) in plain Python, over
tests/_chunk_holders_ref.py's entry lists: dicts, bisect and `sorted`. Both
modes, the common rule, sums modulo 2^64 and, given max_pairs, the overflow.
Every comparison against the library is exact equality."""
import bisect

import numpy as np

from tests._chunk_holders_ref import U64_MAX, pairs

EARLIER, ALL = 0, 1
MASK = (1 << 64) - 1
COUNTS = ("files", "chunks", "common_chunks", "pairs", "edges", "files_with_peer", "overflow")


def counted(entries, pair, fid, mode):
    """the values of `pair`'s entries that count for a file with id `fid`"""
    lo = bisect.bisect_left(entries, (pair[0], pair[1], 0))
    hi = bisect.bisect_right(entries, (pair[0], pair[1], U64_MAX))
    run = [e[2] for e in entries[lo:hi]]
    return [v for v in run if (v < fid if mode == EARLIER else v != fid)]


def peers(entries, keys, digests, chunk_file, chunk_len, file_ids, k, max_holders, mode=EARLIER, valid=None,
          max_pairs=None):
    """-> dict: peer_count uint32[n], peers / peers_bytes uint64[n, k], shared_bytes, unique_bytes, common_bytes
    uint64[n], counts. max_pairs None: no bound."""
    ids = [int(v) for v in np.asarray(file_ids, np.uint64).reshape(-1)]
    n = len(ids)
    score = [dict() for _ in range(n)]
    shared, unique, common = [0] * n, [0] * n, [0] * n
    counts = dict.fromkeys(COUNTS, 0)
    counts["files"] = n
    for c, pair in enumerate(pairs(keys, digests)):
        f, ln = int(chunk_file[c]), int(chunk_len[c])
        if (valid is not None and not valid[c]) or f >= n:
            continue
        counts["chunks"] += 1
        hs = counted(entries, pair, ids[f], mode)
        if len(hs) > max_holders:
            counts["common_chunks"] += 1
            common[f] = (common[f] + ln) & MASK
        elif hs:
            counts["pairs"] += len(hs)
            shared[f] = (shared[f] + ln) & MASK
            for h in hs:
                score[f][h] = (score[f].get(h, 0) + ln) & MASK
        else:
            unique[f] = (unique[f] + ln) & MASK
    over = max_pairs is not None and counts["pairs"] > max_pairs
    counts["overflow"] = int(over)
    cnt = np.zeros(n, np.uint32)
    who, how = np.zeros((n, k), np.uint64), np.zeros((n, k), np.uint64)
    if not over:
        for f in range(n):
            order = sorted(score[f].items(), key=lambda t: (-t[1], t[0]))
            counts["edges"] += len(order)
            counts["files_with_peer"] += bool(order)
            cnt[f] = min(k, len(order))
            for r, (h, b) in enumerate(order[:k]):
                who[f, r], how[f, r] = h, b
    return {"peer_count": cnt, "peers": who, "peers_bytes": how, "shared_bytes": np.array(shared, np.uint64).reshape(-1),
            "unique_bytes": np.array(unique, np.uint64).reshape(-1),
            "common_bytes": np.array(common, np.uint64).reshape(-1), "counts": counts}


def same(a, b):
    """two results equal, array by array and count by count"""
    return all(np.array_equal(a[key], b[key]) for key in ("peer_count", "peers", "peers_bytes", "shared_bytes",
                                                          "unique_bytes", "common_bytes")) and a["counts"] == b["counts"]
