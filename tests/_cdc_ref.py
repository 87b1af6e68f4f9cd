"""Test infrastructure: a numpy restatement of the content-defined chunking and
of the sharing pass (include/sdcas.h). The checker of
tests/test_gpu_chunks.py and tests/test_gpu_chunk_sharing.py; it never calls
the code under test.

gear_table()           G[b] = high 32 bits of sds_mix64("SDCDC001" + b)
window_hash(x)         h(p) = sum over k in 0..min(31, p) of G[x[p - k]] << k, by 32 shifted adds
window_with_hash(t, r) 32 bytes whose window hash is t wherever they lie
cuts(x, params)        the literal cut loop -> (ends, kinds), ends exclusive and relative to the file
chunk_files(...)       the arrays and counts sdcas_chunk_messages returns for a list of files
sharing(...)           the sharing pass with dicts
"""
import numpy as np

from tests._oracle import mix64

GEAR_SEED = 0x3130304344434453  # "SDCDC001" read little-endian
DEFAULT_PARAMS = (2048, 13, 65536)
TEST_PARAMS = (64, 8, 1024)
KIND_END, KIND_HASH, KIND_MAX = 0, 1, 2
MAX_CHUNKS = 1 << 30


def gear_table():
    with np.errstate(over="ignore"):
        g = mix64(np.uint64(GEAR_SEED) + np.arange(256, dtype=np.uint64))
    return (g >> np.uint64(32)).astype(np.uint32)


_G = gear_table()


def window_hash(x):
    """h at every position of one file (uint32[len(x)])"""
    x = np.asarray(x, dtype=np.uint8)
    g = _G[x].astype(np.uint64)
    h = np.zeros(x.size, np.uint64)
    for k in range(min(32, x.size)):
        h[k:] += g[:x.size - k] << np.uint64(k)
    return (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def window_with_hash(target, rng, last=None):
    """32 bytes w whose window hash is `target` wherever they lie in a file
    (window_hash(x)[p] == target for w's last byte at p >= 31). The byte with
    shift k, w[31 - k], decides bit k of the sum once the bytes with lower
    shifts are chosen, so the bytes are drawn for k = 0..31 in turn, each among
    the values whose table entry has the parity that bit needs. last: the value
    w[31] must take (its entry's parity must be target's bit 0)"""
    target = int(target) & 0xFFFFFFFF
    odd = [np.flatnonzero((_G & 1) == v) for v in (0, 1)]
    w = np.zeros(32, np.uint8)
    total = 0
    for k in range(32):
        need = ((target >> k) ^ (total >> k)) & 1
        if k == 0 and last is not None:
            b = int(last)
            assert int(_G[b]) & 1 == need, "the given last byte cannot give this hash"
        else:
            b = int(rng.choice(odd[need]))
        w[31 - k] = b
        total = (total + (int(_G[b]) << k)) & 0xFFFFFFFF
    assert total == target
    return w


def params_valid(params):
    min_len, avg_bits, max_len = (int(v) for v in params)
    return 6 <= avg_bits <= 24 and 32 <= min_len < (1 << avg_bits) < max_len <= (1 << 28)


def cuts(x, params=DEFAULT_PARAMS):
    """-> (ends int64[chunks], kinds uint8[chunks]) of one file"""
    assert params_valid(params), params
    min_len, avg_bits, max_len = (int(v) for v in params)
    avg = 1 << avg_bits
    h = window_hash(x)
    strict = (h >> np.uint32(32 - (avg_bits + 1))) == 0
    loose = (h >> np.uint32(32 - (avg_bits - 1))) == 0
    L = int(np.asarray(x).size)
    ends, kinds = [], []
    s = 0
    while s < L:
        if L - s <= min_len:
            e, found = L, False
        else:
            hi = min(s + max_len, L)
            e, found = hi, False
            # the candidates e in [s + min_len, hi], in order: STRICT(e - 1)
            # while e - s < avg, LOOSE(e - 1) from there on
            mid = min(s + avg, hi + 1)
            cand = np.concatenate([strict[s + min_len - 1:mid - 1], loose[mid - 1:hi]])
            hit = np.flatnonzero(cand)
            if hit.size:
                e, found = s + min_len + int(hit[0]), True
        ends.append(e)
        kinds.append(KIND_END if e == L else KIND_HASH if found else KIND_MAX)
        s = e
    return np.array(ends, np.int64), np.array(kinds, np.uint8)


def chunk_plan(lens, params=DEFAULT_PARAMS):
    """what sdcas_chunk_plan returns: (max_chunks, max_slots); ValueError for
    invalid parameters, OverflowError above 2^30 chunks"""
    if not params_valid(params):
        raise ValueError("invalid chunk parameters")
    min_len = int(params[0])
    max_chunks = sum((int(n) + min_len - 1) // min_len for n in lens)
    if max_chunks > MAX_CHUNKS:
        raise OverflowError("more than 2^30 chunks")
    return max_chunks, sum((int(n) + 1023) // 1024 for n in lens) + max_chunks


def chunk_files(files, offsets, params=DEFAULT_PARAMS, known=None):
    """files: list of uint8 arrays; offsets: where each starts in the blob ->
    dict of file_chunks uint64[n + 1], chunk_off uint64[m] (blob offsets),
    chunk_len uint64[m], chunk_file uint32[m], kinds uint8[m] and counts (files,
    chunks, total_bytes, hash_cuts, max_cuts, end_chunks). known: cuts(file,
    params) of every file, where the caller has them already"""
    fc = [0]
    off, ln, fl, kd = [], [], [], []
    for i, (x, o) in enumerate(zip(files, offsets)):
        x = np.asarray(x, np.uint8)
        if x.size:
            ends, kinds = known[i] if known is not None else cuts(x, params)
            starts = np.concatenate([[0], ends[:-1]])
            off += [int(o) + int(s) for s in starts]
            ln += [int(e - s) for s, e in zip(starts, ends)]
            fl += [i] * len(ends)
            kd += [int(k) for k in kinds]
        fc.append(len(off))
    kd = np.array(kd, np.uint8)
    counts = {"files": len(files), "chunks": len(off), "total_bytes": int(sum(ln)),
              "hash_cuts": int((kd == KIND_HASH).sum()), "max_cuts": int((kd == KIND_MAX).sum()),
              "end_chunks": int((kd == KIND_END).sum())}
    return {"file_chunks": np.array(fc, np.uint64), "chunk_off": np.array(off, np.uint64),
            "chunk_len": np.array(ln, np.uint64), "chunk_file": np.array(fl, np.uint32), "kinds": kd,
            "counts": counts}


def chunk_reps(blob, chunk_off, chunk_len):
    """rep[c]: the lowest chunk with the same bytes (what the group-by over
    the chunk digests gives), from the bytes themselves"""
    first, rep = {}, []
    for c, (o, n) in enumerate(zip(chunk_off, chunk_len)):
        b = bytes(blob[int(o):int(o) + int(n)])
        rep.append(first.setdefault(b, c))
    return np.array(rep, np.int64)


def sharing(chunk_file, chunk_len, rep, n_files):
    """-> dict of new_bytes, self_bytes, other_bytes, peer_bytes (uint64[n_files]),
    peer (int64[n_files]) and counts (files, chunks, distinct_chunks,
    total_bytes, stored_bytes, files_with_peer); all sums modulo 2^64"""
    M = (1 << 64) - 1
    m = len(chunk_file)
    new = [0] * n_files
    B = [dict() for _ in range(n_files)]
    distinct = total = stored = 0
    for c in range(m):
        i, n, r = int(chunk_file[c]), int(chunk_len[c]), int(rep[c])
        if r < 0 or r > c:
            r = c
        total = (total + n) & M
        if r == c:
            new[i] = (new[i] + n) & M
            distinct += 1
            stored = (stored + n) & M
        else:
            f = int(chunk_file[r])
            B[i][f] = (B[i].get(f, 0) + n) & M
    self_b = [B[i].get(i, 0) for i in range(n_files)]
    other = [sum(v for f, v in B[i].items() if f != i) & M for i in range(n_files)]
    peer, peer_b = [], []
    for i in range(n_files):
        best, best_f = 0, -1
        for f in sorted(B[i]):
            if f != i and B[i][f] > best:
                best, best_f = B[i][f], f
        peer.append(best_f)
        peer_b.append(best)
    counts = {"files": n_files, "chunks": m, "distinct_chunks": distinct, "total_bytes": total,
              "stored_bytes": stored, "files_with_peer": sum(1 for p in peer if p >= 0)}
    return {"new_bytes": np.array(new, np.uint64), "self_bytes": np.array(self_b, np.uint64),
            "other_bytes": np.array(other, np.uint64), "peer": np.array(peer, np.int64),
            "peer_bytes": np.array(peer_b, np.uint64), "counts": counts}
