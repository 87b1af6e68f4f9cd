#!/usr/bin/env python3
"""Timing of the holders index (sdcas_dev_chunk_holders_remove / _add / _match,
csrc/chunk_holders.hip) beside what it is priced against. For an index of
n = 2^22, 2^24 and 2^26 entries built from real keys (the
digest's first 8 bytes), legs alternating in ONE process, HIP events around
each, 20 repetitions after a warm-up, median and min:
  remove   sdcas_dev_chunk_holders_remove with about 1 %, 10 % and 50 % of the
           entries removed, each with r = 2^10 and r = 2^20 ids (ids that hold
           nothing fill `removed` up to r)
  copy     the floor: a device-to-device copy of the index's keys, digests and
           values
  rebuild  what the remove replaces: sdcas_dev_chunk_holders_add of the
           surviving triples into an empty index
  match    sdcas_dev_chunk_holders_match of 2^20 queries, half of them stored,
           beside sdcas_dev_chunk_index_match of the same queries against the
           chunk index of the same pairs (each pair's first entry)

Half of the entries belong to 512 large files, the other half to 2^21 small
ones; one pair (the all-zero chunk) is held by n / 16 files, the others by 4 on
average. Before any time is taken every output is compared with the tool's own
numpy reference: the remove's arrays, directory and counts, the rebuild's
arrays against the remove's, the match's pos / value / holders / counts.

--count-only prints the byte and request model without a device. No threshold
is set: the numbers go to profiles/chunk_holders.json and DESIGN.md §3.8.

This tool is no longer the only place where the block scan's third level (2^24
entries and more, so its sizes from 2^24 + 1 on, 2^26 among them) is checked:
tests/test_gpu_index_scale.py compares the remove, the add and the match with a
torch reference at 2^24 + 1 to 2^25 + 257 entries, every output element.

The model. Remove: every entry is read once (48 bytes) and the kept ones are
written once (48 bytes each); per entry one search of `removed` by halving,
ceil_log2(r + 1) dependent 8-byte reads of an array of 8 r bytes; 32 bytes of
keep masks and 4 of counts per 256 entries written and read back; one lower
bound in the new keys per directory slot. Match: chunk_index_match's requests
(one directory read, the bucket halved, digest and value on an equal key) plus
one more halving from the run's first entry to the bucket's end for its last.
Rebuild: ceil_log2(m) merge passes over the m surviving triples, each a halving
of up to log2 of the run width per triple, then one pass that writes m
entries."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spacedrive_amd import _native as N  # noqa: E402

M = 1 << 20
SIZES = (1 << 22, 1 << 24, 1 << 26)
REPS = 20
FRACTIONS = (0.01, 0.10, 0.50)
RS = (1 << 10, 1 << 20)
BIG, IDS = 512, 1 << 21  # ids [0, BIG): the large files, [BIG, IDS): the small ones; ids >= IDS hold nothing
MATCH_COUNTS = [name for name, _ in N.IndexMatchCounts._fields_]
ADD_COUNTS = [name for name, _ in N.IndexAddCounts._fields_]
REMOVE_COUNTS = [name for name, _ in N.HoldersRemoveCounts._fields_]


def dir_bits(n):
    return 0 if n < 8 else min(28, (n - 1).bit_length() - 2)


def ceil_log2(x):
    return max(0, (int(x) - 1).bit_length())


def model(n, m=M):
    bits = dir_bits(n)
    bucket = n / (1 << bits)
    steps = max(1, int(np.ceil(np.log2(bucket + 1))))
    blocks = (n + 255) // 256
    legs = []
    for f in FRACTIONS:
        kept = n - int(n * f)
        for r in RS:
            legs.append({"fraction": f, "r": r, "bytes_read": 48 * n, "bytes_written": 48 * kept,
                         "removed_bytes": 8 * r, "requests_into_removed_per_entry": ceil_log2(r + 1),
                         "rebuild_triples": kept, "rebuild_merge_passes": ceil_log2(kept),
                         "rebuild_workspace_bytes": 16 * kept})
    return {"n": n, "m": m, "bits": bits, "entries_per_bucket": bucket, "copy_bytes_each_way": 48 * n,
            "remove": legs, "remove_workspace_bytes": 36 * blocks, "directory_bytes": 4 * ((1 << bits) + 1),
            "match_dependent_requests_per_query": {"directory": 1, "key_steps_first": steps, "key_steps_last": steps,
                                                   "digest_on_an_equal_key": 1, "value_on_a_hit": 1},
            "match_bytes_in": m * 40, "match_bytes_out": m * 20 + 32}


def bswap64(t):
    """int64 words with their bytes reversed"""
    import torch
    return t.contiguous().view(torch.uint8).view(-1, 8).flip(1).contiguous().view(torch.int64).view(-1)


def directory(keys, n, bits):
    """the directory of n sorted keys (int64 bit patterns of the u64s) on the device, int32"""
    import torch
    bucket = ((keys >> (64 - bits)) & ((1 << bits) - 1)) if bits else torch.zeros(n, dtype=torch.int64, device="cuda")
    d = torch.zeros((1 << bits) + 1, dtype=torch.int64, device="cuda")
    d[1:] = torch.cumsum(torch.bincount(bucket, minlength=1 << bits), 0)
    return d.to(torch.int32)


def gather(t, idx, step=1 << 24):
    import torch
    return torch.cat([t[idx[i:i + step]] for i in range(0, idx.numel(), step)])


def make(n, m, seed):
    """-> the holders index (keys, digests, values, dir, bits), the chunk index of its pairs, and m queries
    (half of them pairs of the index), all on the device"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    lo, hi = -(1 << 63), (1 << 63) - 1
    pairs = n // 4
    words = torch.randint(lo, hi, (pairs + m // 2, 4), dtype=torch.int64, device="cuda", generator=g)
    keys = bswap64(words[:, 0])  # the first 8 digest bytes, big-endian
    order = torch.sort(keys[:pairs] ^ lo).indices  # unsigned order
    pkeys, pwords = gather(keys[:pairs], order), gather(words[:pairs], order)
    assert bool((pkeys[1:] != pkeys[:-1]).all()), "two random 64-bit keys met: another seed"
    # (pair, id) of every entry as one sortable word; pair 0 is held by n / 16 files
    draw = n + n // 8
    pair = torch.randint(1, pairs, (draw,), dtype=torch.int64, device="cuda", generator=g)
    big = torch.rand(draw, device="cuda", generator=g) < 0.5
    ident = torch.where(big, torch.randint(0, BIG, (draw,), device="cuda", generator=g),
                        torch.randint(BIG, IDS, (draw,), device="cuda", generator=g))
    wide = torch.randperm(IDS, device="cuda", generator=g)[:min(n // 16, IDS // 2)]
    word = torch.unique(torch.cat([wide, pair * IDS + ident]))  # sorted, distinct
    assert word.numel() >= n, "too few distinct entries drawn"
    word = word[:n]
    pair, values = word // IDS, word % IDS
    ikeys, iwords = gather(pkeys, pair), gather(pwords, pair)
    bits = dir_bits(n)
    index = (ikeys, iwords.view(torch.uint8).view(-1), values.contiguous(), directory(ikeys, n, bits), bits)
    # the chunk index of the same pairs: each run's first entry
    head = torch.ones(n, dtype=torch.bool, device="cuda")
    head[1:] = pair[1:] != pair[:-1]
    hi_ = torch.nonzero(head).view(-1)
    ck, cw, cv = gather(ikeys, hi_), gather(iwords, hi_), gather(values, hi_)
    cbits = dir_bits(ck.numel())
    cindex = (ck, cw.view(torch.uint8).view(-1), cv.contiguous(), directory(ck, ck.numel(), cbits), cbits)
    pick = torch.randint(0, n, (m // 2,), device="cuda", generator=g)
    qkeys = torch.cat([ikeys[pick], keys[pairs:]])
    qwords = torch.cat([iwords[pick], words[pairs:]])
    p = torch.randperm(m, device="cuda", generator=g)
    return index, cindex, (qkeys[p].contiguous(), qwords[p].contiguous().view(torch.uint8).view(-1))


def removed_ids(rng, fraction, r):
    """r ascending ids of which the first ones hold about `fraction` of the entries (the large files hold half
    of them, the small ones the other half) and the rest nothing"""
    if r <= 2 * BIG:
        holding = rng.permutation(BIG)[:max(1, round(2 * fraction * BIG))]
    else:  # half of the fraction from each class
        holding = np.concatenate([rng.permutation(BIG)[:round(fraction * BIG)],
                                  BIG + rng.permutation(IDS - BIG)[:round(fraction * (IDS - BIG))]])
    assert holding.size <= r
    ids = np.concatenate([holding, IDS + 1 + np.arange(r - holding.size)]).astype(np.uint64)
    return np.sort(ids)


def host(index):
    return (index[0].cpu().numpy().view(np.uint64), index[1].cpu().numpy().reshape(-1, 32),
            index[2].cpu().numpy().view(np.uint64))


def np_directory(keys, bits):
    d = np.searchsorted(keys, np.arange(1 << bits, dtype=np.uint64) << np.uint64(64 - bits)) if bits \
        else np.zeros(1, np.int64)
    return np.concatenate([d, [keys.size]]).astype(np.uint32)


def match_reference(hindex, queries):
    """numpy: keys are unique per pair, so a key finds its run"""
    ik, idg, iv = hindex
    qk, qd = queries[0].cpu().numpy().view(np.uint64), queries[1].cpu().numpy().reshape(-1, 32)
    n, m = ik.size, qk.size
    first = np.searchsorted(ik, qk, side="left")
    last = np.searchsorted(ik, qk, side="right")
    at = np.minimum(first, n - 1)
    hit = (last > first) & (idg[at] == qd).all(axis=1)
    return (np.where(hit, first, -1).astype(np.int64), np.where(hit, iv[at], 0).astype(np.uint64),
            np.where(hit, last - first, 0).astype(np.uint32),
            dict(queries=m, hits=int(hit.sum()), misses=int(m - hit.sum()), skipped=0))


def run(args):
    import torch
    from spacedrive_amd import Engine
    eng = Engine()
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    eng.dev_bind_stream(h)
    results = []
    p = lambda t: t.data_ptr() if t.numel() else 0
    with torch.cuda.stream(stream):
        for n in args.sizes:
            index, cindex, queries = make(n, M, seed=n)
            ik, idg, iv, idr, bits = index
            hindex = host(index)
            rng = np.random.default_rng(n)
            new = [torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(32 * n, dtype=torch.uint8, device="cuda"),
                   torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros((1 << bits) + 1, dtype=torch.int32, device="cuda")]
            rc = torch.zeros(4, dtype=torch.int64, device="cuda")
            copies = [torch.empty_like(t) for t in (ik, idg, iv)]
            legs, checks, info = {}, {}, {}

            def remove_leg(d_ids, r):
                return lambda: eng.dev_chunk_holders_remove(p(ik), p(idg), p(iv), p(idr), n, bits, p(d_ids), r, p(new[0]),
                                                            p(new[1]), p(new[2]), p(new[3]), bits, rc.data_ptr(), stream=h)

            def rebuild_leg(sk, sd, sv, out, m, mbits, ac):
                return lambda: eng.dev_chunk_holders_add(0, 0, 0, 0, 0, 0, p(sk), p(sd), p(sv), 0, m, p(out[0]), p(out[1]),
                                                         p(out[2]), p(out[3]), mbits, 0, 0, ac.data_ptr(), stream=h)

            for f in FRACTIONS:
                for r in RS:
                    name = f"{int(f * 100)}%_r2^{r.bit_length() - 1}"
                    ids = removed_ids(rng, f, r)
                    d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
                    leg = remove_leg(d_ids, r)
                    leg()  # the warm-up, and the run that is checked
                    stream.synchronize()
                    keep = ~np.isin(hindex[2], ids)
                    e = int(keep.sum())
                    wk = hindex[0][keep]
                    got = dict(zip(REMOVE_COUNTS, (int(x) for x in rc.cpu())))
                    checks["remove_" + name] = (
                        got == dict(entries_old=n, removed=n - e, entries_new=e, values=r)
                        and bool((new[0][:e].cpu().numpy().view(np.uint64) == wk).all())
                        and bool((new[1][:32 * e].cpu().numpy().reshape(-1, 32) == hindex[1][keep]).all())
                        and bool((new[2][:e].cpu().numpy().view(np.uint64) == hindex[2][keep]).all())
                        and bool((new[3].cpu().numpy().view(np.uint32) == np_directory(wk, bits)).all()))
                    info[name] = {"fraction_removed": (n - e) / n, "r": r, "kept": e}
                    legs["remove_" + name] = leg
                    # the survivors, shuffled (a rebuild gets them in the files' order, not the index's)
                    perm = torch.randperm(e, device="cuda")
                    sk, sd, sv = (gather(new[0][:e], perm), gather(new[1][:32 * e].view(-1, 32), perm).view(-1),
                                  gather(new[2][:e], perm))
                    mbits = dir_bits(e)
                    out = [torch.zeros(e, dtype=torch.int64, device="cuda"),
                           torch.zeros(32 * e, dtype=torch.uint8, device="cuda"),
                           torch.zeros(e, dtype=torch.int64, device="cuda"),
                           torch.zeros((1 << mbits) + 1, dtype=torch.int32, device="cuda")]
                    ac = torch.zeros(6, dtype=torch.int64, device="cuda")
                    leg = rebuild_leg(sk, sd, sv, out, e, mbits, ac)
                    leg()
                    stream.synchronize()
                    checks["rebuild_" + name] = (
                        dict(zip(ADD_COUNTS, (int(x) for x in ac.cpu()))) ==
                        dict(queries=e, hits=0, added=e, batch_duplicates=0, entries_old=0, entries_new=e)
                        and all(bool((a[:k] == b[:k]).all()) for a, b, k in zip(out, new, (e, 32 * e, e)))
                        and bool((out[3].cpu().numpy().view(np.uint32) == np_directory(wk, mbits)).all()))
                    legs["rebuild_" + name] = leg
            legs["copy"] = lambda: [c.copy_(t) for c, t in zip(copies, (ik, idg, iv))]
            qk, qd = queries
            pos, val = (torch.empty(M, dtype=torch.int64, device="cuda") for _ in range(2))
            hold = torch.empty(M, dtype=torch.int32, device="cuda")
            mc = torch.zeros(4, dtype=torch.int64, device="cuda")
            cpos, cval = (torch.empty(M, dtype=torch.int64, device="cuda") for _ in range(2))
            cmc = torch.zeros(4, dtype=torch.int64, device="cuda")
            ck, cd, cv, cdr, cbits = cindex
            legs["match_holders"] = lambda: eng.dev_chunk_holders_match(p(ik), p(idg), p(iv), p(idr), n, bits, p(qk), p(qd),
                                                                        0, M, p(pos), p(val), p(hold), mc.data_ptr(),
                                                                        stream=h)
            legs["match_index"] = lambda: eng.dev_chunk_index_match(p(ck), p(cd), p(cv), p(cdr), ck.numel(), cbits, p(qk),
                                                                    p(qd), 0, M, p(cpos), p(cval), cmc.data_ptr(), stream=h)
            for name in ("copy", "match_holders", "match_index"):
                legs[name]()
            stream.synchronize()
            wpos, wval, whold, wmc = match_reference(hindex, queries)
            checks["copy"] = all(bool((c == t).all()) for c, t in zip(copies, (ik, idg, iv)))
            checks["match_holders"] = (bool((pos.cpu().numpy() == wpos).all())
                                       and bool((val.cpu().numpy().view(np.uint64) == wval).all())
                                       and bool((hold.cpu().numpy().view(np.uint32) == whold).all())
                                       and dict(zip(MATCH_COUNTS, (int(x) for x in mc.cpu()))) == wmc)
            checks["match_index"] = (bool(((cpos.cpu().numpy() >= 0) == (wpos >= 0)).all())
                                     and bool((cval.cpu().numpy().view(np.uint64) == wval).all())
                                     and dict(zip(MATCH_COUNTS, (int(x) for x in cmc.cpu()))) == wmc)
            if not all(checks.values()):
                print(json.dumps({"n": n, "checks": checks}))
                raise SystemExit(f"n = {n}: an output differs from the reference")
            times = {k: [] for k in legs}
            for _ in range(args.reps):
                for name, f in legs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    f()
                    b.record(stream)
                    b.synchronize()
                    times[name].append(a.elapsed_time(b) * 1000.0)
            us = {k: {"median": float(np.median(v)), "min": float(np.min(v))} for k, v in times.items()}
            r = {"model": model(n), "pairs": int(ck.numel()), "longest_run": int(whold.max()), "remove": info,
                 "checks": checks, "us": us,
                 "over_copy": {k: v["median"] / us["copy"]["median"] for k, v in us.items()
                               if k.startswith(("remove_", "rebuild_"))},
                 "match_holders_over_match_index": us["match_holders"]["median"] / us["match_index"]["median"]}
            results.append(r)
            print(json.dumps({"n": n, "us": us}), flush=True)
            if args.out:  # what is measured so far, should a later size not finish
                with open(args.out, "w") as f:
                    f.write(json.dumps({"m": M, "reps": args.reps, "results": results}, indent=1) + "\n")
            del legs, new, copies, index, cindex, queries, hindex, ik, idg, iv, idr, ck, cd, cv, cdr, qk, qd
            torch.cuda.empty_cache()
    eng.close()
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--count-only", action="store_true", help="print the byte and request model, no device")
    ap.add_argument("--sizes", type=lambda s: tuple(1 << int(x) for x in s.split(",")), default=SIZES,
                    help="log2 of the index sizes, comma separated (default 22,24,26)")
    ap.add_argument("--reps", type=int, default=REPS, help="timed repetitions of every leg (default 20)")
    ap.add_argument("--out", default=None, help="write the result as JSON here too")
    args = ap.parse_args()
    if args.count_only:
        out = {"model": [model(n) for n in args.sizes]}
    else:
        out = {"m": M, "reps": args.reps, "results": run(args)}
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
