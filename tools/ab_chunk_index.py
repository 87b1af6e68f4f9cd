#!/usr/bin/env python3
"""Timing of the chunk index (sdcas_dev_chunk_index_match / _add,
csrc/chunk_index.hip) beside what a caller had to do without it. For an index
of n = 2^22, 2^24 and 2^26 entries (real keys: the digest's first 8 bytes) and
a batch of m = 2^20 pairs, half of them in the index, legs alternating in ONE
process, HIP events around each, 20 repetitions after a warm-up, median and
min:
  match    sdcas_dev_chunk_index_match of the batch against the index
  confirm  the yardstick: sdcas_dev_confirm_duplicates over the n + m
           concatenated pairs, which is how a caller found the batch's pairs
           among the stored ones before (that code is not under test)
  add      sdcas_dev_chunk_index_add of the same batch into the same index
  copy     the yardstick: a device-to-device copy of the index's keys,
           digests and values, the least a merge can move

Before any time is taken every output is compared with the tool's own numpy
reference: the match's pos / value / counts, the add's new arrays, directory,
pos / flags / counts.

--count-only prints the request and byte model without a device. No threshold
is set: the numbers go to profiles/chunk_index.json and DESIGN.md §3.7.

The model, per query of the match: one directory read (two adjacent u32), then
the bucket halved, one dependent 8-byte key read per step (a bucket of the
recommended width holds n / 2^bits = 2 to 4 entries: 2 to 3 steps), then, on an
equal key, 32 digest bytes as two 16-byte loads and the 8-byte value: 4 to 6
dependent requests, whatever n is. The concatenated confirm inserts n + m
pairs into two tables of 2 * 2^ceil_log2(2 (n + m)) u32 slots and reads every
pair at least twice. The add reads the old index once and writes the new one
once (48 bytes per entry each way, and 4 bytes per directory slot); its
batch-sized passes (confirm over m, match, an 8-pass radix sort of the added
keys, and ceil_log2(m) merge launches that work on no items unless a run of
one key is longer than 64) do not grow with n."""
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
MATCH_COUNTS = [name for name, _ in N.IndexMatchCounts._fields_]
ADD_COUNTS = [name for name, _ in N.IndexAddCounts._fields_]


def dir_bits(n):
    return 0 if n < 8 else min(28, (n - 1).bit_length() - 2)


def model(n, m=M):
    bits, nbits = dir_bits(n), dir_bits(n + m)
    bucket = n / (1 << bits)
    steps = max(1, int(np.ceil(np.log2(bucket + 1))))
    cap = 64
    while cap < 2 * (n + m):
        cap <<= 1
    return {"n": n, "m": m, "bits": bits, "bits_new": nbits, "entries_per_bucket": bucket,
            "match_dependent_requests_per_query": {"directory": 1, "key_steps": steps, "digest_and_value_on_a_hit": 2},
            "match_bytes_in": m * 40, "match_bytes_out": m * 16 + 32,
            "index_bytes": n * 48 + 4 * ((1 << bits) + 1),
            "confirm_pairs": n + m, "confirm_table_bytes": 2 * cap * 4, "confirm_slot_bytes": 3 * (n + m) * 4,
            "add_bytes_read": n * 48 + m * 48, "add_bytes_written": (n + m // 2) * 48 + 4 * ((1 << nbits) + 1),
            "copy_bytes_each_way": n * 48, "add_workspace_bytes": 52 * m}


def bswap64(t):
    """int64 words with their bytes reversed"""
    import torch
    return t.contiguous().view(torch.uint8).view(-1, 8).flip(1).contiguous().view(torch.int64).view(-1)


def make(n, m, seed):
    """-> index tensors (keys, digests, values, dir as int64/uint8/int64/int32, sorted by key) and a batch
    of m pairs, the first half drawn from the index, shuffled; all on the device, keys unique"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    lo, hi = -(1 << 63), (1 << 63) - 1
    words = torch.randint(lo, hi, (n + m // 2, 4), dtype=torch.int64, device="cuda", generator=g)
    keys = bswap64(words[:, 0])  # the first 8 digest bytes, big-endian
    order = torch.sort(keys[:n] ^ lo).indices  # unsigned order
    # (gathered 2^24 rows at a time: one indexing launch over 2^26 rows of 32 bytes is refused as too large a grid)
    step = 1 << 24
    ikeys = torch.cat([keys[:n][order[i:i + step]] for i in range(0, n, step)])
    iwords = torch.cat([words[:n][order[i:i + step]] for i in range(0, n, step)])
    assert bool((ikeys[1:] != ikeys[:-1]).all()), "two random 64-bit keys met: another seed"
    ivalues = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
    bits = dir_bits(n)
    bucket = ((ikeys >> (64 - bits)) & ((1 << bits) - 1)) if bits else torch.zeros(n, dtype=torch.int64, device="cuda")
    d = torch.zeros((1 << bits) + 1, dtype=torch.int64, device="cuda")
    d[1:] = torch.cumsum(torch.bincount(bucket, minlength=1 << bits), 0)
    pick = torch.randint(0, n, (m // 2,), device="cuda", generator=g)
    bkeys = torch.cat([ikeys[pick], keys[n:]])
    bwords = torch.cat([iwords[pick], words[n:]])
    p = torch.randperm(m, device="cuda", generator=g)
    bkeys, bwords = bkeys[p].contiguous(), bwords[p].contiguous()
    bvalues = torch.arange(1 << 40, (1 << 40) + m, dtype=torch.int64, device="cuda")
    return (ikeys, iwords.view(torch.uint8).view(-1), ivalues, d.to(torch.int32), bits), \
        (bkeys, bwords.view(torch.uint8).view(-1), bvalues)


def reference(index, batch):
    """numpy: the match's and the add's outputs (keys are unique in the index, so a key finds its entry)"""
    ik, idg, iv = (index[0].cpu().numpy().view(np.uint64), index[1].cpu().numpy().reshape(-1, 32),
                   index[2].cpu().numpy().view(np.uint64))
    bk, bd, bv = (batch[0].cpu().numpy().view(np.uint64), batch[1].cpu().numpy().reshape(-1, 32),
                  batch[2].cpu().numpy().view(np.uint64))
    n, m = ik.size, bk.size
    at = np.minimum(np.searchsorted(ik, bk), n - 1)
    hit = (ik[at] == bk) & (idg[at] == bd).all(axis=1)
    pos = np.where(hit, at, -1).astype(np.int64)
    value = np.where(hit, iv[at], 0).astype(np.uint64)
    mcounts = dict(queries=m, hits=int(hit.sum()), misses=int(m - hit.sum()), skipped=0)
    # the add: the new pairs are distinct in this batch apart from hits drawn twice
    first = np.zeros(m, bool)
    _, fi = np.unique(bk, return_index=True)
    first[fi] = True
    added = first & ~hit
    nk = np.concatenate([ik, bk[added]])
    order = np.argsort(nk, kind="stable")
    nkeys = nk[order]
    ndig = np.concatenate([idg, bd[added]])[order]
    nval = np.concatenate([iv, bv[added]])[order]
    npos = np.searchsorted(nkeys, bk).astype(np.int64)
    flags = np.where(hit, N.SDCAS_INDEX_HIT, np.where(added, N.SDCAS_INDEX_ADDED, 0)).astype(np.uint8)
    nbits = dir_bits(n + m)
    ndir = np.searchsorted(nkeys, (np.arange(1 << nbits, dtype=np.uint64) << np.uint64(64 - nbits)) if nbits
                           else np.zeros(1, np.uint64))
    ndir = np.concatenate([ndir, [nkeys.size]]).astype(np.uint32)
    acounts = dict(queries=m, hits=int(hit.sum()), added=int(added.sum()),
                   batch_duplicates=int(m - hit.sum() - added.sum()), entries_old=n, entries_new=int(nkeys.size))
    return (pos, value, mcounts), (nkeys, ndig, nval, ndir, npos, flags, acounts)


def run(args):
    import torch
    from spacedrive_amd import Engine
    eng = Engine()
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    eng.dev_bind_stream(h)
    results = []
    with torch.cuda.stream(stream):
        for n in args.sizes:
            index, batch = make(n, M, seed=n)
            ik, idg, iv, idr, bits = index
            bk, bd, bv = batch
            nbits = dir_bits(n + M)
            pos = torch.empty(M, dtype=torch.int64, device="cuda")
            val = torch.empty(M, dtype=torch.int64, device="cuda")
            mc = torch.zeros(4, dtype=torch.int64, device="cuda")
            nk = torch.zeros(n + M, dtype=torch.int64, device="cuda")
            nd = torch.zeros(32 * (n + M), dtype=torch.uint8, device="cuda")
            nv = torch.zeros(n + M, dtype=torch.int64, device="cuda")
            ndr = torch.zeros((1 << nbits) + 1, dtype=torch.int32, device="cuda")
            apos = torch.empty(M, dtype=torch.int64, device="cuda")
            afl = torch.empty(M, dtype=torch.uint8, device="cuda")
            ac = torch.zeros(6, dtype=torch.int64, device="cuda")
            ck, cd = torch.cat([ik, bk]), torch.cat([idg, bd])
            crep = torch.empty(n + M, dtype=torch.int64, device="cuda")
            cc = torch.zeros(6, dtype=torch.int64, device="cuda")
            copies = [torch.empty_like(t) for t in (ik, idg, iv)]

            legs = {
                "match": lambda: eng.dev_chunk_index_match(ik.data_ptr(), idg.data_ptr(), iv.data_ptr(), idr.data_ptr(), n,
                                                           bits, bk.data_ptr(), bd.data_ptr(), 0, M, pos.data_ptr(),
                                                           val.data_ptr(), mc.data_ptr(), stream=h),
                "confirm": lambda: eng.dev_confirm_duplicates(ck.data_ptr(), cd.data_ptr(), 0, n + M, rep=crep.data_ptr(),
                                                              counts=cc.data_ptr(), stream=h),
                "add": lambda: eng.dev_chunk_index_add(ik.data_ptr(), idg.data_ptr(), iv.data_ptr(), idr.data_ptr(), n, bits,
                                                       bk.data_ptr(), bd.data_ptr(), bv.data_ptr(), 0, M, nk.data_ptr(),
                                                       nd.data_ptr(), nv.data_ptr(), ndr.data_ptr(), nbits,
                                                       apos.data_ptr(), afl.data_ptr(), ac.data_ptr(), stream=h),
                "copy": lambda: [c.copy_(t) for c, t in zip(copies, (ik, idg, iv))],
            }
            for f in legs.values():  # the warm-up: workspaces are allocated here
                f()
            stream.synchronize()
            # every output against the numpy reference, before any time is taken
            (wpos, wval, wmc), (wk, wd, wv, wdir, wapos, wfl, wac) = reference(index, batch)
            e = wac["entries_new"]
            checks = {
                "match_pos": bool((pos.cpu().numpy() == wpos).all()),
                "match_value": bool((val.cpu().numpy().view(np.uint64) == wval).all()),
                "match_counts": dict(zip(MATCH_COUNTS, (int(x) for x in mc.cpu()))) == wmc,
                "add_counts": dict(zip(ADD_COUNTS, (int(x) for x in ac.cpu()))) == wac,
                "add_keys": bool((nk[:e].cpu().numpy().view(np.uint64) == wk).all()),
                "add_digests": bool((nd[:32 * e].cpu().numpy().reshape(-1, 32) == wd).all()),
                "add_values": bool((nv[:e].cpu().numpy().view(np.uint64) == wv).all()),
                "add_dir": bool((ndr.cpu().numpy().view(np.uint32) == wdir).all()),
                "add_pos": bool((apos.cpu().numpy() == wapos).all()),
                "add_flags": bool((afl.cpu().numpy() == wfl).all()),
                "copy": all(bool((c == t).all()) for c, t in zip(copies, (ik, idg, iv))),
                "confirm_hits": int(cc.cpu()[5]) == M - wac["added"],  # duplicate_files: the batch's pairs stored before
            }
            if not all(checks.values()):
                print(json.dumps({"n": n, "checks": checks}))
                raise SystemExit(f"n = {n}: an output differs from the reference")
            del wk, wd, wv
            times = {k: [] for k in legs}
            for _ in range(REPS):
                for name, f in legs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    f()
                    b.record(stream)
                    b.synchronize()
                    times[name].append(a.elapsed_time(b) * 1000.0)
            r = {"model": model(n), "checks": checks,
                 "us": {k: {"median": float(np.median(v)), "min": float(np.min(v))} for k, v in times.items()}}
            r["match_over_confirm"] = r["us"]["match"]["median"] / r["us"]["confirm"]["median"]
            r["add_over_copy"] = r["us"]["add"]["median"] / r["us"]["copy"]["median"]
            results.append(r)
            print(json.dumps({"n": n, "us": r["us"]}), flush=True)
            del ik, idg, iv, idr, bk, bd, bv, nk, nd, nv, ck, cd, crep, copies, index, batch, legs
            torch.cuda.empty_cache()
    eng.close()
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--count-only", action="store_true", help="print the request and byte model, no device")
    ap.add_argument("--sizes", type=lambda s: tuple(1 << int(x) for x in s.split(",")), default=SIZES,
                    help="log2 of the index sizes, comma separated (default 22,24,26)")
    ap.add_argument("--out", default=None, help="write the result as JSON here too")
    args = ap.parse_args()
    if args.count_only:
        out = {"model": [model(n) for n in args.sizes]}
    else:
        out = {"m": M, "reps": REPS, "results": run(args)}
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
