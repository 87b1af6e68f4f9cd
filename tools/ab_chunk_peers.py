#!/usr/bin/env python3
"""Timing of the chunk peers (sdcas_dev_chunk_peers, csrc/chunk_peers.hip)
beside what it extends. A batch of m = 2^20 chunks of 4096 new files against
tools/ab_chunk_holders.py's holders index of n = 2^22 and 2^24 entries (real
keys; one pair, the all-zero chunk, held by n / 16 files, the others by 4 on
average), at max_holders H = 16 and 64, k = 4, EARLIER mode with file ids above
every stored one, so every holder counts. Legs alternating in ONE process, HIP
events around each, 20 repetitions after a warm-up, median and min:
  peers_plan     sdcas_dev_chunk_peers with max_pairs = min(m H, 2^30), the
                 plan's bound: what a caller that knows nothing passes
  peers_exact    the same with max_pairs = P, the batch's pairs, as
                 ChunkHolders.peers passes after its counting call
  peers_count    that counting call: no outputs, max_pairs = 0
  holders_match  sdcas_dev_chunk_holders_match of the same batch: the floor,
                 it finds the same runs
  sharing        sdcas_dev_chunk_sharing of the same batch (rep from
                 sdcas_dev_confirm_duplicates, outside the timing): the
                 lowest-holder answer the peers extend

Half of the batch's chunks are stored pairs, drawn by entry, so long runs are
drawn more often and about 1 in 32 chunks is the all-zero chunk, which is
common at both H. Before any time is taken every output of both peers legs is
compared with the tool's own numpy reference.

--count-only prints the request and byte model without a device. No ratio is
set in advance: the numbers go to profiles/chunk_peers.json and DESIGN.md §3.9.

The batches here have about 2.7 M pairs; only the plan's bound at H = 64 (2^26
places, nearly all of them empty) is sized past the scans' third level. Pairs
and chunks past 2^24, where that level carries sums, are covered by the suite:
tests/test_gpu_index_scale.py, both modes, against a dense torch reference.

The model. Per chunk three halvings (the pair's two bounds inside its bucket,
the triple's lower bound) and 16 bytes of run description written; the scan of
the counts; per pair place one halving in the offsets (ceil_log2(m) steps) and
20 bytes written; two merge sorts of ceil_log2(max_pairs) passes, each pass one
halving per live item in the sibling run and every pass's grid sized from
max_pairs, not from P; a u64 and a u32 scan over the places; per edge one
halving by file. 57 bytes of workspace per pair place, 16 per chunk."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from spacedrive_amd import _native as N  # noqa: E402
import ab_chunk_holders as AH  # noqa: E402

M = 1 << 20
SIZES = (1 << 22, 1 << 24)
HS = (16, 64)
K = 4
N_FILES = 4096
REPS = 20
COUNTS = [name for name, _ in N.PeersCounts._fields_]


def plan(m, n_files, k, h):
    pairs, ws = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = N.load().sdcas_chunk_peers_plan(m, n_files, k, h, ctypes.byref(pairs), ctypes.byref(ws))
    assert rc == N.SDCAS_OK, rc
    return int(pairs.value), int(ws.value)


def model(n, h, m=M, n_files=N_FILES, k=K):
    bits = AH.dir_bits(n)
    bucket = n / (1 << bits)
    q, ws = plan(m, n_files, k, h)
    return {"n": n, "m": m, "n_files": n_files, "k": k, "max_holders": h, "bits": bits, "entries_per_bucket": bucket,
            "halvings_per_chunk": 3, "steps_per_bucket_halving": max(1, int(np.ceil(np.log2(bucket + 1)))),
            "plan_max_pairs": q, "merge_passes_at_plan_bound": AH.ceil_log2(q), "sorts": 2,
            "workspace_bytes_at_plan_bound": ws, "workspace_bytes_per_pair": 57, "workspace_bytes_per_chunk": 16,
            "offset_steps_per_pair": AH.ceil_log2(m + 1), "batch_bytes_in": m * (8 + 32 + 4 + 8) + 8 * n_files,
            "bytes_out": n_files * (4 + 16 * k + 24) + 56}


def reference(hindex, qk, qd, chunk_file, chunk_len, n_files, k, h):
    """numpy, EARLIER mode with every file id above every stored value: keys are unique per pair, so a key finds
    its run and the whole run counts -> (outputs dict, counts)"""
    ik, idg, iv = hindex
    n, m = ik.size, qk.size
    first = np.searchsorted(ik, qk, side="left")
    last = np.searchsorted(ik, qk, side="right")
    at = np.minimum(first, n - 1)
    hit = (last > first) & (idg[at] == qd).all(axis=1)
    cnt = np.where(hit, last - first, 0)
    common, scoring = cnt > h, (cnt > 0) & (cnt <= h)

    def total(mask):
        out = np.zeros(n_files, np.uint64)
        np.add.at(out, chunk_file[mask], chunk_len[mask])
        return out
    c = np.flatnonzero(scoring)
    reps = cnt[c]
    pc = np.repeat(c, reps)
    j = np.arange(pc.size) - np.repeat(np.cumsum(reps) - reps, reps)
    holder = iv[first[pc] + j]
    edge = chunk_file[pc].astype(np.uint64) << np.uint64(32) | holder  # stored ids are below 2^32 here
    order = np.argsort(edge, kind="stable")
    e_sorted, l_sorted = edge[order], chunk_len[pc][order]
    head = np.concatenate([[True], e_sorted[1:] != e_sorted[:-1]]) if pc.size else np.zeros(0, bool)
    starts = np.flatnonzero(head)
    e_bytes = np.add.reduceat(l_sorted, starts) if pc.size else np.zeros(0, np.uint64)
    e_file, e_holder = (e_sorted[starts] >> np.uint64(32)).astype(np.int64), e_sorted[starts] & np.uint64(0xFFFFFFFF)
    by = np.lexsort((e_holder, -e_bytes.astype(np.int64), e_file))  # lengths are far below 2^63
    e_file, e_holder, e_bytes = e_file[by], e_holder[by], e_bytes[by]
    f_first = np.searchsorted(e_file, np.arange(n_files), side="left")
    rank = np.arange(e_file.size) - f_first[e_file]
    keep = rank < k
    peers, pb = np.zeros((n_files, k), np.uint64), np.zeros((n_files, k), np.uint64)
    peers[e_file[keep], rank[keep]], pb[e_file[keep], rank[keep]] = e_holder[keep], e_bytes[keep]
    per_file = np.bincount(e_file, minlength=n_files)
    out = {"peer_count": np.minimum(per_file, k).astype(np.uint32), "peers": peers, "peer_bytes": pb,
           "shared": total(scoring), "unique": total(cnt == 0), "common": total(common)}
    counts = dict(files=n_files, chunks=m, common_chunks=int(common.sum()), pairs=int(pc.size), edges=int(e_file.size),
                  files_with_peer=int((per_file > 0).sum()), overflow=0)
    return out, counts


def run(args):
    import torch
    from spacedrive_amd import Engine
    eng = Engine()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    eng.dev_bind_stream(s)
    results = []
    p = lambda t: t.data_ptr() if t.numel() else 0  # noqa: E731
    with torch.cuda.stream(stream):
        for n in args.sizes:
            index, _, queries = AH.make(n, M, seed=n)
            ik, idg, iv, idr, bits = index
            hindex = AH.host(index)
            qk, qd = queries
            g = torch.Generator(device="cuda").manual_seed(n + 1)
            d_file = torch.sort(torch.randint(0, N_FILES, (M,), device="cuda", generator=g)).values.to(torch.int32)
            d_len = torch.randint(2048, 65537, (M,), dtype=torch.int64, device="cuda", generator=g)
            d_ids = torch.arange(AH.IDS + 1, AH.IDS + 1 + N_FILES, dtype=torch.int64, device="cuda")
            h_qk, h_qd = qk.cpu().numpy().view(np.uint64), qd.cpu().numpy().reshape(-1, 32)
            h_file, h_len = d_file.cpu().numpy().astype(np.int64), d_len.cpu().numpy().view(np.uint64)
            rep = torch.empty(M, dtype=torch.int64, device="cuda")
            eng.dev_confirm_duplicates(p(qk), p(qd), 0, M, rep=rep.data_ptr(), stream=s)
            outs = {"peer_count": torch.empty(N_FILES, dtype=torch.int32, device="cuda"),
                    "peers": torch.empty(N_FILES * K, dtype=torch.int64, device="cuda"),
                    "peer_bytes": torch.empty(N_FILES * K, dtype=torch.int64, device="cuda"),
                    "shared": torch.empty(N_FILES, dtype=torch.int64, device="cuda"),
                    "unique": torch.empty(N_FILES, dtype=torch.int64, device="cuda"),
                    "common": torch.empty(N_FILES, dtype=torch.int64, device="cuda")}
            cts = torch.zeros(7, dtype=torch.int64, device="cuda")
            pos, val = (torch.empty(M, dtype=torch.int64, device="cuda") for _ in range(2))
            hold = torch.empty(M, dtype=torch.int32, device="cuda")
            mc = torch.zeros(4, dtype=torch.int64, device="cuda")
            sh = [torch.empty(N_FILES, dtype=torch.int64, device="cuda") for _ in range(5)]
            sc = torch.zeros(6, dtype=torch.int64, device="cuda")
            for h in args.holders:
                want, wcounts = reference(hindex, h_qk, h_qd, h_file, h_len, N_FILES, K, h)
                bound = plan(M, N_FILES, K, h)[0]

                def peers_leg(max_pairs, with_outputs=True, h=h):
                    o = [p(outs[name]) for name in ("peer_count", "peers", "peer_bytes", "shared", "unique", "common")] \
                        if with_outputs else [0] * 6
                    return lambda: eng.dev_chunk_peers(p(ik), p(idg), p(iv), p(idr), n, bits, p(qk), p(qd), 0, p(d_file),
                                                       p(d_len), M, p(d_ids), N_FILES, K, h, N.SDCAS_PEERS_EARLIER,
                                                       max_pairs, *o, cts.data_ptr(), stream=s)

                legs = {"peers_plan": peers_leg(bound), "peers_exact": peers_leg(wcounts["pairs"]),
                        "peers_count": peers_leg(0, False),
                        "holders_match": lambda: eng.dev_chunk_holders_match(p(ik), p(idg), p(iv), p(idr), n, bits, p(qk),
                                                                             p(qd), 0, M, p(pos), p(val), p(hold),
                                                                             mc.data_ptr(), stream=s),
                        "sharing": lambda: eng.dev_chunk_sharing(p(d_file), p(d_len), rep.data_ptr(), M, N_FILES,
                                                                 *(t.data_ptr() for t in sh), sc.data_ptr(), stream=s)}
                checks = {}
                for name in ("peers_plan", "peers_exact"):  # the warm-up, and the runs that are checked
                    for t in outs.values():
                        t.fill_(-1)
                    legs[name]()
                    stream.synchronize()
                    got = dict(zip(COUNTS, (int(x) for x in cts.cpu())))
                    checks[name] = got == wcounts and all(
                        bool((outs[key].cpu().numpy().view(want[key].dtype).reshape(want[key].shape) == want[key]).all())
                        for key in want)
                legs["peers_count"]()
                stream.synchronize()
                got = dict(zip(COUNTS, (int(x) for x in cts.cpu())))
                checks["peers_count"] = got == dict(wcounts, edges=0, files_with_peer=0, overflow=int(wcounts["pairs"] > 0))
                legs["holders_match"](), legs["sharing"]()
                stream.synchronize()
                if not all(checks.values()):
                    print(json.dumps({"n": n, "max_holders": h, "checks": checks}))
                    raise SystemExit(f"n = {n}, H = {h}: an output differs from the reference")
                times = {name: [] for name in legs}
                for _ in range(args.reps):
                    for name, f in legs.items():
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        f()
                        b.record(stream)
                        b.synchronize()
                        times[name].append(a.elapsed_time(b) * 1000.0)
                us = {name: {"median": float(np.median(v)), "min": float(np.min(v))} for name, v in times.items()}
                r = {"model": model(n, h), "counts": wcounts, "checks": checks, "us": us,
                     "over_holders_match": {name: v["median"] / us["holders_match"]["median"] for name, v in us.items()
                                            if name.startswith("peers_")},
                     "over_sharing": {name: v["median"] / us["sharing"]["median"] for name, v in us.items()
                                      if name.startswith("peers_")}}
                results.append(r)
                print(json.dumps({"n": n, "max_holders": h, "counts": wcounts, "us": us}), flush=True)
                if args.out:  # what is measured so far, should a later size not finish
                    with open(args.out, "w") as f:
                        f.write(json.dumps({"m": M, "reps": args.reps, "results": results}, indent=1) + "\n")
            del index, queries, hindex, ik, idg, iv, idr, qk, qd, legs
            torch.cuda.empty_cache()
    eng.close()
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--count-only", action="store_true", help="print the request and byte model, no device")
    ap.add_argument("--sizes", type=lambda s: tuple(1 << int(x) for x in s.split(",")), default=SIZES,
                    help="log2 of the index sizes, comma separated (default 22,24)")
    ap.add_argument("--holders", type=lambda s: tuple(int(x) for x in s.split(",")), default=HS,
                    help="the max_holders values, comma separated (default 16,64)")
    ap.add_argument("--reps", type=int, default=REPS, help="timed repetitions of every leg (default 20)")
    ap.add_argument("--out", default=None, help="write the result as JSON here too")
    args = ap.parse_args()
    if args.count_only:
        out = {"model": [model(n, h) for n in args.sizes for h in args.holders]}
    else:
        out = {"m": M, "reps": args.reps, "results": run(args)}
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
