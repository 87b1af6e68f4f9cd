#!/usr/bin/env python3
"""Timing of the (cas key, checksum) group-by (sdcas_dev_confirm_duplicates,
csrc/confirm.hip) beside the existing 8-byte group-by (sdcas_dev_dedup) over
the same keys as the yardstick, the two alternating in ONE process, HIP events
around work that ends in a sync, 20 repetitions after a warm-up.

Workload: a C5-shaped share, 6.25 M files (rank 0 of 8 of the 50 M-file
corpus, bench.c5_share), content ids from synth.c5_content_ids_at; the cas key
is the content key, the digest is derived from the content id, and every
1000th content id (the Zipf head, content 0, among them) gives its copies two
different digests, so collisions exist.

No threshold: the numbers are recorded (--out, default
profiles/confirm_duplicates.json): both medians, their ratio, and the bytes
per file of the model below. --count-only prints the model without a device.

The model (the least HBM traffic of the scheme, every probe finding its slot
at once; n files, C classes, K keys, table capacity cap = 2^k >= 2n):
  clear    2 * cap * 4 (both tables) + 4 n (class counters) written
  insert   per file 8 + 32 + 1 read (key, digest, valid), one word of each
           table probed (8), two slots written (8); a file that finds its class
           (key) claimed gathers the claimer's 40 (8) bytes: 40 (n - C) + 8 (n - K)
  classes  per file its class slot and that table word (8); a class's lowest
           file also its key slot, that table word and the counter (12 C)
  write    per file two slots, two table words, the counter (20) read;
           rep, key_rep, flags (17) written"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from spacedrive_amd import synth as S  # noqa: E402

_U = np.uint64


def workload(n, world=8):
    """(keys uint64[n], digests uint8[n, 32]) of rank 0's C5-shaped share"""
    fi = bench.c5_share(0, n, world).astype(_U)
    cid = S.c5_content_ids_at(fi)
    keys = S.content_key(S.SEED_C5, cid)
    # every 1000th content id: its copies alternate between two digests
    variant = np.where(cid % _U(1000) == _U(0), np.arange(n, dtype=_U) & _U(1), _U(0))
    with np.errstate(over="ignore"):
        words = S.mix64(((cid * _U(2) + variant) * _U(4))[:, None] + np.arange(4, dtype=_U)[None, :])
    return keys, np.ascontiguousarray(words).view(np.uint8).reshape(n, 32)


def model(keys, digests):
    n = keys.size
    cap = 64
    while cap < 2 * n:
        cap <<= 1
    k = np.unique(keys).size
    rec = np.empty(n, dtype=[("k", _U), ("d", _U, 4)])
    rec["k"] = keys
    rec["d"] = digests.view(_U).reshape(n, 4)
    c = np.unique(rec).size
    clear = 2 * cap * 4 + 4 * n
    insert = n * (8 + 32 + 1 + 8 + 8) + 40 * (n - c) + 8 * (n - k)
    classes = 8 * n + 12 * c
    write = n * (20 + 17)
    total = clear + insert + classes + write
    return {"files": n, "classes": int(c), "keys": int(k), "table_capacity": cap,
            "bytes": {"clear": clear, "insert": insert, "classes": classes, "write": write, "total": total},
            "bytes_per_file": total / n}


def device(a, keys, digests, res):
    import torch
    from spacedrive_amd import Engine
    dev = torch.device("cuda", 0)
    n = keys.size
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    dk = t(keys)
    dd = torch.from_numpy(digests).to(dev)
    has = torch.ones(n, dtype=torch.uint8, device=dev)
    rep = torch.zeros(n, dtype=torch.int64, device=dev)
    krep = torch.zeros(n, dtype=torch.int64, device=dev)
    fl = torch.zeros(n, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(6, dtype=torch.int64, device=dev)
    link = torch.zeros(n, dtype=torch.int64, device=dev)
    dcnt = torch.zeros(2, dtype=torch.int64, device=dev)
    eng = Engine()
    stream = torch.cuda.Stream()  # a stream of its own: handle 0 would name the context's stream, not torch's
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    legs = {
        "confirm": lambda: eng.dev_confirm_duplicates(dk.data_ptr(), dd.data_ptr(), has.data_ptr(), n, rep.data_ptr(),
                                                      krep.data_ptr(), fl.data_ptr(), cnt.data_ptr(), sp),
        "dedup": lambda: eng.dev_dedup(dk.data_ptr(), has.data_ptr(), 0, n, 100, link.data_ptr(), dcnt.data_ptr(), sp),
    }
    ms = {k: [] for k in legs}
    for f in legs.values():  # warm both legs (each one's first call allocates its tables)
        for _ in range(2):
            f()
        eng.dev_sync(sp)
    for _ in range(a.reps):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            f()
            e1.record(stream)
            eng.dev_sync(sp)
            ms[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    counts = dict(zip(("files", "classes", "keys", "collided_keys", "collided_files", "duplicate_files"),
                      (int(x) for x in cnt.cpu().numpy())))
    m = res["model"]
    res["device"] = {
        "reps": a.reps, "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
        "confirm_over_dedup": med["confirm"] / med["dedup"],
        "confirm_model_GBps": m["bytes"]["total"] / (med["confirm"] * 1e-3) / 1e9,
        "confirm_files_per_s": n / (med["confirm"] * 1e-3),
        "counts": counts,
        "counts_match_model": counts["files"] == n and counts["classes"] == m["classes"] and counts["keys"] == m["keys"],
    }
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=6_250_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--count-only", action="store_true", help="the model's bytes alone: no device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confirm_duplicates.json"))
    a = ap.parse_args()
    keys, digests = workload(a.files)
    res = {"tool": "tools/ab_confirm.py", "model": model(keys, digests)}
    if a.count_only:
        print(json.dumps(res))
        return
    device(a, keys, digests, res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
