#!/usr/bin/env python3
"""Timing of the duplicate sets (sdcas_dev_duplicate_sets, csrc/dupsets.hip) in
both orders beside the call it follows, sdcas_dev_confirm_duplicates over the
same files, as the yardstick on the device: the three legs alternating in ONE
process, HIP events around work that ends in a sync, 20 repetitions after a
warm-up.

Workload: tools/ab_confirm.py's (a C5-shaped share, 6.25 M files, with its
seeded collisions); the sizes are the corpus's lengths (synth.c5_sizes_of).
Confirm runs once; its rep stays on the device and is what the sets are made
of.

A number of a DIFFERENT KIND beside them, `host_download_and_group`: the host
wall clock of what a caller does today: rep copied down, grouped with numpy
(stable argsort) on the host's CPUs. It is not a device time and is not
alternated with the legs.

Before any time is reported, the outputs of the timed size in both orders are
compared with that numpy grouping.

No threshold: the numbers are recorded (--out, default
profiles/duplicate_sets.json). --count-only prints the model without a device.

The model (the least HBM traffic of the scheme per pass; n files, P of them
taking part, S sets, M members, T = ceil(items / 4096) tiles of a pass, a
digit histogram 1 KiB per tile, written once, read twice and rewritten once by
its scan):
  clear       8 n written (the labels' counters and lowest files)
  count       8 n read; two atomics per participating file (8 P)
  heads       two passes of 8 n + 8 P read; per set 8 read (size), 12 written,
              and 12 more (sort key, value) by reclaimable
  set sort    by reclaimable only, 8 passes: per set 8 + 12 read, 12 written;
              4 KiB per tile of n / 2 + 1
  final       per set 12 + 8 read (4 more by reclaimable), 24 written
  offsets     per set 4 read + 4 read + 4 written (scan), 4 read + 8 written
  members     two passes of 8 n + 4 P read; per member 4 read, 8 written
  member sort ceil(bits(n / 2) / 8) passes: per member 4 + 8 read, 8 written;
              4 KiB per tile of n
  out         per member 4 read, 8 written"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import ab_confirm  # noqa: E402
import bench  # noqa: E402
from spacedrive_amd import synth as S  # noqa: E402

_U = np.uint64
TILE = 4096
HBM_PEAK_GBPS = 8000.0
COUNTS = ("files", "sets", "members", "duplicate_files", "reclaimable_bytes", "largest_set")


def workload(n, world=8):
    """(keys, digests, sizes uint64[n]) of rank 0's C5-shaped share"""
    keys, digests = ab_confirm.workload(n, world)
    cid = S.c5_content_ids_at(bench.c5_share(0, n, world).astype(_U))
    return keys, digests, np.ascontiguousarray(S.c5_sizes_of(cid), _U)


def class_rep(keys, digests):
    """what confirm answers with every file valid: the lowest file of each
    (key, digest), by a stable sort (the model needs no device)"""
    n = keys.size
    rec = np.empty(n, dtype=[("k", _U), ("d", _U, 4)])
    rec["k"] = keys
    rec["d"] = digests.view(_U).reshape(n, 4)
    _, inv = np.unique(rec, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(int(inv.max()) + 1 if n else 0, n, np.int64)
    np.minimum.at(first, inv, np.arange(n, dtype=np.int64))
    return first[inv]


def group(rep, sizes, by_reclaimable):
    """the numpy grouping: (set_rep, set_offsets, set_bytes, members, counts)"""
    n = rep.size
    part = np.flatnonzero((rep >= 0) & (rep < n))
    lab = rep[part]
    o = np.argsort(lab, kind="stable")
    idx, lab = part[o], lab[o]
    starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]]) if lab.size else np.zeros(0, np.int64)
    lens = np.diff(np.r_[starts, lab.size])
    keep = lens >= 2
    starts, lens = starts[keep], lens[keep]
    lowest = idx[starts].astype(np.int64)
    one = sizes[lowest]
    with np.errstate(over="ignore"):
        recl = (lens - 1).astype(_U) * one
    so = np.lexsort((lowest, ~recl)) if by_reclaimable else np.argsort(lowest, kind="stable")
    starts, lens, lowest, one, recl = starts[so], lens[so], lowest[so], one[so], recl[so]
    offs = np.r_[0, np.cumsum(lens)].astype(_U)
    m = int(offs[-1])
    members = idx[np.repeat(starts - offs[:-1].astype(np.int64), lens) + np.arange(m)].astype(np.int64)
    with np.errstate(over="ignore"):
        total = int(np.sum(recl, dtype=_U)) if recl.size else 0
    counts = dict(zip(COUNTS, (int(part.size), int(lens.size), m, m - int(lens.size), total,
                               int(lens.max()) if lens.size else 0)))
    return lowest, offs, one, members, counts


def model(n, counts):
    p, s, m = counts["files"], counts["sets"], counts["members"]
    tiles = lambda x: max(1, -(-x // TILE))
    h = n // 2 + 1
    bits = 1
    while (1 << bits) < n // 2:
        bits += 1
    mpasses = -(-bits // 8)
    passes = {
        "clear": 8 * n,
        "count": 8 * n + 8 * p,
        "heads": 2 * (8 * n + 8 * p) + 20 * s,
        "final": 44 * s,
        "offsets": 24 * s,
        "members": 2 * (8 * n + 4 * p) + 12 * m,
        "member_sort": mpasses * (20 * m + 4096 * tiles(n)),
        "out": 12 * m,
    }
    by_rep = sum(passes.values())
    extra = {"heads_keys": 12 * s, "set_sort": 8 * (32 * s + 4096 * tiles(h)), "final_perm": 4 * s}
    by_recl = by_rep + sum(extra.values())
    return {"files": n, "participating": p, "sets": s, "members": m, "member_sort_passes": mpasses,
            "bytes_by_rep": passes, "bytes_extra_by_reclaimable": extra,
            "bytes_per_file": {"by_rep": by_rep / n, "by_reclaimable": by_recl / n},
            "ms_at_hbm_peak": {"by_rep": by_rep / HBM_PEAK_GBPS / 1e6, "by_reclaimable": by_recl / HBM_PEAK_GBPS / 1e6},
            "workspace_bytes_per_file": 36 + 1024 / TILE}


def device(a, keys, digests, sizes, res):
    import torch
    from spacedrive_amd import Engine
    dev = torch.device("cuda", 0)
    n = keys.size
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    dk, dsz = t(keys), t(sizes)
    dd = torch.from_numpy(digests).to(dev)
    has = torch.ones(n, dtype=torch.uint8, device=dev)
    rep = torch.zeros(n, dtype=torch.int64, device=dev)
    krep = torch.zeros(n, dtype=torch.int64, device=dev)
    fl = torch.zeros(n, dtype=torch.uint8, device=dev)
    ccnt = torch.zeros(6, dtype=torch.int64, device=dev)
    h = n // 2
    outs = [torch.zeros(max(c, 1), dtype=torch.int64, device=dev) for c in (h, h + 1, h, n, 6)]
    eng = Engine()
    stream = torch.cuda.Stream()  # a stream of its own: handle 0 would name the context's stream, not torch's
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    confirm = lambda: eng.dev_confirm_duplicates(dk.data_ptr(), dd.data_ptr(), has.data_ptr(), n, rep.data_ptr(),
                                                 krep.data_ptr(), fl.data_ptr(), ccnt.data_ptr(), sp)
    sets = lambda order: eng.dev_duplicate_sets(rep.data_ptr(), dsz.data_ptr(), n, *(o.data_ptr() for o in outs),
                                                order, sp)
    confirm()
    eng.dev_sync(sp)

    # the host leg, and the answer everything is compared with
    host_s = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        hrep = rep.cpu().numpy()
        want_rep_order = group(hrep, sizes, False)
        host_s.append(time.perf_counter() - t0)
    wants = {0: want_rep_order, 1: group(hrep, sizes, True)}
    equal = {}
    for order, name in ((0, "by_rep"), (1, "by_reclaimable")):
        for o in outs:
            o.fill_(-7)
        torch.cuda.synchronize()
        sets(order)
        eng.dev_sync(sp)
        got = [o.cpu().numpy() for o in outs]
        w = wants[order]
        s, m = w[4]["sets"], w[4]["members"]
        equal[name] = bool(
            dict(zip(COUNTS, (int(x) for x in got[4].view(_U)))) == w[4] and (got[0][:s] == w[0]).all() and
            (got[1][:s + 1].view(_U) == w[1]).all() and (got[2][:s].view(_U) == w[2]).all() and
            (got[3][:m] == w[3]).all() and (got[0][s:] == -7).all() and (got[3][m:] == -7).all())
    res["model"] = model(n, wants[0][4])
    res["outputs_equal_numpy_grouping"] = equal
    if not all(equal.values()):
        res["device"] = "outputs differ from the numpy grouping: no time is reported"
        eng.close()
        return

    legs = {"sets_by_rep": lambda: sets(0), "sets_by_reclaimable": lambda: sets(1), "confirm": confirm}
    ms = {k: [] for k in legs}
    for f in legs.values():
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
    host_ms = float(np.median(host_s)) * 1e3
    mo = res["model"]
    res["device"] = {
        "reps": a.reps, "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
        "over_confirm": {k: med[k] / med["confirm"] for k in ("sets_by_rep", "sets_by_reclaimable")},
        "model_GBps": {"sets_by_rep": mo["bytes_per_file"]["by_rep"] * n / (med["sets_by_rep"] * 1e-3) / 1e9,
                       "sets_by_reclaimable":
                           mo["bytes_per_file"]["by_reclaimable"] * n / (med["sets_by_reclaimable"] * 1e-3) / 1e9},
        "hbm_peak_GBps": HBM_PEAK_GBPS,
        "counts": wants[0][4],
    }
    res["host_download_and_group"] = {
        "what": "host wall clock, a different kind of number: rep copied down and grouped with numpy in set_rep "
                "order (stable argsort), not a device time",
        "reps": a.host_reps, "median_ms": host_ms, "min_ms": float(np.min(host_s)) * 1e3,
        "cpus": len(os.sched_getaffinity(0)),
        "over_device_by_rep": host_ms / med["sets_by_rep"],
    }
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=6_250_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--count-only", action="store_true", help="the model's bytes alone: no device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duplicate_sets.json"))
    a = ap.parse_args()
    keys, digests, sizes = workload(a.files)
    res = {"tool": "tools/ab_sets.py"}
    if a.count_only:
        res["model"] = model(a.files, group(class_rep(keys, digests), sizes, False)[4])
        print(json.dumps(res))
        return
    device(a, keys, digests, sizes, res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
