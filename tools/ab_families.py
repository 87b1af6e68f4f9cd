#!/usr/bin/env python3
"""Timing of the file families (sdcas_dev_file_families, csrc/families.hip)
beside the existing group-by of the same n. n = 2^20 and 2^22 rows, k = 4, ids
2 i + 1 (so every even id is missing), every size 1000, threshold 1/2. Legs
alternating in ONE process, HIP events around each, 20 repetitions after a
warm-up, median and min:
  families_random  a random graph: rows in blocks of 32; slot 0 links a random
                   row of the block (half of the rows; the others name it
                   weakly), slot 3 links inside the block for a quarter of
                   the rows and is the row itself for the rest
  families_chain   the ascending chain: slot 0 of row i lists row i - 1. When
                   all its hooks land at once they build a tree of depth n:
                   the case the jump passes exist for
  families_star    the star on the LAST row: slot 0 of every row lists row
                   n - 1, every hook contends for one root
                   (in all three, slot 1 names a random row weakly, slot 2 a
                   missing id, and in the chain and the star slot 3 is the row
                   itself: the slots read are the same 4 n, only the links
                   differ)
  sets             sdcas_dev_duplicate_sets over families_random's labels: the
                   yardstick, the existing group-by of the same n
What to read off: chain : random and star : random at equal n, the measured
price of the one data-dependent loop (find inside k_ff_union). Before any time
is taken every output of the three families legs is compared with the tool's
own numpy reference (min-label hooking and pointer jumping, vectorised).

--count-only prints the byte and request model without a device. No ratio is
set in advance: the numbers go to profiles/file_families.json and DESIGN.md
§3.10. The split by kernel is a run of its own under the profiler,
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
      python tools/ab_families.py --sizes 20 --reps 5
whose kernel_stats.csv is kept as profiles/file_families_kernel_stats.csv.

The model. Per row 8 bytes of workspace (parent, size); per slot one halving in
ids (ceil_log2(n + 1) steps) and, on a link, one unite; ceil_log2(n) jump
launches, of which those behind a pass that moved nothing read one word and
leave; one atomic add per row for the sizes (one per wave where a wave's rows
share a root)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spacedrive_amd import _native as N  # noqa: E402

SIZES = (1 << 20, 1 << 22)
K = 4
NUM, DEN = 1, 2
SIZE, STRONG, FAINT = 1000, 600, 100
BLOCK = 32
REPS = 20
COUNTS = [name for name, _ in N.FamiliesCounts._fields_]


def ceil_log2(n):
    return max(0, int(n) - 1).bit_length()


def plan(n, k):
    ws = ctypes.c_uint64(0)
    rc = N.load().sdcas_file_families_plan(n, k, ctypes.byref(ws))
    assert rc == N.SDCAS_OK, rc
    return int(ws.value)


def model(n, k=K):
    return {"n": n, "k": k, "num": NUM, "den": DEN, "workspace_bytes": plan(n, k), "workspace_bytes_per_row": 8,
            "halvings_per_slot": 1, "steps_per_halving": ceil_log2(n + 1), "jump_launches": ceil_log2(n),
            "launches": 5 + ceil_log2(n), "bytes_in": n * (8 + 8 + 4 + 16 * k), "bytes_out": n * (8 + 4) + 80,
            "sets_workspace_bytes_per_row": 36}


def graph(kind, n, k=K, seed=0):
    """-> ids, sizes, peer_count u32[n], peers u64[n, k], peer_bytes u64[n, k]"""
    rng = np.random.default_rng(seed + n)
    rows = np.arange(n, dtype=np.int64)
    ids = (2 * rows + 1).astype(np.uint64)
    sizes = np.full(n, SIZE, np.uint64)
    peers, pb = np.zeros((n, k), np.uint64), np.zeros((n, k), np.uint64)
    count = np.full(n, k, np.uint32)
    peers[:, 1], pb[:, 1] = ids[rng.integers(0, n, n)], FAINT
    peers[:, 2], pb[:, 2] = 2 * rng.integers(0, n, n).astype(np.uint64), STRONG
    peers[:, 3], pb[:, 3] = ids, STRONG
    if kind == "chain":
        peers[1:, 0], pb[1:, 0] = ids[:-1], STRONG
        peers[0, 0] = ids[0]
    elif kind == "star":
        peers[:, 0], pb[:, 0] = ids[-1], STRONG
    elif kind == "random":
        base = rows // BLOCK * BLOCK

        def inside():
            return ids[np.minimum(base + rng.integers(0, BLOCK, n), n - 1)]
        peers[:, 0], pb[:, 0] = inside(), np.where(rng.random(n) < 0.5, STRONG, FAINT)
        peers[:, 3] = np.where(rng.random(n) < 0.25, inside(), ids)
    else:
        raise ValueError(kind)
    return ids, sizes, count, peers, pb


def components(n, src, dst):
    """the lowest row of every row's component: hook the larger label under the smaller, jump until flat, repeat"""
    lab = np.arange(n, dtype=np.int64)
    while src.size:
        a, b = lab[src], lab[dst]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        live = lo != hi
        if not live.any():
            break
        np.minimum.at(lab, hi[live], lo[live])
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    return lab


def reference(ids, sizes, count, peers, pb, num=NUM, den=DEN):
    """numpy; the sizes and bytes of this tool are far below 2^31, so no product wraps"""
    n, k = peers.shape
    read = np.arange(k)[None, :] < np.minimum(count, k)[:, None]
    at = np.searchsorted(ids, peers)
    j = np.minimum(at, n - 1)
    found = (at < n) & (ids[j] == peers)
    own = found & (peers == ids[:, None])
    big = np.maximum(sizes[:, None], sizes[j])
    strong = (pb > 0) & (pb * np.uint64(den) >= np.uint64(num) * big)
    link = read & found & ~own & strong
    i_of = np.broadcast_to(np.arange(n)[:, None], (n, k))
    family = components(n, i_of[link], j[link])
    size = np.bincount(family, minlength=n)
    roots = size[size >= 2]
    counts = dict(files=n, slots=int(read.sum()), missing=int((read & ~found).sum()), self_slots=int((read & own).sum()),
                  weak=int((read & found & ~own & ~strong).sum()), links=int(link.sum()), families=int(roots.size),
                  members=int(roots.sum()), largest=int(roots.max()) if roots.size else 0, unsorted=0)
    return family.astype(np.int64), size[family].astype(np.uint32), counts


def run(args):
    import torch
    from spacedrive_amd import Engine
    eng = Engine()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    eng.dev_bind_stream(s)
    results = []
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()  # noqa: E731
    with torch.cuda.stream(stream):
        for n in args.sizes:
            family = torch.empty(n, dtype=torch.int64, device="cuda")
            fsize = torch.empty(n, dtype=torch.int32, device="cuda")
            cts = torch.zeros(10, dtype=torch.int64, device="cuda")
            set_rep, set_bytes = (torch.empty(n // 2, dtype=torch.int64, device="cuda") for _ in range(2))
            set_off = torch.empty(n // 2 + 1, dtype=torch.int64, device="cuda")
            members = torch.empty(n, dtype=torch.int64, device="cuda")
            scts = torch.zeros(6, dtype=torch.int64, device="cuda")
            legs, checks, allcounts, keep = {}, {}, {}, []
            for kind in ("random", "chain", "star"):
                g = graph(kind, n)
                want_family, want_size, want_counts = reference(*g)
                d = [up(g[0], np.int64), up(g[1], np.int64), up(g[2], np.int32), up(g[3], np.int64), up(g[4], np.int64)]
                keep.append(d)
                legs["families_" + kind] = lambda d=d: eng.dev_file_families(
                    *(t.data_ptr() for t in d), n, K, NUM, DEN, family.data_ptr(), fsize.data_ptr(), cts.data_ptr(), stream=s)
                family.fill_(-1), fsize.fill_(-1)
                legs["families_" + kind]()  # the warm-up, and the run that is checked
                stream.synchronize()
                got = dict(zip(COUNTS, (int(x) for x in cts.cpu())))
                checks[kind] = bool(got == want_counts and np.array_equal(family.cpu().numpy(), want_family) and
                                    np.array_equal(fsize.cpu().numpy().view(np.uint32), want_size))
                allcounts[kind] = want_counts
                if kind == "random":
                    labels = family.clone()
                del g, want_family, want_size
            legs["sets"] = lambda: eng.dev_duplicate_sets(labels.data_ptr(), 0, n, set_rep.data_ptr(), set_off.data_ptr(),
                                                          0, members.data_ptr(), scts.data_ptr(), stream=s)
            legs["sets"]()
            stream.synchronize()
            sets_counts = [int(x) for x in scts.cpu()]
            checks["sets"] = sets_counts[1] == allcounts["random"]["families"] and \
                sets_counts[2] == allcounts["random"]["members"]
            if not all(checks.values()):
                print(json.dumps({"n": n, "checks": checks}))
                raise SystemExit(f"n = {n}: an output differs from the reference")
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
            base = us["families_random"]["median"]
            r = {"model": model(n), "counts": allcounts, "checks": checks, "us": us,
                 "chain_over_random": us["families_chain"]["median"] / base,
                 "star_over_random": us["families_star"]["median"] / base,
                 "over_sets": {name: v["median"] / us["sets"]["median"] for name, v in us.items()
                               if name.startswith("families_")}}
            results.append(r)
            print(json.dumps({"n": n, "us": us, "chain_over_random": r["chain_over_random"],
                              "star_over_random": r["star_over_random"]}), flush=True)
            if args.out:  # what is measured so far, should a later size not finish
                with open(args.out, "w") as f:
                    f.write(json.dumps({"k": K, "reps": args.reps, "results": results}, indent=1) + "\n")
            del legs, keep, labels
            torch.cuda.empty_cache()
    eng.close()
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--count-only", action="store_true", help="print the byte and request model, no device")
    ap.add_argument("--sizes", type=lambda s: tuple(1 << int(x) for x in s.split(",")), default=SIZES,
                    help="log2 of the row counts, comma separated (default 20,22)")
    ap.add_argument("--reps", type=int, default=REPS, help="timed repetitions of every leg (default 20)")
    ap.add_argument("--out", default=None, help="write the result as JSON here too")
    args = ap.parse_args()
    if args.count_only:
        out = {"model": [model(n) for n in args.sizes]}
    else:
        out = {"k": K, "reps": args.reps, "results": run(args)}
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
