#!/usr/bin/env python3
"""Timing of the family bytes (sdcas_dev_family_bytes, csrc/family_bytes.hip)
beside the existing sharing pass over the same arrays. m = 2^20 and 2^22
chunks, n_files = m / 64, 64 adjacent chunks per file but in the last leg.
Legs alternating in ONE process, HIP events around each, 20 repetitions after a
warm-up, median and min:
  bytes_random     families of 1 to 16 consecutive rows; about half of the
                   chunks repeat an earlier chunk of their family (confirm-style
                   reps that never leave the family)
  bytes_one_class  every chunk is one class in one family (the zero chunk of
                   sparse images): every insert aims at one table word
  bytes_one_file   one file holds every chunk, all classes distinct, one
                   family: every sum aims at one row
  sharing          sdcas_dev_chunk_sharing over bytes_random's arrays: the
                   yardstick, the existing pass that answers the same question
                   corpus-wide
What to read off: every bytes leg against bytes_random and against sharing.
Before any time is taken every output of the three bytes legs is compared with
the tool's own numpy reference, and sharing's new / self / other with
bytes_random's delta / self / inherited (its reps stay inside the families, so
the two agree).

--count-only prints the byte and launch model without a device. No ratio is set
in advance: the numbers go to profiles/family_bytes.json and DESIGN.md §3.11.
The split by kernel is a run of its own under the profiler,
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
      python tools/ab_family_bytes.py --sizes 20 --reps 5
whose kernel_stats.csv is kept as profiles/family_bytes_kernel_stats.csv.

The model. A table of 2 m u32 slots (the power of two at or above), 4 bytes per
chunk for its slot and 65 bytes per row; two fills, the insert and the classify
over m, the rows and the heads over n_files, ceil_log2(n_files) merge launches,
the write and the totals."""
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
PER_FILE = 64
REPS = 20
COUNTS = [name for name, _ in N.FamilyBytesCounts._fields_]
ROWS = ("file_bytes", "delta_bytes", "self_bytes", "inherited_bytes")
SETS = ("set_rep", "set_files", "set_total", "set_stored")
KINDS = ("random", "one_class", "one_file")


def ceil_log2(n):
    return max(0, int(n) - 1).bit_length()


def plan(m, n):
    ws = ctypes.c_uint64(0)
    rc = N.load().sdcas_family_bytes_plan(m, n, ctypes.byref(ws))
    assert rc == N.SDCAS_OK, rc
    return int(ws.value)


def table_slots(m):
    return max(16, 1 << ceil_log2(2 * m))


def model(m):
    n = m // PER_FILE
    return {"m": m, "n_files": n, "workspace_bytes": plan(m, n), "table_slots": table_slots(m),
            "workspace_bytes_per_chunk": 4, "workspace_bytes_per_row": 65, "fills": 2,
            "merge_launches": ceil_log2(n), "launches": 6 + ceil_log2(n),
            "bytes_in": m * (4 + 8 + 8) + n * 8, "bytes_out": n * 32 + (n // 2) * (8 + 4 + 8 + 8) + 72,
            "sharing_bytes_in": m * (4 + 8 + 8), "sharing_bytes_out": n * 40 + 48}


def corpus(kind, m, seed=0):
    """-> chunk_file u32[m], chunk_len u64[m], rep i64[m], family i64[n]"""
    rng = np.random.default_rng(seed + m)
    n = max(m // PER_FILE, 1)
    pos = np.arange(m, dtype=np.int64)
    chunk_len = rng.integers(1, 1 << 16, m).astype(np.uint64)
    if kind == "one_file":
        return np.zeros(m, np.uint32), chunk_len, pos.copy(), np.zeros(n, np.int64)
    chunk_file = np.minimum(pos // PER_FILE, n - 1).astype(np.uint32)
    if kind == "one_class":
        return chunk_file, chunk_len, np.zeros(m, np.int64), np.zeros(n, np.int64)
    if kind != "random":
        raise ValueError(kind)
    # families: runs of 1 to 16 rows, labelled by their first row
    starts = np.cumsum(rng.integers(1, 17, n))
    starts = np.concatenate([[0], starts[starts < n]])
    head = np.zeros(n, bool)
    head[starts] = True
    family = np.maximum.accumulate(np.where(head, np.arange(n), 0)).astype(np.int64)
    # the family's first chunk, and for half of the others a random earlier chunk of the family,
    # snapped down to the last chunk at or below it that stands for itself
    first_row = np.searchsorted(chunk_file, family[chunk_file], side="left")
    own = (rng.random(m) < 0.5) | (pos == first_row)
    target = first_row + (rng.random(m) * (pos - first_row + 1)).astype(np.int64)
    last_own = np.maximum.accumulate(np.where(own, pos, 0))
    rep = np.where(own, pos, last_own[np.minimum(target, pos)])
    return chunk_file, chunk_len, rep.astype(np.int64), family


def reference(chunk_file, chunk_len, rep, family):
    """numpy, exact modulo 2^64 -> dict with the four per-row arrays, the four set arrays and "counts\""""
    m, n = chunk_file.size, family.size
    pos = np.arange(m, dtype=np.int64)
    row_ok = (family >= 0) & (family < n)
    cf = chunk_file.astype(np.int64)
    on = (cf < n) & (row_ok[np.minimum(cf, n - 1)] if n else np.zeros(m, bool))
    idx = pos[on]
    rows = cf[idx]
    r = np.where((rep >= 0) & (rep <= pos), rep, pos)[idx]
    cls = (family[rows].astype(np.uint64) << np.uint64(32)) | r.astype(np.uint64)
    _, first_at, inv = np.unique(cls, return_index=True, return_inverse=True)
    first = idx[first_at[inv.reshape(-1)]] if idx.size else idx
    ln = chunk_len[idx]
    out = {name: np.zeros(n, np.uint64) for name in ROWS}
    is_first = first == idx
    own = ~is_first & (cf[first] == rows)
    np.add.at(out["file_bytes"], rows, ln)
    np.add.at(out["delta_bytes"], rows[is_first], ln[is_first])
    np.add.at(out["self_bytes"], rows[own], ln[own])
    np.add.at(out["inherited_bytes"], rows[~is_first & ~own], ln[~is_first & ~own])
    live = np.flatnonzero(row_ok)
    lab = family[live]
    total, stored = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    np.add.at(total, lab, out["file_bytes"][live])
    np.add.at(stored, lab, out["delta_bytes"][live])
    cnt = np.bincount(lab, minlength=n) if n else np.zeros(0, np.int64)
    low = np.full(n, n, np.int64)
    np.minimum.at(low, lab, live)
    sets = np.flatnonzero(cnt >= 2)
    back = total[sets] - stored[sets]
    order = np.lexsort((low[sets], ~back))
    sets, back = sets[order], back[order]
    out.update(set_rep=low[sets].astype(np.int64), set_files=cnt[sets].astype(np.uint32), set_total=total[sets],
               set_stored=stored[sets])
    with np.errstate(over="ignore"):
        out["counts"] = dict(files=int(live.size), chunks=int(idx.size), classes=int(is_first.sum()),
                             total_bytes=int(out["file_bytes"].sum(dtype=np.uint64)),
                             stored_bytes=int(out["delta_bytes"].sum(dtype=np.uint64)), sets=int(sets.size),
                             members=int(cnt[sets].sum()), set_reclaimable_bytes=int(back.sum(dtype=np.uint64)),
                             largest_reclaimable=int(back.max()) if back.size else 0)
    return out


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
        for m in args.sizes:
            n = max(m // PER_FILE, 1)
            rows = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(4)]
            set_rep, set_total, set_stored = (torch.empty(n // 2, dtype=torch.int64, device="cuda") for _ in range(3))
            set_files = torch.empty(n // 2, dtype=torch.int32, device="cuda")
            cts = torch.zeros(9, dtype=torch.int64, device="cuda")
            sh = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(5)]
            scts = torch.zeros(6, dtype=torch.int64, device="cuda")
            legs, checks, allcounts, keep = {}, {}, {}, {}
            for kind in KINDS:
                g = corpus(kind, m)
                want = reference(*g)
                d = [up(g[0], np.int32), up(g[1], np.int64), up(g[2], np.int64), up(g[3], np.int64)]
                keep[kind] = d
                legs["bytes_" + kind] = lambda d=d: eng.dev_family_bytes(
                    d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, d[3].data_ptr(), n,
                    *(t.data_ptr() for t in rows), set_rep.data_ptr(), set_files.data_ptr(), set_total.data_ptr(),
                    set_stored.data_ptr(), cts.data_ptr(), stream=s)
                legs["bytes_" + kind]()  # the warm-up, and the run that is checked
                stream.synchronize()
                got = dict(zip(COUNTS, (int(x) for x in cts.cpu().numpy().view(np.uint64))))
                k = got["sets"]
                ok = got == want["counts"] and k <= n // 2
                for name, t in zip(ROWS, rows):
                    ok = ok and np.array_equal(t.cpu().numpy().view(np.uint64), want[name])
                for name, t in zip(SETS, (set_rep, set_files, set_total, set_stored)):
                    ok = ok and np.array_equal(t[:k].cpu().numpy().view(want[name].dtype), want[name])
                checks[kind] = bool(ok)
                allcounts[kind] = want["counts"]
                if kind == "random":
                    random_rows = [want[name] for name in ROWS[1:]]
                del g, want
            d = keep["random"]
            legs["sharing"] = lambda d=d: eng.dev_chunk_sharing(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, n,
                                                                *(t.data_ptr() for t in sh), scts.data_ptr(), stream=s)
            legs["sharing"]()
            stream.synchronize()
            checks["sharing"] = all(np.array_equal(t.cpu().numpy().view(np.uint64), w)
                                    for t, w in zip(sh[:3], random_rows))
            if not all(checks.values()):
                print(json.dumps({"m": m, "checks": checks}))
                raise SystemExit(f"m = {m}: an output differs from the reference")
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
            base = us["bytes_random"]["median"]
            r = {"model": model(m), "counts": allcounts, "checks": checks, "us": us,
                 "over_random": {name: v["median"] / base for name, v in us.items() if name.startswith("bytes_")},
                 "over_sharing": {name: v["median"] / us["sharing"]["median"] for name, v in us.items()
                                  if name.startswith("bytes_")}}
            results.append(r)
            print(json.dumps({"m": m, "us": us, "over_random": r["over_random"], "over_sharing": r["over_sharing"]}),
                  flush=True)
            if args.out:  # what is measured so far, should a later size not finish
                with open(args.out, "w") as f:
                    f.write(json.dumps({"reps": args.reps, "results": results}, indent=1) + "\n")
            del legs, keep
            torch.cuda.empty_cache()
    eng.close()
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--count-only", action="store_true", help="print the byte and launch model, no device")
    ap.add_argument("--sizes", type=lambda s: tuple(1 << int(x) for x in s.split(",")), default=SIZES,
                    help="log2 of the chunk counts, comma separated (default 20,22)")
    ap.add_argument("--reps", type=int, default=REPS, help="timed repetitions of every leg (default 20)")
    ap.add_argument("--out", default=None, help="write the result as JSON here too")
    args = ap.parse_args()
    if args.count_only:
        out = {"model": [model(m) for m in args.sizes]}
    else:
        out = {"reps": args.reps, "results": run(args)}
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
