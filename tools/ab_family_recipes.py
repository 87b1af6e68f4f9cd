#!/usr/bin/env python3
"""Timing of the family recipes (sdcas_dev_family_recipes,
csrc/family_recipes.hip) beside the family bytes over the same arrays. m = 2^20
and 2^22 chunks, n_files = m / 64, 64 adjacent chunks per file but in the
one-run leg. Legs alternating in ONE process, HIP events around each, 20
repetitions after a warm-up, median and min:
  recipes_random     tools/ab_family_bytes.py's random corpus (families of 1 to
                     16 consecutive rows, about half of the chunks repeat an
                     earlier chunk of their family) with the per-file running
                     offsets
  recipes_one_run    one file holds every chunk, all classes distinct: one
                     literal op of m chunks, whose length crosses every wave and
                     workgroup
  recipes_no_runs    every odd chunk repeats the chunk before it: literal and
                     copy alternate, m ops, every thread writes one
  recipes_one_class  every chunk is one class in one family: every insert aims
                     at one table word, and every chunk but the first is a copy
                     op of its own
  bytes              sdcas_dev_family_bytes over recipes_random's arrays: the
                     yardstick, the call whose saving the recipes spell out
What to read off: every recipes leg against recipes_random and against bytes.
Before any time is taken every output of the four recipes legs is compared with
the tool's own numpy reference, and bytes' delta_bytes with the literal bytes
per row of recipes_random (law 1).

--count-only prints the byte and launch model without a device. No ratio is set
in advance: the numbers go to profiles/family_recipes.json and DESIGN.md §3.12.
The split by kernel is a run of its own under the profiler,
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
      python tools/ab_family_recipes.py --sizes 20 --reps 5
whose kernel_stats.csv is kept as profiles/family_recipes_kernel_stats.csv.

The model. A table of 2 m u32 slots (the power of two at or above), 17 bytes
per chunk (slot, source, head flag, the op's start), a count per 256 chunks,
8 bytes per row and 8 KiB of counters; two fills and seven launches whatever the data: the insert,
the source, the one-workgroup scan, the emit and the close over m, the rows
over n_files, the totals."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ab_family_bytes as FB  # noqa: E402
from spacedrive_amd import _native as N  # noqa: E402

SIZES = (1 << 20, 1 << 22)
PER_FILE = FB.PER_FILE
REPS = 20
COUNTS = [name for name, _ in N.FamilyRecipesCounts._fields_]
OPS32 = ("op_chunk", "op_src_chunk", "op_row", "op_src_row")
OPS64 = ("op_dst_off", "op_src_off", "op_len")
REST = ("chunk_op", "row_ops", "row_first_op")
KINDS = ("random", "one_run", "no_runs", "one_class")
NONE = 0xFFFFFFFF


def plan(m, n):
    ws = ctypes.c_uint64(0)
    rc = N.load().sdcas_family_recipes_plan(m, n, ctypes.byref(ws))
    assert rc == N.SDCAS_OK, rc
    return int(ws.value)


def model(m):
    n = m // PER_FILE
    return {"m": m, "n_files": n, "workspace_bytes": plan(m, n), "table_slots": FB.table_slots(m),
            "workspace_bytes_per_chunk": 17, "workspace_bytes_per_row": 8, "scan_counts": (m + 255) // 256,
            "scan_passes": ((m + 255) // 256 + 1023) // 1024, "fills": 2, "launches": 7,
            "bytes_in": m * (4 + 8 + 8 + 8) + n * 8, "bytes_out_most": m * (4 * 4 + 3 * 8 + 4) + n * 8 + 64,
            "bytes_bytes_in": m * (4 + 8 + 8) + n * 8}


def running_offsets(chunk_file, chunk_len):
    """the per-file running sums of chunk_len for chunk_file ascending (adjacent chunks per file)"""
    before = np.cumsum(chunk_len, dtype=np.uint64) - chunk_len
    start = np.flatnonzero(np.concatenate([np.ones(min(chunk_file.size, 1), bool), chunk_file[1:] != chunk_file[:-1]]))
    return before - np.repeat(before[start], np.diff(np.concatenate([start, [chunk_file.size]])))


def corpus(kind, m, seed=0):
    """-> chunk_file u32[m], chunk_off u64[m], chunk_len u64[m], rep i64[m], family i64[n]"""
    pos = np.arange(m, dtype=np.int64)
    if kind == "one_run":
        cf, ln, rep, fam = FB.corpus("one_file", m, seed)
    elif kind == "no_runs":
        cf, ln, _, _ = FB.corpus("one_class", m, seed)
        rep, fam = pos - (pos & 1), np.zeros(max(m // PER_FILE, 1), np.int64)
    else:
        cf, ln, rep, fam = FB.corpus(kind, m, seed)
    return cf, running_offsets(cf, ln), ln, rep.astype(np.int64), fam


def reference(chunk_file, chunk_off, chunk_len, rep, family):
    """numpy, exact modulo 2^64 -> dict with the seven op arrays, chunk_op, the two per-row arrays and "counts\""""
    m, n = chunk_file.size, family.size
    pos = np.arange(m, dtype=np.int64)
    row_ok = (family >= 0) & (family < n)
    cf = chunk_file.astype(np.int64)
    on = (cf < n) & (row_ok[np.minimum(cf, n - 1)] if n else np.zeros(m, bool))
    idx = pos[on]
    r = np.where((rep >= 0) & (rep <= pos), rep, pos)[idx]
    cls = (family[cf[idx]].astype(np.uint64) << np.uint64(32)) | r.astype(np.uint64)
    _, first_at, inv = np.unique(cls, return_index=True, return_inverse=True)
    first = np.zeros(m, np.int64)  # f(c); 0 where the chunk takes no part (never used there)
    first[idx] = idx[first_at[inv.reshape(-1)]] if idx.size else idx
    lit = first == pos
    with np.errstate(over="ignore"):
        cont = np.zeros(m, bool)
        if m > 1:
            a, b = slice(0, m - 1), slice(1, m)  # c - 1 and c
            cont[b] = (on[a] & on[b] & (cf[a] == cf[b]) & (lit[a] == lit[b]) &
                       (chunk_off[b] == chunk_off[a] + chunk_len[a]) & (cf[first[a]] == cf[first[b]]) &
                       (chunk_off[first[b]] == chunk_off[first[a]] + chunk_len[a]))
        head = on & ~cont
        op_of = np.cumsum(head) - 1
        heads = np.flatnonzero(head)
        k = heads.size
        op_len = np.zeros(k, np.uint64)
        np.add.at(op_len, op_of[on], chunk_len[on])
        out = dict(op_chunk=heads.astype(np.uint32), op_src_chunk=first[heads].astype(np.uint32),
                   op_row=cf[heads].astype(np.uint32), op_src_row=cf[first[heads]].astype(np.uint32),
                   op_dst_off=chunk_off[heads], op_src_off=chunk_off[first[heads]], op_len=op_len,
                   chunk_op=np.where(on, op_of, NONE).astype(np.uint32),
                   row_ops=np.bincount(cf[heads], minlength=n).astype(np.uint32) if n else np.zeros(0, np.uint32))
        row_first = np.full(n, NONE, np.int64)
        np.minimum.at(row_first, cf[heads], np.arange(k))
        out["row_first_op"] = row_first.astype(np.uint32)
        is_lit = lit[heads]
        out["counts"] = dict(files=int(row_ok.sum()), chunks=int(idx.size), ops=int(k), literal_ops=int(is_lit.sum()),
                             copy_ops=int(k - is_lit.sum()), literal_bytes=int(op_len[is_lit].sum(dtype=np.uint64)),
                             copy_bytes=int(op_len[~is_lit].sum(dtype=np.uint64)),
                             longest_op=int(op_len.max()) if k else 0)
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
            o32 = [torch.empty(m, dtype=torch.int32, device="cuda") for _ in range(4)]
            o64 = [torch.empty(m, dtype=torch.int64, device="cuda") for _ in range(3)]
            rest = [torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
                    torch.empty(n, dtype=torch.int32, device="cuda")]
            cts = torch.zeros(8, dtype=torch.int64, device="cuda")
            rows = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(4)]
            bcts = torch.zeros(9, dtype=torch.int64, device="cuda")
            legs, checks, allcounts, keep = {}, {}, {}, {}
            for kind in KINDS:
                g = corpus(kind, m)
                want = reference(*g)
                d = [up(g[0], np.int32)] + [up(a, np.int64) for a in g[1:]]
                keep[kind] = d
                legs["recipes_" + kind] = lambda d=d: eng.dev_family_recipes(
                    d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), m, d[4].data_ptr(), n,
                    *(t.data_ptr() for t in o32 + o64 + rest), cts.data_ptr(), stream=s)
                legs["recipes_" + kind]()  # the warm-up, and the run that is checked
                stream.synchronize()
                got = dict(zip(COUNTS, (int(x) for x in cts.cpu().numpy().view(np.uint64))))
                k = got["ops"]
                ok = got == want["counts"] and k <= m
                for name, t in zip(OPS32 + OPS64, o32 + o64):
                    ok = ok and np.array_equal(t[:k].cpu().numpy().view(want[name].dtype), want[name])
                for name, t in zip(REST, rest):
                    ok = ok and np.array_equal(t.cpu().numpy().view(np.uint32), want[name])
                checks[kind] = bool(ok)
                allcounts[kind] = want["counts"]
                if kind == "random":
                    lit = want["op_chunk"] == want["op_src_chunk"]
                    random_delta = np.zeros(n, np.uint64)
                    np.add.at(random_delta, want["op_row"][lit], want["op_len"][lit])
                del g, want
            d = keep["random"]
            legs["bytes"] = lambda d=d: eng.dev_family_bytes(d[0].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), m,
                                                             d[4].data_ptr(), n, *(t.data_ptr() for t in rows),
                                                             counts=bcts.data_ptr(), stream=s)
            legs["bytes"]()
            stream.synchronize()
            checks["bytes"] = bool(np.array_equal(rows[1].cpu().numpy().view(np.uint64), random_delta))
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
            base = us["recipes_random"]["median"]
            r = {"model": model(m), "counts": allcounts, "checks": checks, "us": us,
                 "over_random": {name: v["median"] / base for name, v in us.items() if name.startswith("recipes_")},
                 "over_bytes": {name: v["median"] / us["bytes"]["median"] for name, v in us.items()
                                if name.startswith("recipes_")}}
            results.append(r)
            print(json.dumps({"m": m, "us": us, "over_random": r["over_random"], "over_bytes": r["over_bytes"]}),
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
