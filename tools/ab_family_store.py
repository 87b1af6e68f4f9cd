#!/usr/bin/env python3
"""Timing of the family store (sdcas_dev_family_store_layout, sdcas_dev_family_pack
and sdcas_dev_family_restore, csrc/family_store.hip) beside a device-to-device
copy of the same byte count. Legs alternating in ONE process, HIP events around
each, 20 repetitions after a warm-up, median and min. Four shapes:
  random     tools/ab_family_recipes.py's random-families corpus, 2^20 chunks of
             16 384 files, a repeated chunk given its source's length (so that
             the offsets obey the recipes' law 2) and every length divided by
             --shrink (default 4: about 8 GiB of files)
  one_op     one row, one literal op of everything (4 GiB)
  min_ops    2^20 literal ops of the chunker's default minimum length (2048
             bytes) and a copy of each, at several (source, destination)
             residues modulo 16; the slowest pair is the one reported
  one_class  one literal op of 64 KiB and 2^16 copy ops that all read it: every
             restore tile reads one hot store range
What to read off: pack and restore of every shape against `copy`, torch's
contiguous uint8 device-to-device copy (a hipMemcpyAsync) of the bytes the leg
moves; "x the copy" is the yardstick DESIGN.md sections 3.7 and 3.8 use. Before
any time is taken the store and the restored blob are compared on the device
with the tool's own gather (torch index arithmetic over the same ops).

--count-only prints the byte model without a device: bytes read plus bytes
written per call, tiles, launches. No ratio is set in advance: the numbers go
to profiles/family_store.json and DESIGN.md section 3.13. The split by kernel is
a run of its own under the profiler,
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
      python tools/ab_family_store.py --shapes random --reps 5
whose kernel_stats.csv is kept as profiles/family_store_kernel_stats.csv.

The model. Layout: 28 bytes read per op (the two chunk numbers, the length; a
copy also its source chunk's op and that op's row, offsets and length) and 8
written; five launches and one fill. Pack and restore: 36 bytes read per op and
per row 24, 32 written per op that moves; then every moved byte read once and
written once, plus up to 16 bytes of a neighbouring granule per 16-byte unit
whose source is not 16-byte aligned (served from cache: every granule is also
its neighbour's); five launches and one fill, the copy a constant 2048
workgroups."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ab_family_recipes as FR  # noqa: E402
from spacedrive_amd import _native as N  # noqa: E402
from spacedrive_amd.recipes import STORE_NONE, store_layout  # noqa: E402

SHAPES = ("random", "one_op", "min_ops", "one_class")
REPS = 20
M = 1 << 20
RESIDUES = ((0, 0), (1, 0), (0, 1), (7, 9), (15, 1))
LAUNCHES = {"layout": 5, "pack": 5, "restore": 5}


def tile_bytes():
    return int(N.load().sdcas_family_store_tile_bytes())


def plan(max_ops, n):
    ws = ctypes.c_uint64(0)
    rc = N.load().sdcas_family_store_plan(max_ops, n, ctypes.byref(ws))
    assert rc == N.SDCAS_OK, rc
    return int(ws.value)


def place(sizes, residue=0, gap=0):
    """rows one after another, each at an offset that is `residue` modulo 16 -> (row_at, bytes)"""
    step = (np.asarray(sizes, np.uint64) + np.uint64(gap + 15)) // np.uint64(16) * np.uint64(16) + np.uint64(16)
    at = np.cumsum(step, dtype=np.uint64) - step + np.uint64(residue)
    return at, int(step.sum()) + 16


def shape(kind, shrink=4, residues=(0, 0)):
    """-> (recipes dict of numpy arrays with "chunk_op", row sizes uint64[n]); the store's residue is made by one
    leading literal op of residues[1] bytes in a row of its own"""
    if kind == "random":
        cf, _, ln, rep, fam = FR.corpus("random", M)
        ln = np.maximum(ln // np.uint64(shrink), np.uint64(1))
        own = rep == np.arange(M)
        ln = np.where(own, ln, ln[rep])  # rep points at a chunk that stands for itself
        rec = FR.reference(cf, FR.running_offsets(cf, ln), ln, rep, fam)
        sizes = np.zeros(fam.size, np.uint64)
        np.add.at(sizes, cf, ln)
        return rec, sizes
    if kind == "one_op":
        big = np.uint64(4 << 30)
        rec = dict(op_chunk=[0], op_src_chunk=[0], op_row=[0], op_src_row=[0], op_dst_off=[0], op_src_off=[0],
                   op_len=[big], chunk_op=[0])
        sizes = np.array([big], np.uint64)
    elif kind == "min_ops":
        k, pad = M, int(residues[1])
        # op 0: `pad` bytes in row 0, so that every later store offset is pad modulo 16; then k literals of 2048
        # bytes in rows 1 .. k and their copies in rows k + 1 .. 2 k
        ln = np.concatenate([[pad], np.full(2 * k, 2048)]).astype(np.uint64)
        chunk = np.arange(2 * k + 1)
        src = np.concatenate([chunk[:k + 1], chunk[1:k + 1]])
        rec = dict(op_chunk=chunk, op_src_chunk=src, op_row=chunk, op_src_row=src, op_dst_off=np.zeros(2 * k + 1),
                   op_src_off=np.zeros(2 * k + 1), op_len=ln, chunk_op=chunk)
        sizes = ln
    elif kind == "one_class":
        k, span = 1 << 16, 64 << 10
        chunk = np.arange(k + 1)
        src = np.zeros(k + 1, np.int64)
        rec = dict(op_chunk=chunk, op_src_chunk=src, op_row=chunk, op_src_row=src, op_dst_off=np.zeros(k + 1),
                   op_src_off=np.zeros(k + 1), op_len=np.full(k + 1, span), chunk_op=chunk)
        sizes = np.full(k + 1, span, np.uint64)
    else:
        raise ValueError(kind)
    rec = {name: np.asarray(v, np.uint32 if name in FR.OPS32 + ("chunk_op",) else np.uint64)
           for name, v in rec.items()}
    return rec, sizes


def moved(rec, lay):
    """(pack's bytes, restore's bytes, pack's tiles, restore's tiles) for whole rows at 16-byte aligned places"""
    lit = rec["op_chunk"] == rec["op_src_chunk"]
    has = lay["op_store_off"] != np.uint64(STORE_NONE)
    ln, t = rec["op_len"].astype(np.uint64), np.uint64(tile_bytes())
    tiles = lambda at, n: int((((at % np.uint64(16)) + n + t - np.uint64(1)) // t)[n != 0].sum())  # noqa: E731
    p, r = lit & has, has
    return (int(ln[p].sum()), int(ln[r].sum()), tiles(lay["op_store_off"][p], ln[p]),
            tiles(rec["op_dst_off"][r], ln[r]))


def model(kind, shrink=4):
    rec, sizes = shape(kind, shrink)
    lay = store_layout(rec)
    k, n = rec["op_chunk"].size, sizes.size
    pb, rb, pt, rt = moved(rec, lay)
    per_op = {"layout": 28 * k + 8 * k, "pack": 36 * k + 24 * n + 32 * lay["counts"]["literal_ops"],
              "restore": 36 * k + 24 * n + 32 * k}
    return {"shape": kind, "ops": k, "n_files": n, "counts": lay["counts"], "workspace_bytes": plan(k, n),
            "tile_bytes": tile_bytes(), "launches": LAUNCHES, "fills": 1,
            "pack": {"bytes_moved": pb, "tiles": pt, "bytes_read_plus_written": 2 * pb + per_op["pack"]},
            "restore": {"bytes_moved": rb, "tiles": rt, "bytes_read_plus_written": 2 * rb + per_op["restore"]},
            "layout": {"bytes_read_plus_written": per_op["layout"]}}


def run_shape(eng, torch, stream, kind, args, residues=(0, 0)):
    s = stream.cuda_stream
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()  # noqa: E731
    rec, sizes = shape(kind, args.shrink, residues)
    want = store_layout(rec)
    k, n = rec["op_chunk"].size, sizes.size
    at, blob_bytes = place(sizes, residues[0])
    store_bytes = want["counts"]["store_bytes"]
    d32 = {name: up(rec[name], np.int32) for name in FR.OPS32 + ("chunk_op",)}
    d64 = {name: up(rec[name], np.int64) for name in FR.OPS64}
    d_ops = up(np.array([k], np.uint64), np.int64)
    d_off = torch.empty(max(k, 2), dtype=torch.int64, device="cuda")
    lcts, mcts = torch.zeros(6, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    d_at, d_ln = up(at, np.int64), up(sizes, np.int64)
    blob = torch.randint(0, 256, (blob_bytes + 16,), dtype=torch.uint8, device="cuda")
    back = torch.zeros(blob_bytes + 16, dtype=torch.uint8, device="cuda")
    store = torch.zeros(store_bytes + 32, dtype=torch.uint8, device="cuda")
    layout = lambda: eng.dev_family_store_layout(  # noqa: E731
        *(d32[x].data_ptr() for x in FR.OPS32), *(d64[x].data_ptr() for x in FR.OPS64), d32["chunk_op"].data_ptr(),
        rec["chunk_op"].size, d_ops.data_ptr(), k, d_off.data_ptr(), lcts.data_ptr(), stream=s)
    pack = lambda: eng.dev_family_pack(  # noqa: E731
        d32["op_chunk"].data_ptr(), d32["op_src_chunk"].data_ptr(), d32["op_row"].data_ptr(),
        d64["op_dst_off"].data_ptr(), d64["op_len"].data_ptr(), d_off.data_ptr(), d_ops.data_ptr(), k, d_at.data_ptr(), 0,
        d_ln.data_ptr(), n, blob.data_ptr(), blob_bytes, store.data_ptr(), store_bytes, mcts.data_ptr(), stream=s)
    restore = lambda: eng.dev_family_restore(  # noqa: E731
        d32["op_row"].data_ptr(), d64["op_dst_off"].data_ptr(), d64["op_len"].data_ptr(), d_off.data_ptr(),
        d_ops.data_ptr(), k, d_at.data_ptr(), 0, d_ln.data_ptr(), n, store.data_ptr(), store_bytes, back.data_ptr(),
        blob_bytes, mcts.data_ptr(), stream=s)
    # the warm-up, and the run that is checked
    layout()
    stream.synchronize()
    got = dict(zip([x for x, _ in N.FamilyStoreCounts._fields_], (int(x) for x in lcts.cpu().numpy().view(np.uint64))))
    ok = {"layout": got == want["counts"] and
          bool(np.array_equal(d_off[:k].cpu().numpy().view(np.uint64), want["op_store_off"]))}
    pb, rb, pt, rt = moved(rec, want)
    pack()
    stream.synchronize()
    pc = [int(x) for x in mcts.cpu().numpy().view(np.uint64)]
    restore()
    stream.synchronize()
    rc = [int(x) for x in mcts.cpu().numpy().view(np.uint64)]
    ok["pack_counts"], ok["restore_counts"] = pc[1:3] == [pb, 0], rc[1:3] == [rb, 0]
    # the tool's own gather over a sample of ops, whole ops, on the device
    rng = np.random.default_rng(1)
    lit = np.flatnonzero(rec["op_chunk"] == rec["op_src_chunk"])
    good_p = good_r = True
    for o in rng.choice(k, min(k, 64), replace=False):
        ln_o = min(int(rec["op_len"][o]), 1 << 20)  # the head of a very long op
        so, b = int(want["op_store_off"][o]), int(at[rec["op_row"][o]]) + int(rec["op_dst_off"][o])
        tail = int(rec["op_len"][o]) - ln_o
        for lo in {0, tail}:
            good_r = good_r and bool(torch.equal(back[b + lo:b + lo + ln_o], store[so + lo:so + lo + ln_o]))
            if o in lit:
                good_p = good_p and bool(torch.equal(blob[b + lo:b + lo + ln_o], store[so + lo:so + lo + ln_o]))
    lit_rows = rec["op_row"][lit]
    if kind != "random":  # literal rows come back whole: the blob's own bytes
        r = int(lit_rows[-1])
        good_r = good_r and bool(torch.equal(back[int(at[r]):int(at[r] + sizes[r])], blob[int(at[r]):int(at[r] + sizes[r])]))
    ok["pack_bytes"], ok["restore_bytes"] = good_p, good_r
    if not all(ok.values()):
        print(json.dumps({"shape": kind, "residues": residues, "checks": ok, "pack": pc, "restore": rc}))
        raise SystemExit(f"{kind}: an output differs from the tool's reference")
    src_p, dst_p = blob[:max(pb, 16)], back[:max(pb, 16)]
    src_r, dst_r = blob[:max(rb, 16)], back[:max(rb, 16)]
    legs = {"layout": layout, "pack": pack, "copy_of_pack": lambda: dst_p.copy_(src_p), "restore": restore,
            "copy_of_restore": lambda: dst_r.copy_(src_r)}
    for f in legs.values():
        f()
    stream.synchronize()
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
    r = {"shape": kind, "residues": list(residues), "ops": k, "n_files": n, "counts": want["counts"], "checks": ok,
         "pack": {"bytes_moved": pb, "tiles": pt}, "restore": {"bytes_moved": rb, "tiles": rt}, "us": us,
         "tb_per_s_moved": {"pack": pb / us["pack"]["median"] / 1e6, "restore": rb / us["restore"]["median"] / 1e6,
                            "copy_of_pack": pb / us["copy_of_pack"]["median"] / 1e6,
                            "copy_of_restore": rb / us["copy_of_restore"]["median"] / 1e6},
         "x_the_copy": {"pack": us["pack"]["median"] / us["copy_of_pack"]["median"],
                        "restore": us["restore"]["median"] / us["copy_of_restore"]["median"]}}
    del blob, back, store
    torch.cuda.empty_cache()
    return r


def run(args):
    import torch
    from spacedrive_amd import Engine
    eng = Engine()
    stream = torch.cuda.Stream()
    eng.dev_bind_stream(stream.cuda_stream)
    results = []
    with torch.cuda.stream(stream):
        for kind in args.shapes:
            pairs = RESIDUES if kind == "min_ops" else ((0, 0),)
            rs = [run_shape(eng, torch, stream, kind, args, p) for p in pairs]
            r = max(rs, key=lambda x: x["x_the_copy"]["restore"] + x["x_the_copy"]["pack"])
            if len(rs) > 1:
                r["all_residues"] = [{"residues": x["residues"], "us": x["us"], "x_the_copy": x["x_the_copy"]} for x in rs]
            results.append(r)
            print(json.dumps({"shape": kind, "residues": r["residues"], "us": r["us"], "x_the_copy": r["x_the_copy"],
                              "tb_per_s_moved": r["tb_per_s_moved"]}), flush=True)
            if args.out:  # what is measured so far, should a later shape not finish
                with open(args.out, "w") as f:
                    f.write(json.dumps({"reps": args.reps, "shrink": args.shrink, "results": results}, indent=1) + "\n")
    eng.close()
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--count-only", action="store_true", help="print the byte and launch model, no device")
    ap.add_argument("--shapes", type=lambda s: tuple(s.split(",")), default=SHAPES,
                    help="comma separated, of " + ", ".join(SHAPES))
    ap.add_argument("--shrink", type=int, default=4, help="the random corpus' chunk lengths divided by this (default 4)")
    ap.add_argument("--reps", type=int, default=REPS, help="timed repetitions of every leg (default 20)")
    ap.add_argument("--out", default=None, help="write the result as JSON here too")
    args = ap.parse_args()
    if args.count_only:
        out = {"model": [model(kind, args.shrink) for kind in args.shapes]}
    else:
        out = {"reps": args.reps, "shrink": args.shrink, "results": run(args)}
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
