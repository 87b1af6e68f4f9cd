#!/usr/bin/env python3
"""Timing of a family store that forgets rows (sdcas_dev_family_chunks_keep and
sdcas_dev_family_store_moves, csrc/family_forget.hip, and the moves carried by
sdcas_dev_family_restore) beside what it replaces. Legs alternating in ONE
process, HIP events around each, 10 repetitions after a warm-up, median and min.
The corpus is tools/ab_family_store.py's random shape: 2^20 chunks of 16 384
files in families of 1 to 16 rows, every length divided by --shrink (default 4:
about 8 GiB of files). Three removals, in turn:
  tenth         a tenth of the rows at random
  firsts        the first version of every family (a family of one row goes whole)
  every_second  every second row
The legs:
  keep      sdcas_dev_family_chunks_keep over the old chunk arrays
  plan      sdcas_dev_family_recipes and sdcas_dev_family_store_layout over what
            keep leaves (code that was there before; removal and rebuild both run it)
  moves     sdcas_dev_family_store_moves
  carry     sdcas_dev_family_restore with the moves as its ops: old store to new
  copy      torch's contiguous uint8 device-to-device copy of the new store's bytes
  rebuild   what removal replaces when the originals are still at hand and already
            in HBM: sdcas_dev_family_recipes, sdcas_dev_family_store_layout and
            sdcas_dev_family_pack over the survivors' contents. Reading the files
            again, which is the real cost, is not in it.
What to read off: carry against copy ("x the copy", the yardstick of DESIGN.md
sections 3.7, 3.8 and 3.13), and keep + plan + moves + carry against rebuild.
Before any time is taken every output of keep and moves is compared with the
numpy forms in spacedrive_amd/recipes.py, and the new store with a gather of the
tool's own over the moves.

--count-only prints the byte and launch model without a device. No ratio is set
in advance: the numbers go to profiles/family_forget.json and DESIGN.md section
3.14.

The model. keep: per row 9 bytes read (label, flag) and 16 written; per chunk 28
read (file, offset, length, rep) and 28 written per survivor; nine launches and
two fills. moves: per new chunk 24 bytes read of its own arrays, about 40 through
chunk_from and the two ops, twice (the chunk below is computed again), 9 written;
per move 24 written; five launches and one fill. carry: the mover's model with
one op per move."""
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
from spacedrive_amd.recipes import keep_chunks, store_layout, store_moves  # noqa: E402

REMOVALS = ("tenth", "firsts", "every_second")
REPS = 10
M = 1 << 20
LAUNCHES = {"keep": 9, "recipes": 7, "layout": 5, "moves": 5, "carry": 5}
KEEP_OUT = ("row_new", "row_from", "family", "chunk_from", "chunk_file", "chunk_off", "chunk_len", "rep")


def plan(m, n):
    ws = ctypes.c_uint64(0)
    rc = N.load().sdcas_family_forget_plan(m, n, ctypes.byref(ws))
    assert rc == N.SDCAS_OK, rc
    return int(ws.value)


def corpus(m=M, shrink=4):
    """ab_family_store.py's random shape as chunk arrays -> chunk_file, chunk_off, chunk_len, rep, family"""
    cf, _, ln, rep, fam = FR.corpus("random", m)
    ln = np.maximum(ln // np.uint64(shrink), np.uint64(1))
    ln = np.where(rep == np.arange(m), ln, ln[rep])  # a repeated chunk has its source's length
    return cf, FR.running_offsets(cf, ln), ln, rep, fam


def mask(removal, family, seed=0):
    n = family.size
    if removal == "tenth":
        return (np.random.default_rng(seed).random(n) >= 0.1).astype(np.uint8)
    if removal == "firsts":
        return (family != np.arange(n)).astype(np.uint8)
    if removal == "every_second":
        return (np.arange(n) % 2 == 0).astype(np.uint8)
    raise ValueError(removal)


def recipes_of(cf, off, ln, rep, fam):
    rec = FR.reference(cf, off, ln, rep, fam)
    rec["chunk_off"] = off
    return rec, store_layout(rec)


def chain(arrays, old, removal):
    """the removal on the host -> (keep mask, keep_chunks' dict, new recipes, new layout, store_moves' dict)"""
    cf, off, ln, rep, fam = arrays
    keep = mask(removal, fam)
    kept = keep_chunks(cf, off, ln, rep, fam, keep)
    rec2, lay2 = recipes_of(kept["chunk_file"], kept["chunk_off"], kept["chunk_len"], kept["rep"], kept["family"])
    mv = store_moves(old[0], old[1], rec2, lay2, kept["chunk_from"], kept["chunk_len"])
    return keep, kept, rec2, lay2, mv


def model(removal, m=M, shrink=4, arrays=None, old=None):
    arrays = corpus(m, shrink) if arrays is None else arrays
    old = recipes_of(*arrays) if old is None else old
    _, kept, rec2, lay2, mv = chain(arrays, old, removal)
    n, m2, n2 = arrays[4].size, kept["counts"]["chunks_kept"], kept["counts"]["rows_kept"]
    size2, moves = lay2["counts"]["store_bytes"], mv["counts"]["moves"]
    return {"removal": removal, "rows": n, "chunks": m, "rows_removed": n - n2, "chunks_kept": m2,
            "bytes_kept": kept["counts"]["bytes_kept"], "old_store_bytes": old[1]["counts"]["store_bytes"],
            "new_store_bytes": size2, "new_ops": rec2["counts"]["ops"], "moves": moves,
            "moved_bytes": mv["counts"]["moved_bytes"], "lost_chunks": mv["counts"]["lost_chunks"],
            "longest_move": mv["counts"]["longest_move"], "workspace_bytes": plan(m, n), "launches": LAUNCHES,
            "fills": {"keep": 2, "moves": 1, "carry": 1},
            "bytes_read_plus_written": {"keep": 9 * n + 16 * n2 + 28 * m + 28 * m2,
                                        "moves": 2 * 64 * m2 + 9 * m2 + 24 * moves,
                                        "carry": 2 * size2 + 36 * moves + 32 * moves}}


def run_removal(eng, torch, stream, arrays, old, removal, args):
    s = stream.cuda_stream
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda() if np.asarray(a).size else \
        torch.zeros(16, dtype=torch.uint8, device="cuda")  # noqa: E731
    room = lambda k, dt: torch.zeros(max(int(k), 2), dtype=dt, device="cuda")  # noqa: E731
    i32, i64 = torch.int32, torch.int64
    cf, off, ln, rep, fam = arrays
    rec, lay = old
    keep, kept, rec2, lay2, mv = chain(arrays, old, removal)
    m, n, k = cf.size, fam.size, rec["op_chunk"].size
    m2, n2, k2 = kept["counts"]["chunks_kept"], kept["counts"]["rows_kept"], rec2["op_chunk"].size
    size1, size2, moves = lay["counts"]["store_bytes"], lay2["counts"]["store_bytes"], mv["counts"]["moves"]
    # the old side
    o_file, o_off, o_len, o_rep, o_fam, o_keep = (up(a, dt) for a, dt in (
        (cf, np.int32), (off, np.int64), (ln, np.int64), (rep, np.int64), (fam, np.int64), (keep, np.uint8)))
    o_chunk_op, o_dst, o_so = up(rec["chunk_op"], np.int32), up(rec["op_dst_off"], np.int64), \
        up(lay["op_store_off"], np.int64)
    o_ops = up(np.array([k], np.uint64), np.int64)
    store1 = torch.randint(0, 256, (size1 + 32,), dtype=torch.uint8, device="cuda")
    store2 = torch.zeros(size2 + 32, dtype=torch.uint8, device="cuda")
    # keep's outputs, the new recipes and layout, the moves
    k_out = {"row_new": room(n, i32), "row_from": room(n, i32), "family": room(n, i64), "chunk_from": room(m, i32),
             "chunk_file": room(m, i32), "chunk_off": room(m, i64), "chunk_len": room(m, i64), "rep": room(m, i64)}
    kc, rc, lc, mc, cc = room(6, i64), room(8, i64), room(6, i64), room(6, i64), room(4, i64)
    op32, op64 = [room(m2, i32) for _ in range(4)], [room(m2, i64) for _ in range(3)]
    chunk_op2, row_ops2, row_first2, so2 = room(m2, i32), room(n2, i32), room(n2, i32), room(m2, i64)
    mv_dst, mv_src, mv_len, zeros = room(m2, i64), room(m2, i64), room(m2, i64), room(m2, i32)
    w_at, w_len = up(np.zeros(1, np.uint64), np.int64), up(np.array([size2], np.uint64), np.int64)

    def leg_keep():
        eng.dev_family_chunks_keep(o_file.data_ptr(), o_off.data_ptr(), o_len.data_ptr(), o_rep.data_ptr(), m,
                                   o_fam.data_ptr(), o_keep.data_ptr(), n, *(k_out[x].data_ptr() for x in KEEP_OUT),
                                   kc.data_ptr(), stream=s)

    def plan_over(c_file, c_off, c_len, c_rep, c_fam):
        eng.dev_family_recipes(c_file.data_ptr(), c_off.data_ptr(), c_len.data_ptr(), c_rep.data_ptr(), m2,
                               c_fam.data_ptr(), n2, *(t.data_ptr() for t in op32 + op64), chunk_op2.data_ptr(),
                               row_ops2.data_ptr(), row_first2.data_ptr(), rc.data_ptr(), stream=s)
        eng.dev_family_store_layout(*(t.data_ptr() for t in op32 + op64), chunk_op2.data_ptr(), m2,
                                    rc.data_ptr() + 16, m2, so2.data_ptr(), lc.data_ptr(), stream=s)

    def leg_plan():
        plan_over(k_out["chunk_file"], k_out["chunk_off"], k_out["chunk_len"], k_out["rep"], k_out["family"])

    def leg_moves():
        eng.dev_family_store_moves(o_off.data_ptr(), o_chunk_op.data_ptr(), m, o_dst.data_ptr(), o_so.data_ptr(),
                                   o_ops.data_ptr(), k, k_out["chunk_from"].data_ptr(), k_out["chunk_off"].data_ptr(),
                                   k_out["chunk_len"].data_ptr(), chunk_op2.data_ptr(), kc.data_ptr() + 16, m2,
                                   op32[0].data_ptr(), op32[1].data_ptr(), op64[0].data_ptr(), so2.data_ptr(),
                                   rc.data_ptr() + 16, m2, mv_dst.data_ptr(), mv_src.data_ptr(), mv_len.data_ptr(),
                                   mc.data_ptr(), stream=s)

    def leg_carry():
        eng.dev_family_restore(zeros.data_ptr(), mv_dst.data_ptr(), mv_len.data_ptr(), mv_src.data_ptr(),
                               mc.data_ptr(), m2, w_at.data_ptr(), 0, w_len.data_ptr(), 1, store1.data_ptr(), size1,
                               store2.data_ptr(), size2, cc.data_ptr(), stream=s)

    # the warm-up, and the run that is checked
    leg_keep(), leg_plan(), leg_moves(), leg_carry()
    stream.synchronize()
    down = lambda t, cnt, dt: t[:int(cnt)].cpu().numpy().view(dt)  # noqa: E731
    dts = {"row_new": np.uint32, "row_from": np.uint32, "family": np.int64, "chunk_from": np.uint32,
           "chunk_file": np.uint32, "chunk_off": np.uint64, "chunk_len": np.uint64, "rep": np.int64}
    cnt = {"row_new": n, "row_from": n2, "family": n2}
    ok = {"keep": all(np.array_equal(down(k_out[x], cnt.get(x, m2), dts[x]), kept[x]) for x in KEEP_OUT) and
          [int(x) for x in down(kc, 6, np.uint64)] == list(kept["counts"].values()),
          "plan": bool(np.array_equal(down(so2, k2, np.uint64), lay2["op_store_off"])) and
          int(down(lc, 6, np.uint64)[4]) == size2,
          "moves": all(np.array_equal(down(t, moves, np.uint64), mv[x]) for t, x in
                       ((mv_dst, "move_dst"), (mv_src, "move_src"), (mv_len, "move_len"))) and
          [int(x) for x in down(mc, 6, np.uint64)] == list(mv["counts"].values()),
          "carry_counts": [int(x) for x in down(cc, 4, np.uint64)][:3] == [moves if size2 else 0, size2, 0]}
    # the tool's own gather over a sample of moves, whole moves, and nothing lost
    rng = np.random.default_rng(1)
    good = mv["counts"]["lost_chunks"] == 0
    for j in rng.choice(moves, min(moves, 256), replace=False) if moves else ():
        d, a, b = int(mv["move_dst"][j]), int(mv["move_src"][j]), int(mv["move_len"][j])
        good = good and bool(torch.equal(store2[d:d + b], store1[a:a + b]))
    ok["carry_bytes"] = good
    if not all(ok.values()):
        print(json.dumps({"removal": removal, "checks": ok}))
        raise SystemExit(f"{removal}: an output differs from the tool's reference")
    # what removal replaces: the survivors' contents in HBM, their recipes, layout and pack
    sizes2 = np.zeros(n2, np.uint64)
    np.add.at(sizes2, kept["chunk_file"].astype(np.int64), kept["chunk_len"])
    step = (sizes2 + np.uint64(15)) // np.uint64(16) * np.uint64(16) + np.uint64(16)
    at = np.cumsum(step, dtype=np.uint64) - step
    blob_bytes = int(step.sum()) + 16
    blob = torch.randint(0, 256, (blob_bytes + 16,), dtype=torch.uint8, device="cuda")
    s_file, s_off, s_len, s_rep, s_fam = (up(kept[x], dt) for x, dt in (
        ("chunk_file", np.int32), ("chunk_off", np.int64), ("chunk_len", np.int64), ("rep", np.int64),
        ("family", np.int64)))
    d_at, d_ln = up(at, np.int64), up(sizes2, np.int64)
    packed = torch.zeros(size2 + 32, dtype=torch.uint8, device="cuda")
    pc = room(4, i64)

    def leg_rebuild():
        plan_over(s_file, s_off, s_len, s_rep, s_fam)
        eng.dev_family_pack(op32[0].data_ptr(), op32[1].data_ptr(), op32[2].data_ptr(), op64[0].data_ptr(),
                            op64[2].data_ptr(), so2.data_ptr(), rc.data_ptr() + 16, m2, d_at.data_ptr(), 0,
                            d_ln.data_ptr(), n2, blob.data_ptr(), blob_bytes, packed.data_ptr(), size2, pc.data_ptr(),
                            stream=s)

    src_c, dst_c = store1[:max(size2, 16)], packed[:max(size2, 16)]
    legs = {"keep": leg_keep, "plan": leg_plan, "moves": leg_moves, "carry": leg_carry,
            "copy": lambda: dst_c.copy_(src_c), "rebuild": leg_rebuild}
    for f in legs.values():
        f()
    stream.synchronize()
    if [int(x) for x in down(pc, 4, np.uint64)][1:3] != [size2, 0]:
        raise SystemExit(f"{removal}: the rebuild packed other bytes than the new store's")
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
    med = {name: v["median"] for name, v in us.items()}
    removal_us = med["keep"] + med["plan"] + med["moves"] + med["carry"]
    r = {"removal": removal, "rows": n, "chunks": m, "rows_removed": n - n2, "chunks_kept": m2,
         "old_store_bytes": size1, "new_store_bytes": size2, "new_ops": k2, "moves": moves,
         "longest_move": mv["counts"]["longest_move"], "checks": ok, "us": us,
         "removal_us": removal_us, "tb_per_s_moved": {"carry": size2 / med["carry"] / 1e6,
                                                      "copy": size2 / med["copy"] / 1e6},
         "x_the_copy": {"carry": med["carry"] / med["copy"]}, "x_the_rebuild": removal_us / med["rebuild"]}
    del blob, packed, store1, store2
    torch.cuda.empty_cache()
    return r


def run(args):
    import torch
    from spacedrive_amd import Engine
    eng = Engine()
    stream = torch.cuda.Stream()
    eng.dev_bind_stream(stream.cuda_stream)
    arrays = corpus(args.chunks, args.shrink)
    old = recipes_of(*arrays)
    results = []
    with torch.cuda.stream(stream):
        for removal in args.removals:
            r = run_removal(eng, torch, stream, arrays, old, removal, args)
            results.append(r)
            print(json.dumps({k: r[k] for k in ("removal", "us", "removal_us", "x_the_copy", "x_the_rebuild",
                                                "tb_per_s_moved")}), flush=True)
            if args.out:  # what is measured so far, should a later removal not finish
                with open(args.out, "w") as f:
                    f.write(json.dumps({"reps": args.reps, "shrink": args.shrink, "results": results}, indent=1) + "\n")
    eng.close()
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--count-only", action="store_true", help="print the byte and launch model, no device")
    ap.add_argument("--removals", type=lambda s: tuple(s.split(",")), default=REMOVALS,
                    help="comma separated, of " + ", ".join(REMOVALS))
    ap.add_argument("--chunks", type=int, default=M, help="the corpus' chunks (default 2^20), 64 to a file")
    ap.add_argument("--shrink", type=int, default=4, help="the corpus' chunk lengths divided by this (default 4)")
    ap.add_argument("--reps", type=int, default=REPS, help="timed repetitions of every leg (default 10)")
    ap.add_argument("--out", default=None, help="write the result as JSON here too")
    args = ap.parse_args()
    if args.count_only:
        arrays = corpus(args.chunks, args.shrink)
        old = recipes_of(*arrays)
        out = {"model": [model(r, args.chunks, args.shrink, arrays, old) for r in args.removals]}
    else:
        out = {"reps": args.reps, "shrink": args.shrink, "results": run(args)}
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
