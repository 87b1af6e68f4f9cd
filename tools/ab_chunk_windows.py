#!/usr/bin/env python3
"""Timing of the chunk windows (sdcas_dev_chunk_windows, csrc/cdc.hip) beside
sdcas_dev_chunk on the same bytes: one synthetic 1 GiB file built on the
device, at the default parameters. Legs alternating in ONE process, HIP events
around each, after a warm-up:
  a        sdcas_dev_chunk: one wave walks the whole file's chain (k_cdc_cut)
  b        sdcas_dev_chunk_windows, one final window: 1024 segments of 1 MiB
           (k_cdc_cut_seg, k_cdc_stitch, k_cdc_gather)
  c        the same file in windows of 256 MiB that are not final, each
           starting at the consumed of the one before (its download is the
           one wait per window)
  d_chunk / d_windows
           tools/ab_chunks.py's 100 000-file corpus through both calls; no
           file of it reaches two segments
Legs a, b and d run without keys and digests (the cut passes are what
differs; no host wait), a_hashed and b_hashed with them.

Before any time is taken every output is compared: legs a, b and c against
the tool's numpy reference of the 1 GiB file (cuts, kinds, counts, consumed)
and the oracle's CPU BLAKE3 of every chunk; leg d's two calls against each
other in every array, and the first 2 000 files against the numpy reference.

--count-only prints the byte model without a device; --legs ab (or d) restricts
the run, for a `rocprofv3 --kernel-trace --stats --output-format csv` run whose
per-kernel split --kernel-stats DIR (--kernel-stats-d DIR) then adds to the profile. Results: profiles/chunk_windows.json.

The model (B bytes, M = sdcas_chunk_plan's max_chunks, S segments of seg bytes,
L = ceil(seg / min_len) list entries): the gear pass, emit, pack and hash are
tools/ab_chunks.py's. The cut passes read the bitmap once more or less (B / 4;
a walked stretch is read twice) and write 8 L S list bytes at most, of which
the cuts made are touched; the stitch reads one list entry per walked cut."""
import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ab_chunks as A  # noqa: E402
from spacedrive_amd import _native as N  # noqa: E402

_U = np.uint64
PARAMS = N.SDCAS_CHUNK_PARAMS_DEFAULT
FILE_BYTES = 1 << 30
WINDOW_BYTES = 256 << 20
SEG_DEFAULT = 1 << 20
COUNTS = A.CHUNK_COUNTS
KEY = 0x5DC0FFEE


def seg_bytes():
    v = os.environ.get("SDCAS_CHUNK_SEG_BYTES", "")
    x = int(v) if v.isdigit() and int(v) else SEG_DEFAULT
    return (max(x, 2 * PARAMS[2]) + 63) // 64 * 64


def model(B=FILE_BYTES):
    seg = seg_bytes()
    mc = -(-B // PARAMS[0])
    slots = -(-B // 1024)
    segs = -(-B // seg) if B >= 2 * seg else 0
    max_segs = 3 * 1024 * slots // (2 * seg) + 1 if 1024 * slots >= 2 * seg else 0
    spl = -(-seg // PARAMS[0])
    # windows that are not final leave less than max_len behind each: one more window takes the tails
    windows = -(-B // WINDOW_BYTES) + (1 if B > WINDOW_BYTES else 0)
    est = B // (PARAMS[0] + (1 << PARAMS[1])) + 1
    return {"file_bytes": B, "seg_bytes": seg, "segments": segs, "max_segs": max_segs, "list_entries": spl,
            "window_bytes": WINDOW_BYTES, "windows": windows, "max_chunks": mc, "chunks_estimate": est,
            "spec_bytes": 8 * max_segs * spl, "bitmap_bytes": 256 * slots,
            "bytes_cut_passes": {"bitmap_read": 256 * slots, "lists_written": 8 * est, "lists_read": 8 * est,
                                 "ends_written": 8 * est},
            "serial_cuts": {"a": est, "b_model": "about one walked cut per segment but the first: %d" % max(segs - 1, 0)}}


# ---- the reference (numpy) -------------------------------------------------------------

def candidates(x, params, block=32 << 20, threads=16):
    """the STRICT and LOOSE positions of x, block by block (a position's hash
    needs the 31 bytes before it only)"""
    g = A.gear_table()
    bits = params[1]

    def work(lo):
        a = max(lo - 31, 0)
        gx = g[x[a:min(lo + block, x.size)]]
        h = gx.copy()
        with np.errstate(over="ignore"):
            for k in range(1, min(32, gx.size)):
                h[k:] += gx[:gx.size - k] << np.uint32(k)
        h = h[lo - a:]
        return (np.flatnonzero(h < np.uint32(1 << (31 - bits))) + lo, np.flatnonzero(h < np.uint32(1 << (33 - bits))) + lo)

    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(work, range(0, x.size, block)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def step(strict, loose, s, W, params, final):
    """-> (e, kind) with kind 0 HASH, 1 MAX, 2 END, or None where a window that is not final stops"""
    min_len, bits, max_len = params
    left = W - s
    if final and left <= min_len:
        return W, 2
    if not final and left < min_len:
        return None
    hi = min(s + max_len, W)
    a = np.searchsorted(strict, s + min_len - 1)
    e = None
    if a < strict.size and strict[a] < min(s + (1 << bits) - 1, hi):
        e = int(strict[a]) + 1
    else:
        b = np.searchsorted(loose, s + (1 << bits) - 1)
        if b < loose.size and loose[b] < hi:
            e = int(loose[b]) + 1
    if e is not None:
        return e, 2 if final and e == W else 0
    if s + max_len <= W:
        return s + max_len, 2 if final and s + max_len == W else 1
    return (W, 2) if final else None


def chain(strict, loose, s, W, params, final, limit=None):
    ends, kinds = [], []
    while s < W:
        st = step(strict, loose, s, W, params, final)
        if st is None:
            break
        ends.append(st[0]), kinds.append(st[1])
        s = st[0]
        if limit is not None and s >= limit:
            break
    return ends, kinds, s


def walk_counts(strict, loose, true_ends, W, params, seg):
    """per segment but the first: the cuts the true chain makes from its entry
    cut until it lands on a cut of the segment's own chain (the model of
    k_cdc_stitch's walk)"""
    true_ends = np.asarray(true_ends)
    walks = []
    for j in range(1, -(-W // seg)):
        at = int(np.searchsorted(true_ends, j * seg))
        if at >= true_ends.size:
            walks.append(0)
            continue
        c = int(true_ends[at])
        if c == j * seg:
            walks.append(0)
            continue
        spec = set(chain(strict, loose, j * seg, W, params, True, (j + 1) * seg)[0])
        n = 0
        for e in true_ends[at + 1:]:
            n += 1
            if int(e) in spec or e >= (j + 1) * seg:
                break
        walks.append(n)
    return walks


# ---- the device ---------------------------------------------------------------------------

def device(a, res):
    import torch
    from spacedrive_amd import Engine
    from tests._oracle import load_oracle
    oracle = load_oracle()
    dev = torch.device("cuda", 0)
    eng = Engine()
    seg = eng.chunk_seg_bytes(PARAMS)
    res["model"] = model()
    assert seg == res["model"]["seg_bytes"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    i64 = lambda k: torch.zeros(max(k, 1), dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    B = FILE_BYTES
    equal = {}
    if set("abc") & set(a.legs):  # the 1 GiB file
        blob = torch.zeros(B + 64 + 16, dtype=torch.uint8, device=dev)
        d = [t(np.array([v], _U)) for v in (KEY, 0, B, 0)]
        eng.dev_synth_content(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 1, blob.data_ptr())
        eng.dev_sync()
        mc, ms = eng.chunk_plan([B], PARAMS)
        one = np.array([B], _U)
        d_off0, d_len, d_fin1, d_fin0 = t(np.zeros(1, _U)), t(one), torch.ones(8, dtype=torch.uint8, device=dev), \
            torch.zeros(8, dtype=torch.uint8, device=dev)
        out = lambda: {"fc": i64(2), "off": i64(mc), "ln": i64(mc), "fl": torch.zeros(mc, dtype=torch.int32, device=dev),
                       "keys": i64(mc), "dig": torch.zeros(32 * mc, dtype=torch.uint8, device=dev), "cons": i64(1),
                       "cnt": i64(6)}
        oa, ob, oc = out(), out(), out()

        def leg_a(o=oa, hashed=True):
            eng.dev_chunk(blob.data_ptr(), d_off0.data_ptr(), d_len.data_ptr(), 1, mc, ms, PARAMS, o["fc"].data_ptr(),
                          o["off"].data_ptr(), o["ln"].data_ptr(), o["fl"].data_ptr(), o["keys"].data_ptr() if hashed else 0,
                          o["dig"].data_ptr() if hashed else 0, o["cnt"].data_ptr(), sp)

        def leg_b(o=ob, hashed=True):
            eng.dev_chunk_windows(blob.data_ptr(), d_off0.data_ptr(), d_len.data_ptr(), d_fin1.data_ptr(), 1, mc, ms, PARAMS,
                                  o["fc"].data_ptr(), o["off"].data_ptr(), o["ln"].data_ptr(), o["fl"].data_ptr(),
                                  o["keys"].data_ptr() if hashed else 0, o["dig"].data_ptr() if hashed else 0,
                                  o["cons"].data_ptr(), o["cnt"].data_ptr(), sp)

        wmc, wms = eng.chunk_plan([WINDOW_BYTES], PARAMS)
        d_woff, d_wlen = i64(1), i64(1)

        def leg_c(o=oc, collect=None):
            """the windows of the file; collect: a list that takes (pos, counts, consumed, chunks) per window"""
            pos = 0
            while True:
                w = min(WINDOW_BYTES, B - pos)
                final = pos + w >= B
                # a cut falls on any byte and a window's offset is 16-byte aligned by contract: the window's
                # bytes are copied to an aligned buffer, as a reader delivers them
                win[:w].copy_(blob[pos:pos + w])
                d_woff.zero_()
                d_wlen.copy_(t(np.array([w], _U)))
                eng.dev_chunk_windows(win.data_ptr(), d_woff.data_ptr(), d_wlen.data_ptr(),
                                      (d_fin1 if final else d_fin0).data_ptr(), 1, wmc, wms, PARAMS, o["fc"].data_ptr(),
                                      o["off"].data_ptr(), o["ln"].data_ptr(), o["fl"].data_ptr(), o["keys"].data_ptr(),
                                      o["dig"].data_ptr(), o["cons"].data_ptr(), o["cnt"].data_ptr(), sp)
                eng.dev_sync(sp)
                used = int(o["cons"].cpu().numpy().view(_U)[0])
                if collect is not None:
                    cnt = dict(zip(COUNTS, (int(x) for x in o["cnt"].cpu().numpy().view(_U))))
                    m = cnt["chunks"]
                    collect.append((pos, cnt, used, o["off"].cpu().numpy().view(_U)[:m].copy(),
                                    o["ln"].cpu().numpy().view(_U)[:m].copy(),
                                    o["dig"].cpu().numpy().reshape(-1, 32)[:m].copy()))
                if final:
                    return
                if used == 0:
                    raise RuntimeError("a window of 256 MiB consumed nothing")
                pos += used

        win = torch.zeros(WINDOW_BYTES + 64 + 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            leg_a()
            leg_b()
            eng.dev_sync(sp)
            windows = []
            if "c" in a.legs:
                leg_c(collect=windows)

        # ---- every output against the reference, before any time is taken
        x = blob[:B].cpu().numpy()
        strict, loose = candidates(x, PARAMS)
        w_ends, w_kinds, _ = chain(strict, loose, 0, B, PARAMS, True)
        w_ends, w_kinds = np.array(w_ends, _U), np.array(w_kinds)
        m = int(w_ends.size)
        w_off = np.r_[_U(0), w_ends[:-1]]
        w_ln = w_ends - w_off
        want_counts = dict(zip(COUNTS, (1, m, B, int((w_kinds == 0).sum()), int((w_kinds == 1).sum()),
                                        int((w_kinds == 2).sum()))))
        stepn = max(1, m // 64)
        with ThreadPoolExecutor(16) as pool:
            parts = list(pool.map(lambda lo: b"".join(bytes.fromhex(oracle.hash(x[int(w_off[c]):int(w_ends[c])]))
                                                      for c in range(lo, min(lo + stepn, m))), range(0, m, stepn)))
        w_dig = np.frombuffer(b"".join(parts), np.uint8).reshape(m, 32)
        for name, o in (("a", oa), ("b", ob)):
            cnt = dict(zip(COUNTS, (int(v) for v in o["cnt"].cpu().numpy().view(_U))))
            ok = cnt == want_counts
            if ok:
                ok = bool((o["off"].cpu().numpy().view(_U)[:m] == w_off).all() and
                          (o["ln"].cpu().numpy().view(_U)[:m] == w_ln).all() and
                          (o["fl"].cpu().numpy()[:m] == 0).all() and
                          (o["fc"].cpu().numpy().view(_U) == np.array([0, m], _U)).all() and
                          (o["dig"].cpu().numpy().reshape(-1, 32)[:m] == w_dig).all() and
                          (o["keys"].cpu().numpy().view(_U)[:m] == w_dig[:, :8].copy().view(">u8").reshape(-1)).all())
            equal[name] = ok
            res["counts_" + name] = cnt
        equal["b_consumed"] = int(ob["cons"].cpu().numpy().view(_U)[0]) == B
        if "c" in a.legs:
            c_ends = np.concatenate([_U(p) + off + ln for p, _, _, off, ln, _ in windows])
            c_dig = np.concatenate([dg for *_, dg in windows])
            c_counts = {k: sum(w[1][k] for w in windows) for k in COUNTS}
            equal["c"] = bool(c_ends.size == m and (c_ends.astype(_U) == w_ends).all() and (c_dig == w_dig).all() and
                              c_counts == want_counts)
            # each window starts at the consumed of the one before, and its consumed is where the reference's
            # chain of that window stops
            pos, ok = 0, True
            for p, _, used, *_ in windows:
                ok = ok and p == pos
                if pos + WINDOW_BYTES < B:
                    ok = ok and used == chain(strict, loose, pos, pos + WINDOW_BYTES, PARAMS, False)[2] - pos
                pos += used
            equal["c_consumed"] = bool(ok and len(windows) == res["model"]["windows"])
            res["windows"] = [{"pos": p, "consumed": u, "chunks": c["chunks"]} for p, c, u, *_ in windows]
        walks = walk_counts(strict, loose, w_ends.astype(np.int64), B, PARAMS, seg)
        res["walked_cuts_per_segment_model"] = {"segments": len(walks) + 1, "mean": float(np.mean(walks)), "max": int(max(walks)),
                                                "total": int(sum(walks)), "chunks": m}
        del x, strict, loose

    # ---- leg d: the small-file corpus through both calls
    legs = {}
    if "d" in a.legs:
        lens, keys, kind, at = A.workload(a.files)
        n = lens.size
        cblob, coffs = A.build_corpus(eng, torch, dev, lens, keys, kind, at)
        cmc, cms = eng.chunk_plan(lens, PARAMS)
        d_coffs, d_clens = t(coffs), t(lens)
        od = [{"fc": i64(n + 1), "off": i64(cmc), "ln": i64(cmc), "fl": torch.zeros(cmc, dtype=torch.int32, device=dev),
               "cons": i64(n), "cnt": i64(6)} for _ in range(2)]
        d_chunk = lambda: eng.dev_chunk(cblob.data_ptr(), d_coffs.data_ptr(), d_clens.data_ptr(), n, cmc, cms, PARAMS,
                                        od[0]["fc"].data_ptr(), od[0]["off"].data_ptr(), od[0]["ln"].data_ptr(),
                                        od[0]["fl"].data_ptr(), 0, 0, od[0]["cnt"].data_ptr(), sp)
        d_windows = lambda: eng.dev_chunk_windows(cblob.data_ptr(), d_coffs.data_ptr(), d_clens.data_ptr(), 0, n, cmc,
                                                  cms, PARAMS, od[1]["fc"].data_ptr(), od[1]["off"].data_ptr(),
                                                  od[1]["ln"].data_ptr(), od[1]["fl"].data_ptr(), 0, 0,
                                                  od[1]["cons"].data_ptr(), od[1]["cnt"].data_ptr(), sp)
        d_chunk()
        d_windows()
        eng.dev_sync(sp)
        cm = int(od[0]["cnt"].cpu().numpy().view(_U)[1])
        equal["d"] = bool(all((od[0][k].cpu().numpy()[:cm if k != "fc" else n + 1] ==
                               od[1][k].cpu().numpy()[:cm if k != "fc" else n + 1]).all() for k in ("fc", "off", "ln", "fl"))
                          and (od[0]["cnt"].cpu().numpy() == od[1]["cnt"].cpu().numpy()).all()
                          and (od[1]["cons"].cpu().numpy().view(_U) == lens).all())
        few = min(2000, n)
        end = int(coffs[few - 1] + lens[few - 1])
        r_fc, r_off, r_ln, r_fl = A.ref_chunks(cblob[:end].cpu().numpy(), coffs[:few], lens[:few], PARAMS)
        k = int(r_fc[-1])
        equal["d_first_files_reference"] = bool((od[1]["fc"].cpu().numpy().view(_U)[:few + 1] == r_fc).all() and
                                                (od[1]["off"].cpu().numpy().view(_U)[:k] == r_off).all() and
                                                (od[1]["ln"].cpu().numpy().view(_U)[:k] == r_ln).all())
        res["corpus"] = {"files": int(n), "content_bytes": int(lens.sum()), "chunks": cm}
        legs.update({"d_chunk": d_chunk, "d_windows": d_windows})
    res["outputs_equal_reference"] = equal
    if not all(equal.values()):
        res["device"] = "outputs differ from the reference: no time is reported"
        eng.close()
        return
    if "a" in a.legs:
        legs.update({"a": lambda: leg_a(hashed=False), "a_hashed": leg_a})
    if "b" in a.legs:
        legs.update({"b": lambda: leg_b(hashed=False), "b_hashed": leg_b})
    if "c" in a.legs:
        legs["c"] = leg_c
    msr = {k: [] for k in legs}
    with torch.cuda.stream(stream):
        for f in legs.values():
            f()
            eng.dev_sync(sp)
        for _ in range(a.reps):
            for k, f in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                eng.dev_sync(sp)
                msr[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in msr.items()}
    dev_res = {"reps": a.reps, "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in msr.items()},
               "max_ms": {k: float(np.max(v)) for k, v in msr.items()}}
    if "a" in med and "b" in med:
        dev_res["a_over_b"] = med["a"] / med["b"]
        dev_res["file_GBps"] = {k: B / med[k] / 1e6 for k in med if k[0] in "abc"}
    if "d_chunk" in med:
        dev_res["d_windows_over_d_chunk"] = med["d_windows"] / med["d_chunk"]
    res["device"] = dev_res
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=100_000, help="leg d's corpus")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--count-only", action="store_true", help="the model alone: no device")
    ap.add_argument("--kernel-stats", help="a rocprofv3 --kernel-trace --stats output directory of a --legs ab run")
    ap.add_argument("--kernel-stats-d", help="the same of a --legs d run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_windows.json"))
    a = ap.parse_args()
    res = {"tool": "tools/ab_chunk_windows.py", "params": list(PARAMS), "legs": a.legs}
    if a.count_only:
        res["model"] = model()
        print(json.dumps(res))
        return
    if a.kernel_stats_d:
        with open(a.out) as f:
            res = json.load(f)
        # per leg: the check's call, one warm-up and the timed repetitions
        res["kernel_trace_d"] = {"legs": "d", "calls_per_leg": a.reps + 2,
                                 "kernels": A.kernel_stats(a.kernel_stats_d, a.reps + 2)}
    elif a.kernel_stats:
        with open(a.out) as f:
            res = json.load(f)
        # per leg: the check's call, one warm-up and the timed repetitions, plain and hashed
        calls = 2 * (a.reps + 1) + 1
        k = A.kernel_stats(a.kernel_stats, calls)
        res["kernel_trace"] = {"legs": "ab", "calls_per_leg": calls, "kernels": k}
        cut = k.get("k_cdc_cut", {}).get("ms_per_call")
        new = [k.get(n, {}).get("ms_per_call") for n in ("k_cdc_cut_seg", "k_cdc_stitch", "k_cdc_gather")]
        if cut and all(v is not None for v in new):
            res["kernel_trace"]["cut_passes_ms"] = {"a_k_cdc_cut": cut, "b_cut_seg_stitch_gather": sum(new),
                                                    "a_over_b": cut / sum(new)}
    else:
        device(a, res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
