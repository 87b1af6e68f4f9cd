#!/usr/bin/env python3
"""Timing of the content-defined chunking (sdcas_dev_chunk, csrc/cdc.hip), the
group-by over its chunks and the sharing pass, beside the whole-file hash of
the same bytes as the yardstick (one read of every byte plus BLAKE3): four
legs alternating in ONE process, HIP events around each, 20 repetitions after
a warm-up.
  chunk     sdcas_dev_chunk with keys and digests (its one host wait included)
  hash      sdcas_dev_hash_messages over the same files as whole messages
  confirm   sdcas_dev_confirm_duplicates over the chunks
  sharing   sdcas_dev_chunk_sharing

Workload, built on the device: a C2-shaped share (sizes of sds_c2_size, 1 to
100 KiB) at the default parameters; every fourth file is its predecessor with
one byte inserted or one 4 KiB block overwritten, at a seeded place.

Before any time is reported every output of the three calls is compared with
the tool's own reference: numpy for the window hash, the cut loop and the
sharing sums, the oracle's CPU BLAKE3 for the digests.

No threshold: the numbers are recorded (--out, default
profiles/chunk_sharing.json). --count-only prints the byte model without a
device; --kernel-stats DIR adds the per-kernel split of a separate
`rocprofv3 --kernel-trace --stats` run of this tool to the profile.

The model (the least HBM traffic of the scheme; B content bytes, n files,
m chunks, M = sdcas_chunk_plan's max_chunks):
  gear     B read; 2 bits per position written (B / 4, rounded up to 256 B per
           1 KiB slot of a file)
  cut      the bitmap read once (B / 4); 8 M written (ends)
  emit     8 M read; 44 m written (the four arrays and the pack's two copies)
  wait     48 + 8 M down, 8 m up (PCIe, not HBM: listed, not summed)
  pack     B read, B + padding written
  hash     B + padding read; 40 m written
  confirm / sharing: per chunk 40 read + 16 table bytes twice + 8 written;
           24 read + 16 table bytes per chunk, 16 per table slot twice"""
import argparse
import csv
import glob
import json
import os
import re
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spacedrive_amd import _native as N  # noqa: E402
from spacedrive_amd import synth as S  # noqa: E402

_U = np.uint64
HBM_PEAK_GBPS = 8000.0
PARAMS = N.SDCAS_CHUNK_PARAMS_DEFAULT
CHUNK_COUNTS = ("files", "chunks", "total_bytes", "hash_cuts", "max_cuts", "end_chunks")
SHARE_COUNTS = ("files", "chunks", "distinct_chunks", "total_bytes", "stored_bytes", "files_with_peer")
SEED = 0x5DCDC


def workload(n):
    """(lens, keys, kind, at): kind 0 a file of its own, 1 its predecessor
    with one byte inserted at `at`, 2 with the 4 KiB block at `at` overwritten"""
    lens, keys = S.c2_files(0, n)
    r = S.mix64(_U(SEED) + np.arange(n, dtype=_U))
    kind = np.zeros(n, np.int64)
    at = np.zeros(n, np.int64)
    lens = lens.astype(np.int64)
    for i in range(3, n, 4):
        lens[i] = lens[i - 1]
        kind[i] = 1 + int(r[i] & _U(1))
        if kind[i] == 1:
            at[i] = int(r[i] >> _U(8)) % (lens[i] + 1)
            lens[i] += 1
        else:
            at[i] = int(r[i] >> _U(8)) % max(1, lens[i] - 4096)
    return lens.astype(_U), keys, kind, at


def model(lens, m, max_chunks):
    B = int(lens.sum())
    slots = int(((lens + _U(1023)) // _U(1024)).sum())
    pad = 8 * m  # 16-byte alignment: 8 bytes a chunk on average
    cap = 16
    while cap < 2 * m:
        cap *= 2
    chunk = {"gear": B + 256 * slots, "cut": 256 * slots + 8 * max_chunks, "emit": 8 * max_chunks + 44 * m,
             "pack": 2 * B + pad, "hash": B + pad + 40 * m}
    total = sum(chunk.values())
    return {"content_bytes": B, "files": int(lens.size), "chunks": m, "max_chunks": max_chunks,
            "bytes_chunk": chunk, "passes_over_content": total / B,
            "pcie_bytes_of_the_wait": {"down": 48 + 8 * max_chunks, "up": 8 * m},
            "bytes_hash_yardstick": B + 32 * int(lens.size), "bytes_confirm": 80 * m, "bytes_sharing": 40 * m + 32 * cap,
            "ms_at_hbm_peak": {"chunk": total / HBM_PEAK_GBPS / 1e6, "hash": B / HBM_PEAK_GBPS / 1e6,
                               "confirm": 80 * m / HBM_PEAK_GBPS / 1e6,
                               "sharing": (40 * m + 32 * cap) / HBM_PEAK_GBPS / 1e6}}


# ---- the reference (numpy) -------------------------------------------------------------

def gear_table():
    return (S.mix64(_U(0x3130304344434453) + np.arange(256, dtype=_U)) >> _U(32)).astype(np.uint32)


def ref_ends(x, g, params):
    """the exclusive ends of one file's chunks"""
    min_len, bits, max_len = params
    avg, L = 1 << bits, x.size
    gx = g[x]
    h = gx.copy()
    with np.errstate(over="ignore"):
        for k in range(1, min(32, L)):
            h[k:] += gx[:L - k] << np.uint32(k)
    strict = np.flatnonzero(h < np.uint32(1 << (31 - bits)))
    loose = np.flatnonzero(h < np.uint32(1 << (33 - bits)))
    ends, s = [], 0
    while s < L:
        if L - s <= min_len:
            e = L
        else:
            hi = min(s + max_len, L)
            e = hi
            # STRICT at positions [s + min_len - 1, s + avg - 1), LOOSE at [s + avg - 1, hi)
            a = np.searchsorted(strict, s + min_len - 1)
            if a < strict.size and strict[a] < min(s + avg - 1, hi):
                e = int(strict[a]) + 1
            else:
                b = np.searchsorted(loose, s + avg - 1)
                if b < loose.size and loose[b] < hi:
                    e = int(loose[b]) + 1
        ends.append(e)
        s = e
    return ends


def ref_chunks(blob, offs, lens, params, threads=16):
    g = gear_table()
    work = lambda i: ref_ends(blob[int(offs[i]):int(offs[i]) + int(lens[i])], g, params)
    with ThreadPoolExecutor(threads) as pool:
        per = list(pool.map(work, range(lens.size), chunksize=64))
    fc = np.zeros(lens.size + 1, _U)
    fc[1:] = np.cumsum([len(e) for e in per])
    m = int(fc[-1])
    off, ln, fl = np.zeros(m, _U), np.zeros(m, _U), np.zeros(m, np.uint32)
    c = 0
    for i, ends in enumerate(per):
        s = 0
        for e in ends:
            off[c], ln[c], fl[c] = int(offs[i]) + s, e - s, i
            s = e
            c += 1
    return fc, off, ln, fl


def ref_sharing(fl, ln, rep, n):
    """vectorised: the sums per file and per (file, origin) pair"""
    idx = np.arange(rep.size)
    first = rep == idx
    origin = fl[rep]
    with np.errstate(over="ignore"):
        new = np.bincount(fl[first], ln[first].astype(np.float64), n).astype(_U)  # (sums below 2^53 here)
        own = np.bincount(fl[~first & (origin == fl)], ln[~first & (origin == fl)].astype(np.float64), n).astype(_U)
        sel = ~first & (origin != fl)
        other = np.bincount(fl[sel], ln[sel].astype(np.float64), n).astype(_U)
    pair = fl[sel].astype(_U) << _U(32) | origin[sel].astype(_U)
    up, inv = np.unique(pair, return_inverse=True)
    pb = np.bincount(inv.reshape(-1), ln[sel].astype(np.float64)).astype(_U)
    peer = np.full(n, -1, np.int64)
    peer_bytes = np.zeros(n, _U)
    order = np.lexsort((up & _U(0xFFFFFFFF), ~pb, up >> _U(32)))  # per file: most bytes first, then the lowest origin
    f_sorted = (up >> _U(32))[order]
    lead = np.flatnonzero(np.r_[True, f_sorted[1:] != f_sorted[:-1]]) if order.size else np.zeros(0, np.int64)
    peer[f_sorted[lead].astype(np.int64)] = (up & _U(0xFFFFFFFF))[order][lead].astype(np.int64)
    peer_bytes[f_sorted[lead].astype(np.int64)] = pb[order][lead]
    counts = dict(zip(SHARE_COUNTS, (n, int(rep.size), int(first.sum()), int(ln.sum()), int(ln[first].sum()),
                                     int((peer >= 0).sum()))))
    return new, own, other, peer, peer_bytes, counts


# ---- the device ---------------------------------------------------------------------------

def build_corpus(eng, torch, dev, lens, keys, kind, at):
    n = lens.size
    offs = np.zeros(n, _U)
    offs[1:] = np.cumsum((lens[:-1] + _U(64 + 15)) // _U(16) * _U(16))
    size = int(offs[-1] + lens[-1]) + 64
    blob = torch.zeros(size + 16, dtype=torch.uint8, device=dev)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    own = np.flatnonzero(kind == 0)
    d = [t(a[own]) for a in (keys, np.zeros(n, _U), lens, offs)]
    eng.dev_synth_content(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), own.size, blob.data_ptr())
    eng.dev_sync()
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    for i in np.flatnonzero(kind):
        o, po, a = int(offs[i]), int(offs[i - 1]), int(at[i])
        pl = int(lens[i - 1])
        if kind[i] == 1:
            blob[o:o + a] = blob[po:po + a]
            blob[o + a] = 0x42
            blob[o + a + 1:o + pl + 1] = blob[po + a:po + pl]
        else:
            blob[o:o + pl] = blob[po:po + pl]
            w = min(4096, pl - a)
            blob[o + a:o + a + w] = torch.randint(0, 256, (w,), dtype=torch.uint8, device=dev, generator=gen)
    torch.cuda.synchronize()
    return blob, offs


def device(a, res):
    import torch
    from spacedrive_amd import Engine
    from tests._oracle import load_oracle
    oracle = load_oracle()
    dev = torch.device("cuda", 0)
    lens, keys, kind, at = workload(a.files)
    n = lens.size
    eng = Engine()
    blob, offs = build_corpus(eng, torch, dev, lens, keys, kind, at)
    mc, ms = eng.chunk_plan(lens, PARAMS)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)
    i64 = lambda k: torch.zeros(max(k, 1), dtype=torch.int64, device=dev)
    d_offs, d_lens = t(offs), t(lens)
    fc, off, ln, ckeys, rep, ccnt, scnt, cfcnt = i64(n + 1), i64(mc), i64(mc), i64(mc), i64(mc), i64(6), i64(6), i64(6)
    fl = torch.zeros(mc, dtype=torch.int32, device=dev)
    dig = torch.zeros(32 * mc, dtype=torch.uint8, device=dev)
    fdig = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    share = [i64(n) for _ in range(5)]
    eng.dev_reserve(n, int(((lens + _U(1023)) // _U(1024)).sum()) + n)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    chunk = lambda: eng.dev_chunk(blob.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, mc, ms, PARAMS,
                                  fc.data_ptr(), off.data_ptr(), ln.data_ptr(), fl.data_ptr(), ckeys.data_ptr(),
                                  dig.data_ptr(), ccnt.data_ptr(), sp)
    chunk()
    eng.dev_sync(sp)
    counts = dict(zip(CHUNK_COUNTS, (int(x) for x in ccnt.cpu().numpy().view(_U))))
    m = counts["chunks"]
    whole = lambda: eng.dev_hash_messages(blob.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, fdig.data_ptr(), 0,
                                          sp)
    confirm = lambda: eng.dev_confirm_duplicates(ckeys.data_ptr(), dig.data_ptr(), 0, m, rep.data_ptr(), 0, 0,
                                                 cfcnt.data_ptr(), sp)
    sharing = lambda: eng.dev_chunk_sharing(fl.data_ptr(), ln.data_ptr(), rep.data_ptr(), m, n,
                                            *(o.data_ptr() for o in share), scnt.data_ptr(), sp)
    confirm()
    sharing()
    eng.dev_sync(sp)

    # the reference, before any time is reported
    hblob = blob.cpu().numpy()
    w_fc, w_off, w_ln, w_fl = ref_chunks(hblob, offs, lens, PARAMS)
    wm = int(w_fc[-1])
    equal = {"chunk_count": wm == m}
    if wm == m:
        g_off, g_ln = off.cpu().numpy().view(_U)[:m], ln.cpu().numpy().view(_U)[:m]
        equal["file_chunks"] = bool((fc.cpu().numpy().view(_U) == w_fc).all())
        equal["chunk_off"] = bool((g_off == w_off).all())
        equal["chunk_len"] = bool((g_ln == w_ln).all())
        equal["chunk_file"] = bool((fl.cpu().numpy().view(np.uint32)[:m] == w_fl).all())
        equal["total_bytes"] = counts["total_bytes"] == int(lens.sum()) and counts["files"] == n
        g_dig = dig.cpu().numpy().reshape(-1, 32)[:m]

        def digests_of(lo, hi):
            return b"".join(bytes.fromhex(oracle.hash(hblob[int(w_off[c]):int(w_off[c] + w_ln[c])]))
                            for c in range(lo, hi))
        step = max(1, m // 64)
        with ThreadPoolExecutor(16) as pool:
            parts = list(pool.map(lambda lo: digests_of(lo, min(lo + step, m)), range(0, m, step)))
        w_dig = np.frombuffer(b"".join(parts), np.uint8).reshape(m, 32)
        equal["digests"] = bool((g_dig == w_dig).all())
        equal["keys"] = bool((ckeys.cpu().numpy().view(_U)[:m] == w_dig[:, :8].copy().view(">u8").reshape(-1)).all())
        # rep from the reference digests: the lowest chunk with the same 32 bytes
        _, first_idx, inv = np.unique(w_dig.view(np.dtype((np.void, 32))).reshape(-1), return_index=True,
                                      return_inverse=True)
        w_rep = first_idx[inv.reshape(-1)].astype(np.int64)
        equal["rep"] = bool((rep.cpu().numpy()[:m] == w_rep).all())
        want = ref_sharing(w_fl, w_ln, w_rep, n)
        got = [o.cpu().numpy() for o in share]
        for j, name in enumerate(("new_bytes", "self_bytes", "other_bytes", "peer", "peer_bytes")):
            equal[name] = bool((got[j].view(want[j].dtype) == want[j]).all())
        s_counts = dict(zip(SHARE_COUNTS, (int(x) for x in scnt.cpu().numpy().view(_U))))
        equal["sharing_counts"] = s_counts == want[5]
        res["sharing_counts"] = s_counts
        res["derived_files"] = {"count": int((kind != 0).sum()),
                                "median_peer_share": float(np.median(
                                    want[4][kind != 0].astype(np.float64) / lens[kind != 0].astype(np.float64)))}
    del hblob
    res["chunk_counts"] = counts
    res["model"] = model(lens, m, mc)
    res["outputs_equal_reference"] = equal
    if not all(equal.values()):
        res["device"] = "outputs differ from the reference: no time is reported"
        eng.close()
        return

    legs = {"chunk": chunk, "hash": whole, "confirm": confirm, "sharing": sharing}
    msr = {k: [] for k in legs}
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
            msr[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in msr.items()}
    mo = res["model"]
    B = mo["content_bytes"]
    res["device"] = {
        "reps": a.reps, "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in msr.items()},
        "chunk_over_hash": med["chunk"] / med["hash"],
        "content_GBps": {"chunk": B / med["chunk"] / 1e6, "hash": B / med["hash"] / 1e6},
        "model_GBps": {"chunk": sum(mo["bytes_chunk"].values()) / med["chunk"] / 1e6,
                       "confirm": mo["bytes_confirm"] / med["confirm"] / 1e6,
                       "sharing": mo["bytes_sharing"] / med["sharing"] / 1e6},
        "median_over_model_at_peak": {k: med[k] / mo["ms_at_hbm_peak"][k] for k in legs},
        "hbm_peak_GBps": HBM_PEAK_GBPS,
    }
    eng.close()


def kernel_stats(d, calls):
    """per-kernel milliseconds per call from rocprofv3's *_kernel_stats.csv under d"""
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                found = re.search(r"\bk_\w+", r["Name"])
                if not found:
                    continue  # not one of the library's kernels (copies, the corpus builder's)
                name = found.group(0)
                rows.setdefault(name, [0, 0.0])
                rows[name][0] += int(r["Calls"])
                rows[name][1] += float(r["TotalDurationNs"])
    return {k: {"launches": v[0], "ms_per_call": v[1] / 1e6 / calls} for k, v in sorted(rows.items(), key=lambda x: -x[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--count-only", action="store_true", help="the model's bytes alone: no device")
    ap.add_argument("--kernel-stats", help="a rocprofv3 --kernel-trace --stats output directory of this tool's run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_sharing.json"))
    a = ap.parse_args()
    res = {"tool": "tools/ab_chunks.py", "files": a.files, "params": list(PARAMS)}
    if a.count_only:
        lens = workload(a.files)[0]
        mc = int(((lens + _U(PARAMS[0] - 1)) // _U(PARAMS[0])).sum())
        # (without the content the chunk count is an estimate: a cut every min_len + avg bytes on average)
        m = int((lens // _U(PARAMS[0] + (1 << PARAMS[1]))).sum()) + int(lens.size)
        res["model"] = model(lens, m, mc)
        res["model"]["chunks_are_an_estimate"] = True
        print(json.dumps(res))
        return
    if a.kernel_stats:
        with open(a.out) as f:
            res = json.load(f)
        # warm-up 1 + 2 and the timed repetitions, per leg
        res["kernel_trace"] = {"calls_per_leg": a.reps + 3, "kernels": kernel_stats(a.kernel_stats, a.reps + 3)}
    else:
        device(a, res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
