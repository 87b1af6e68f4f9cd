#!/usr/bin/env python3
"""A/B of the one-pass cas_id + checksum (sdcas_dev_identify, csrc/b3_dual.hip)
against the two passes it replaces, legs alternating in ONE process
(cdna_hip_programming.md §5.4 rule 24), HIP events around work that ends in a
sync.

Device (C2's shape: contents of 1-100 KiB from dev_synth_content, resident):
  A  dev_hash_messages over the cas messages (le64(size) || content)
  B  dev_hash_messages over the contents
  D  dev_identify over the contents
A and B are code this kernel does not touch. Reports D / (A + B), each leg's
compressions x 680 / time / 78.64 T, and D's outputs against A's and B's.

End to end (--e2e-files N): identify_checksums over N C2-shaped files in the
page cache against file_metadata followed by file_checksums, alternating,
and the bytes each stages for upload — the sum over files of len against
2 * len + 8 (plus the reads' spare byte), counted from the sizes with the
staging rule (128-byte aligned slots), which needs no device: --count-only.

Writes one JSON object (--out, default profiles/dual_identify.json)."""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

PEAK = 78.6432e12  # int32 VALU lane-ops/s (bench.py's roofline)


def align(x, a):
    a = np.uint64(a)
    return (x + a - np.uint64(1)) // a * a


def upload_bytes(sizes):
    """bytes each path stages for upload, from the sizes alone"""
    s = sizes.astype(np.uint64)
    one = np.uint64(1)
    return {
        "content_bytes": int(s.sum()),
        "two_pass_message_bytes": int((2 * s + np.uint64(8)).sum()),
        "identify_staged": int(align(s, 128).sum()),
        "two_pass_staged": int(align(s + np.uint64(8) + one, 128).sum() + align(s + one, 128).sum()),
    }


def device_ab(a, res):
    import torch
    from spacedrive_amd import Engine
    dev = torch.device("cuda", 0)
    n = a.files
    sizes, keys, _ = bench.files_of("c2", 0, n)
    sizes = sizes.astype(np.uint64)
    mlens = sizes + np.uint64(8)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(dev)

    def lay(lens):
        padded = align(lens, 128)
        offs = np.zeros(n, np.uint64)
        offs[1:] = np.cumsum(padded[:-1])
        return offs, int(offs[-1] + padded[-1]) + 64

    moffs, mtotal = lay(mlens)
    coffs, ctotal = lay(sizes)
    chunks = lambda l: int(np.maximum(np.uint64(1), (l + np.uint64(1023)) // np.uint64(1024)).sum())
    eng = Engine()
    mblob = torch.empty(mtotal, dtype=torch.uint8, device=dev)
    cblob = torch.empty(ctotal, dtype=torch.uint8, device=dev)
    dk, ds, dmo, dml, dco = t(keys), t(sizes), t(moffs), t(mlens), t(coffs)
    zero = torch.zeros(n, dtype=torch.int64, device=dev)
    eng.dev_reserve(n, 2 * (chunks(mlens) + 2048) + 4096)
    stream = torch.cuda.Stream()  # a stream of its own: handle 0 would name the context's stream, not torch's
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    eng.dev_synth_cas_messages(dk.data_ptr(), ds.data_ptr(), dmo.data_ptr(), n, mblob.data_ptr(), sp)
    eng.dev_synth_content(dk.data_ptr(), zero.data_ptr(), ds.data_ptr(), dco.data_ptr(), n, cblob.data_ptr(), sp)
    ka = torch.zeros(n, dtype=torch.int64, device=dev)
    kd = torch.zeros(n, dtype=torch.int64, device=dev)
    db = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    dd = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    legs = {
        "A": lambda: eng.dev_hash_messages(mblob.data_ptr(), dmo.data_ptr(), dml.data_ptr(), n, 0, ka.data_ptr(), sp),
        "B": lambda: eng.dev_hash_messages(cblob.data_ptr(), dco.data_ptr(), ds.data_ptr(), n, db.data_ptr(), 0, sp),
        "D": lambda: eng.dev_identify(cblob.data_ptr(), dco.data_ptr(), ds.data_ptr(), n, kd.data_ptr(), dd.data_ptr(),
                                      0, sp),
    }
    ms = {k: [] for k in legs}
    for k, f in legs.items():  # warm every leg (D's first call allocates its scratch)
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
    comp = {"A": int(bench.compressions(mlens).sum()), "B": int(bench.compressions(sizes).sum())}
    comp["D"] = comp["A"] + comp["B"]
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res["device"] = {
        "files": n, "content_bytes": int(sizes.sum()), "reps": a.reps,
        "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
        "compressions": comp,
        "valu_frac": {k: comp[k] * 680 / (med[k] * 1e-3) / PEAK for k in legs},
        "D_over_A_plus_B": med["D"] / (med["A"] + med["B"]),
        "keys_equal_A": bool(torch.equal(kd, ka)),
        "digests_equal_B": bool(torch.equal(dd, db)),
    }
    eng.close()


def e2e(a, res):
    from spacedrive_amd import Engine
    n = a.e2e_files
    sizes, _, _ = bench.files_of("c2", 0, n)
    res["e2e"] = {"files": n, "upload": upload_bytes(sizes)}
    if a.count_only:
        return
    d = a.dir
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    buf = np.random.default_rng(1).integers(0, 256, 1 << 17, dtype=np.uint8).tobytes()
    paths = []
    for i in range(n):
        p = os.path.join(d, f"{i:07d}")
        with open(p, "wb") as f:
            f.write(buf[: int(sizes[i])])
        paths.append(p)
    os.sync()
    try:
        with Engine() as e:
            best = {"two_pass": None, "identify": None}
            same = True
            for r in range(a.e2e_reps + 1):  # the first round reads every file once (page cache) and warms both
                t0 = time.perf_counter()
                msz, mk, mst, mfl = e.file_metadata(paths, sizes)
                cd, cst = e.file_checksums(paths)
                t1 = time.perf_counter()
                isz, ik, idg, ist, ifl = e.identify_checksums(paths, sizes)
                t2 = time.perf_counter()
                same = same and np.array_equal(mk, ik) and np.array_equal(cd, idg) and not ist.any() and not cst.any()
                if r == 0:
                    continue
                for k, dt in (("two_pass", t1 - t0), ("identify", t2 - t1)):
                    best[k] = dt if best[k] is None else min(best[k], dt)
        res["e2e"].update({"files_per_s": {k: n / v for k, v in best.items()},
                           "identify_over_two_pass_time": best["identify"] / best["two_pass"],
                           "same_results": bool(same)})
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1_000_000, help="device A/B: contents resident in HBM (0: skip)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-files", type=int, default=200_000, help="files in the page cache (0: skip)")
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--count-only", action="store_true", help="the upload-byte count alone: no device, no files")
    ap.add_argument("--dir", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "sdcas_ab_dual"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_identify.json"))
    a = ap.parse_args()
    res = {"tool": "tools/ab_dual.py"}
    if a.files and not a.count_only:
        device_ab(a, res)
    if a.e2e_files:
        e2e(a, res)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
