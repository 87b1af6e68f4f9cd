#!/usr/bin/env python3
"""Timing of the directory digests and the top-most duplicate rule
(sdcas_dev_tree_digests, sdcas_dev_tree_top, csrc/dirtree.hip) beside the two
calls they feed, sdcas_dev_confirm_duplicates and sdcas_dev_duplicate_sets
over the same entries: the four legs alternating in ONE process, HIP events
around work that ends in a sync, 20 repetitions after a warm-up.

Workload: a seeded generated tree (--entries, default about 6 M): depth <= 12,
heavy-tailed directory sizes (a clipped Pareto), one directory of 200 000
files, about a third of the depth-1 subtrees cloned as siblings and then about
a third of the root subtrees cloned (so some clones lie in clones). A clone
keeps names, digests and sizes and gets a new name for its top.

Before any time is reported every output is compared with this tool's own
reference: numpy for the order, the rollups and the top-most rule, the CPU
BLAKE3 of the test oracle for the digests. The host wall clock of that
reference is recorded as a number of a DIFFERENT KIND (one Python thread; not a
device time, not alternated with the legs).

No threshold: the numbers are recorded (--out, default
profiles/duplicate_trees.json). --count-only prints the model without a device.

The model (the least HBM traffic of the scheme, pass by pass; n entries, F
files, D directories, C = n - roots children, T = ceil(n / 4096) tiles, p the
parent sort's digits):
  clear        16 n written (the accumulators)
  keys         8 n read, 12 n written
  name sort    8 digits: 8 n read (histogram), 12 n read + 12 n written
               (scatter), 4 KiB per tile
  parent keys  4 n + 4 n read, 4 n written
  parent sort  p digits: 4 n read, 8 n read + 8 n written, 4 KiB per tile
  fix          8 n read (entry, rank), 24 n read (own and both neighbours'
               prefixes), 4 n written
  files        n read, 8 F read, 17 F written
  gather       per child 4 + 4 + 16 read (position, rank, the directory's
               numbers), 1 + 64 + 9 read (kind, name, content, size or
               accumulators), 72 written, 16 of atomics
  head         per directory 16 read, 32 written
  hash         the messages read once: 16 D + 72 C, 32 D written
  finish       per directory 20 + 32 read, 58 written
  top          12 n cleared; count 8 n read + 8 per participating entry; mark
               and write 2 x (16 n read + 8 per entry with a parent), 9 n written
The shape's upload (5 n + 16 D bytes over PCIe) is not HBM traffic and is
listed apart."""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

_U = np.uint64
TILE = 4096
HBM_PEAK_GBPS = 8000.0
MAX_DEPTH = 12
BIG_DIR = 200_000
TREE_COUNTS = ("entries", "dirs", "complete_dirs", "empty_dirs", "levels", "largest_dir")
TOP_COUNTS = ("entries", "dup_entries", "nested_entries", "top_entries", "kept_classes", "dropped_classes")
SETS_COUNTS = ("files", "sets", "members", "duplicate_files", "reclaimable_bytes", "largest_set")


# ---- the generated tree ------------------------------------------------------------

def _grow(rng, roots):
    """`roots` root directories grown level by level -> parent, is_dir, depth"""
    parent = [np.full(roots, -1, np.int64)]
    is_dir = [np.ones(roots, np.uint8)]
    depth = [np.zeros(roots, np.int64)]
    dirs, base = np.arange(roots, dtype=np.int64), roots
    for level in range(1, MAX_DEPTH):
        kids = np.minimum((rng.pareto(1.2, dirs.size) * 2.5).astype(np.int64), 4000)
        p = np.repeat(dirs, kids)
        share = 0.0 if level == MAX_DEPTH - 1 else 0.10
        d = (rng.random(p.size) < share).astype(np.uint8)
        parent.append(p), is_dir.append(d), depth.append(np.full(p.size, level, np.int64))
        dirs = base + np.flatnonzero(d)
        base += p.size
        if not dirs.size:
            break
    return np.concatenate(parent), np.concatenate(is_dir), np.concatenate(depth)


def _clone(rng, t, tops):
    """append a copy of every subtree whose top is in `tops` (entries of one
    depth), each as a sibling of its original under a new name"""
    parent, depth = t["parent"], t["depth"]
    n = parent.size
    level = int(depth[tops[0]])
    anc = np.arange(n, dtype=np.int64)  # the ancestor at `level`, -1 above it
    anc[depth < level] = -1
    for _ in range(MAX_DEPTH):
        deeper = (anc >= 0) & (depth[np.maximum(anc, 0)] > level)
        if not deeper.any():
            break
        anc[deeper] = parent[anc[deeper]]
    chosen = np.zeros(n, bool)
    chosen[tops] = True
    e = np.flatnonzero((anc >= 0) & chosen[np.maximum(anc, 0)])
    new = np.full(n, -1, np.int64)
    new[e] = n + np.arange(e.size)
    is_top = depth[e] == level
    t["parent"] = np.r_[parent, np.where(is_top, parent[e], new[np.maximum(parent[e], 0)])]
    for k in ("is_dir", "depth", "sizes", "valid"):
        t[k] = np.r_[t[k], t[k][e]]
    names = t["names"][e].copy()
    names[is_top] = rng.integers(0, 256, (int(is_top.sum()), 32), dtype=np.uint8)
    t["names"] = np.concatenate([t["names"], names])
    t["digests"] = np.concatenate([t["digests"], t["digests"][e]])


def generate(entries, seed=1):
    """about `entries` entries: the number of roots is corrected (a few
    times) from the size the heavy-tailed growth actually gave, and the
    closest tree is kept"""
    big = min(BIG_DIR, max(1, entries // 4))
    roots = max(3, (entries - big) // 600)
    best = None
    for _ in range(6):
        t = _generate(roots, big, seed)
        got = t["parent"].size
        if best is None or abs(got - entries) < abs(best["parent"].size - entries):
            best = t
        if 0.85 * entries <= got <= 1.15 * entries:
            break
        roots = max(3, int(roots * (entries - big) / max(got - big, 1)))
    return best


def _generate(roots, big, seed):
    rng = np.random.default_rng(seed)
    parent, is_dir, depth = _grow(rng, roots)
    n = parent.size
    t = {"parent": parent, "is_dir": is_dir, "depth": depth,
         "names": rng.integers(0, 256, (n, 32), dtype=np.uint8),
         "digests": rng.integers(0, 256, (n, 32), dtype=np.uint8),
         "sizes": np.where(is_dir == 0, (rng.pareto(1.1, n) * 20000).astype(_U) % _U(1 << 34), 0).astype(_U),
         "valid": ((rng.random(n) > 0.0005) & (is_dir == 0)).astype(np.uint8)}
    for level in (1, 0):  # clones inside the root subtrees first, then root subtrees with their clones
        tops = np.flatnonzero((t["depth"] == level) & (t["is_dir"] != 0))
        tops = tops[rng.random(tops.size) < 1 / 3]
        if tops.size:
            _clone(rng, t, tops)
    # one directory of BIG_DIR files, as a root
    n = t["parent"].size
    t["parent"] = np.r_[t["parent"], -1, np.full(big, n)]
    t["is_dir"] = np.r_[t["is_dir"], 1, np.zeros(big, np.uint8)].astype(np.uint8)
    t["depth"] = np.r_[t["depth"], 0, np.ones(big, np.int64)]
    t["names"] = np.concatenate([t["names"], rng.integers(0, 256, (big + 1, 32), dtype=np.uint8)])
    t["digests"] = np.concatenate([t["digests"], rng.integers(0, 256, (big + 1, 32), dtype=np.uint8)])
    t["sizes"] = np.r_[t["sizes"], 0, rng.integers(1, 1 << 22, big).astype(_U)].astype(_U)
    t["valid"] = np.r_[t["valid"], 0, np.ones(big, np.uint8)].astype(np.uint8)
    # entries in no particular order: children may stand before their parents
    n = t["parent"].size
    perm = rng.permutation(n)  # new index of old entry i
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    out = {k: np.ascontiguousarray(v[inv]) for k, v in t.items()}
    out["parent"] = np.where(out["parent"] >= 0, perm[np.maximum(out["parent"], 0)], -1).astype(np.int64)
    d = out["is_dir"] != 0
    out["digests"][d] = 0
    out["keys"] = np.zeros(n, _U)
    out["keys"][~d] = out["digests"][~d, :8].copy().view(">u8").reshape(-1).astype(_U)
    del out["depth"]
    return out


# ---- the reference -----------------------------------------------------------------

def depths(parent):
    n = parent.size
    depth = np.full(n, -1, np.int64)
    depth[parent < 0] = 0
    todo = np.flatnonzero(parent >= 0)
    while todo.size:
        pd = depth[parent[todo]]
        ready = pd >= 0
        assert ready.any(), "a cycle"
        depth[todo[ready]] = pd[ready] + 1
        todo = todo[~ready]
    return depth


def reference(t, hash_fn):
    """numpy + CPU BLAKE3: the arrays sdcas_tree_digests answers with"""
    parent, is_dir = t["parent"], t["is_dir"]
    n = parent.size
    depth = depths(parent)
    w = t["names"].view(">u8").reshape(n, 4)
    order = np.lexsort((np.arange(n), w[:, 3], w[:, 2], w[:, 1], w[:, 0], parent))  # by parent, name, index
    order = order[parent[order] >= 0]
    po = parent[order]
    starts = np.flatnonzero(np.r_[True, po[1:] != po[:-1]]) if po.size else np.zeros(0, np.int64)
    first = np.full(n, -1, np.int64)
    first[po[starts]] = starts
    k = np.bincount(po, minlength=n).astype(np.int64)
    dig, keys, valid = t["digests"].copy(), t["keys"].copy(), t["valid"].copy()
    d = is_dir != 0
    tree_bytes = np.where(d, 0, t["sizes"]).astype(_U)
    tree_files = np.where(d, 0, 1).astype(_U)
    complete = np.where(d, True, valid != 0)
    flags = np.zeros(n, np.uint8)
    head = b"SDTREE01"
    for level in range(int(depth.max()), -1, -1):
        for i in np.flatnonzero(d & (depth == level)):
            c = order[first[i]:first[i] + k[i]] if k[i] else order[:0]
            with np.errstate(over="ignore"):
                tree_bytes[i] = tree_bytes[c].sum(dtype=_U)
            tree_files[i] = tree_files[c].sum(dtype=_U)
            complete[i] = bool(complete[c].all())
            empty = tree_files[i] == 0
            flags[i] = 1 | (0 if complete[i] else 2) | (4 if empty else 0)
            if complete[i]:
                rec = np.empty((c.size, 72), np.uint8)
                rec[:, :32], rec[:, 32:64] = t["names"][c], dig[c]
                rec[:, 64:] = 0
                rec[:, 64] = is_dir[c]
                dig[i] = np.frombuffer(hash_fn(head + struct.pack("<Q", c.size) + rec.tobytes()), np.uint8)
                keys[i] = int.from_bytes(dig[i, :8].tobytes(), "big")
            else:
                dig[i], keys[i] = 0, 0
            valid[i] = 1 if complete[i] and not empty else 0
    counts = dict(zip(TREE_COUNTS, (n, int(d.sum()), int((d & complete).sum()), int((d & (tree_files == 0)).sum()),
                                    int(depth.max()) + 1, int(k[d].max()) if d.any() else 0)))
    return {"keys": keys, "digests": dig, "valid": valid, "tree_bytes": tree_bytes, "tree_files": tree_files,
            "flags": flags, "counts": counts, "depth": depth}


def top_reference(parent, rep):
    n = rep.size
    part = (rep >= 0) & (rep < n)
    carriers = np.bincount(rep[part], minlength=n)
    dup = np.zeros(n, bool)
    dup[part] = carriers[rep[part]] >= 2
    nested = np.zeros(n, bool)
    has = dup & (parent >= 0)
    nested[has] = dup[parent[has]]
    loose = np.zeros(n, bool)
    loose[rep[dup & ~nested]] = True
    kept = np.zeros(n, bool)
    kept[dup] = loose[rep[dup]]
    classes = np.unique(rep[dup])
    counts = dict(zip(TOP_COUNTS, (int(part.sum()), int(dup.sum()), int(nested.sum()), int(kept.sum()),
                                   int(loose[classes].sum()), int((~loose[classes]).sum()))))
    return np.where(kept, rep, -1).astype(np.int64), (dup * 1 + nested * 2).astype(np.uint8), counts


# ---- the model -----------------------------------------------------------------------

def model(t):
    parent, is_dir = t["parent"], t["is_dir"]
    n = parent.size
    dirs = int((is_dir != 0).sum())
    files = n - dirs
    roots = int((parent < 0).sum())
    c = n - roots
    depth = depths(parent)
    k = np.bincount(parent[parent >= 0], minlength=n)
    tiles = max(1, -(-n // TILE))
    bits = 1
    while (1 << bits) <= dirs:
        bits += 1
    p = -(-bits // 8)
    tree = {
        "clear": 16 * n,
        "keys": 20 * n,
        "name_sort": 8 * (32 * n + 4096 * tiles),
        "parent_keys": 12 * n,
        "parent_sort": p * (20 * n + 4096 * tiles),
        "fix": 36 * n,
        "files": n + 25 * files,
        "gather": (24 + 74 + 72 + 16) * c,
        "head": 48 * dirs,
        "hash": 16 * dirs + 72 * c + 32 * dirs,
        "finish": 110 * dirs,
    }
    with_parent = c
    top = {"clear": 12 * n, "count": 16 * n, "mark": 16 * n + 8 * with_parent,
           "write": 16 * n + 8 * with_parent + 9 * n}
    tb, pb = sum(tree.values()), sum(top.values())
    level_dirs = np.bincount(depth[is_dir != 0]) if dirs else np.zeros(0, np.int64)
    return {"entries": n, "files": files, "dirs": dirs, "roots": roots, "levels": int(depth.max()) + 1 if n else 0,
            "dir_levels": int(level_dirs.size), "largest_dir": int(k[is_dir != 0].max()) if dirs else 0,
            "message_bytes": 16 * dirs + 72 * c, "parent_sort_passes": p,
            "bytes_tree_digests": tree, "bytes_tree_top": top,
            "bytes_per_entry": {"tree_digests": tb / n, "tree_top": pb / n},
            "ms_at_hbm_peak": {"tree_digests": tb / HBM_PEAK_GBPS / 1e6, "tree_top": pb / HBM_PEAK_GBPS / 1e6},
            "shape_upload_bytes": 5 * n + 16 * dirs,
            "launches": {"tree_digests_fixed": 4 + 8 * 5 + p * 5, "per_level_with_directories": "3 + the batch hash's"}}


# ---- the device ------------------------------------------------------------------------

def device(a, t, res):
    import torch
    import ab_sets
    from spacedrive_amd import Engine
    from tests._oracle import load_oracle
    oracle = load_oracle()
    hash_fn = lambda m: bytes.fromhex(oracle.hash(m))
    t0 = time.perf_counter()
    want = reference(t, hash_fn)
    ref_s = time.perf_counter() - t0

    dev = torch.device("cuda", 0)
    n = t["parent"].size
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.uint8).copy()).to(dev)
    d = {k: up(t[k]) for k in ("names", "digests", "keys", "valid", "sizes", "parent")}
    i64 = lambda m: torch.zeros(max(m, 1), dtype=torch.int64, device=dev)
    u8 = lambda m: torch.zeros(max(m, 1), dtype=torch.uint8, device=dev)
    tb, tf, fl, cts = i64(n), i64(n), u8(n), i64(6)
    rep, top, tfl, tcts = i64(n), i64(n), u8(n), i64(6)
    h = n // 2
    sets_out = [i64(c) for c in (h, h + 1, h, n, 6)]
    eng = Engine()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()
    tree = lambda: eng.dev_tree_digests(t["parent"], t["is_dir"], d["names"].data_ptr(), d["sizes"].data_ptr(), n,
                                        d["keys"].data_ptr(), d["digests"].data_ptr(), d["valid"].data_ptr(),
                                        tb.data_ptr(), tf.data_ptr(), fl.data_ptr(), cts.data_ptr(), sp)
    confirm = lambda: eng.dev_confirm_duplicates(d["keys"].data_ptr(), d["digests"].data_ptr(), d["valid"].data_ptr(),
                                                 n, rep.data_ptr(), 0, 0, 0, sp)
    tops = lambda: eng.dev_tree_top(d["parent"].data_ptr(), rep.data_ptr(), n, top.data_ptr(), tfl.data_ptr(),
                                    tcts.data_ptr(), sp)
    sets = lambda: eng.dev_duplicate_sets(top.data_ptr(), tb.data_ptr(), n, *(o.data_ptr() for o in sets_out), 1, sp)
    for f in (tree, confirm, tops, sets):
        f()
    eng.dev_sync(sp)

    host = lambda x, dt: x.cpu().numpy().view(dt)
    equal = {
        "digests": bool((host(d["digests"], np.uint8).reshape(n, 32) == want["digests"]).all()),
        "keys": bool((host(d["keys"], _U) == want["keys"]).all()),
        "valid": bool((host(d["valid"], np.uint8) == want["valid"]).all()),
        "tree_bytes": bool((host(tb, _U) == want["tree_bytes"]).all()),
        "tree_files": bool((host(tf, _U) == want["tree_files"]).all()),
        "flags": bool((host(fl, np.uint8) == want["flags"]).all()),
        "tree_counts": dict(zip(TREE_COUNTS, (int(x) for x in host(cts, _U)))) == want["counts"],
    }
    hrep = host(rep, np.int64)
    wtop = top_reference(t["parent"], hrep)
    equal["top_rep"] = bool((host(top, np.int64) == wtop[0]).all())
    equal["top_flags"] = bool((host(tfl, np.uint8) == wtop[1]).all())
    equal["top_counts"] = dict(zip(TOP_COUNTS, (int(x) for x in host(tcts, _U)))) == wtop[2]
    wsets = ab_sets.group(wtop[0], want["tree_bytes"], True)
    got = [o.cpu().numpy() for o in sets_out]
    s, m = wsets[4]["sets"], wsets[4]["members"]
    equal["sets"] = bool(dict(zip(SETS_COUNTS, (int(x) for x in got[4].view(_U)))) == wsets[4] and
                         (got[0][:s] == wsets[0]).all() and (got[3][:m] == wsets[3]).all() and
                         (got[2][:s].view(_U) == wsets[2]).all())
    res["model"] = model(t)
    res["outputs_equal_reference"] = equal
    res["counts"] = {"tree": want["counts"], "top": wtop[2], "sets": wsets[4]}
    is_dir_set = int((t["is_dir"][wsets[0]] != 0).sum()) if s else 0
    res["counts"]["directory_sets"] = is_dir_set
    if not all(equal.values()):
        res["device"] = "outputs differ from the reference: no time is reported"
        eng.close()
        return

    legs = {"tree_digests": tree, "confirm": confirm, "tree_top": tops, "duplicate_sets_by_reclaimable": sets}
    ms = {k: [] for k in legs}
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
            ms[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    mo = res["model"]
    res["device"] = {
        "reps": a.reps, "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
        "what": "HIP events around each call; tree_digests includes the host's shape pass and upload, which "
                "run before its kernels are enqueued",
        "model_GBps": {"tree_digests": mo["bytes_per_entry"]["tree_digests"] * n / (med["tree_digests"] * 1e-3) / 1e9,
                       "tree_top": mo["bytes_per_entry"]["tree_top"] * n / (med["tree_top"] * 1e-3) / 1e9},
        "over_model_at_hbm_peak": {"tree_digests": med["tree_digests"] / mo["ms_at_hbm_peak"]["tree_digests"],
                                   "tree_top": med["tree_top"] / mo["ms_at_hbm_peak"]["tree_top"]},
        "hbm_peak_GBps": HBM_PEAK_GBPS,
    }
    # the host side of one tree_digests call alone (shape pass + enqueue), wall clock
    w = []
    for _ in range(3):
        eng.dev_sync(sp)
        t0 = time.perf_counter()
        tree()
        w.append(time.perf_counter() - t0)
        eng.dev_sync(sp)
    res["tree_digests_host_enqueue_ms"] = {"what": "host wall clock until the call returns (shape pass, upload, "
                                                   "launches), not a device time", "median": float(np.median(w)) * 1e3}
    res["cpu_reference"] = {
        "what": "host wall clock, a different kind of number: this tool's numpy + CPU BLAKE3 reference for the "
                "tree digests over the same tree, one Python thread; not a device time",
        "seconds": ref_s}
    eng.close()


def kernel_stats(path):
    """rocprofv3's trace_kernel_stats.csv of a (separate) traced run of this
    tool, summed per sdcas_dev_tree_digests call -> the profile's kernel_trace
    block. The traced run's calls are k_dt_keys' launches."""
    import csv
    rows = list(csv.DictReader(open(path)))
    short = lambda r: r["Name"].split("::")[-1].split("(")[0]
    pick = lambda *names: [r for r in rows if any(k in r["Name"] for k in names)]
    total_ms = lambda rs: sum(int(r["TotalDurationNs"]) for r in rs) / 1e6
    calls = sum(int(r["Calls"]) for r in pick("k_dt_keys"))
    hash_ms = total_ms(pick("k_leaf_tree", "k_finish_q", "k_finish_t", "k_shape_", "k_plan_")) / calls
    dt = {short(r): int(r["TotalDurationNs"]) / 1e6 / calls for r in pick("k_dt_")}
    # the sorts' kernels are shared with the duplicate sets, whose few launches in the traced run are
    # counted in: an upper bound for the tree call's two sorts and the long-run path's empty passes
    sort_ms = total_ms(pick("k_ds_scatter", "k_ds_hist", "k_ds_scan")) / calls
    sort_launches = sum(int(r["Calls"]) for r in pick("k_ds_scatter", "k_ds_hist", "k_ds_scan")) / calls
    new_ms = sum(dt.values()) + sort_ms
    return {"what": "a separate rocprofv3 --kernel-trace --stats run of this tool, merged with --kernel-stats; "
                    "milliseconds per sdcas_dev_tree_digests call",
            "tree_digests_calls": calls,
            "levels_with_directories": sum(int(r["Calls"]) for r in pick("k_dt_finish")) / calls,
            "tree_digests_ms_per_call": {"batch_hash": hash_ms, "k_dt_kernels": dt,
                                         "sort_kernels_upper_bound": sort_ms,
                                         "sort_kernel_launches_upper_bound": sort_launches,
                                         "all_but_the_batch_hash": new_ms,
                                         "batch_hash_share_of_kernel_time": hash_ms / (hash_ms + new_ms)},
            "batch_hash_largest_launch_ms": {short(r): int(r["MaxNs"]) / 1e6 for r in pick("k_leaf_tree", "k_finish_q")},
            "tree_top_average_ms_per_launch": {short(r): float(r["AverageNs"]) / 1e6
                                               for r in pick("k_tt_", "k_ds_count")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=6_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--count-only", action="store_true", help="the model's bytes alone: no device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duplicate_trees.json"))
    ap.add_argument("--kernel-stats", metavar="CSV",
                    help="merge a traced run's trace_kernel_stats.csv into --out as its kernel_trace block: no device")
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            res = json.load(f)
        res["kernel_trace"] = kernel_stats(a.kernel_stats)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res["kernel_trace"]))
        return
    t = generate(a.entries, a.seed)
    res = {"tool": "tools/ab_tree.py", "entries_asked": a.entries, "seed": a.seed}
    if a.count_only:
        res["model"] = model(t)
        print(json.dumps(res))
        return
    device(a, t, res)
    if os.path.exists(a.out):  # a kernel_trace block merged earlier stays, marked as the earlier run's
        try:
            with open(a.out) as f:
                old = json.load(f).get("kernel_trace")
            if old:
                res["kernel_trace"] = dict(old, stale="from a traced run before these timings were taken")
        except (OSError, ValueError):
            pass
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
