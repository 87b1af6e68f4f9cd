"""Test infrastructure: the definitions of include/sdcas.h's "duplicate
directories" section restated in plain Python over numpy arrays — the shape
check (sdcas_tree_plan), the directory digests with their flags, rollups and
counts (sdcas_tree_digests) and the top-most duplicates (sdcas_tree_top).
BLAKE3 is the oracle's `hash()`. tests/test_tree_ref.py checks it on a tree
written out by hand."""
import struct

import numpy as np

INVALID, CAPACITY = -2, -5  # SDCAS_E_INVALID, SDCAS_E_CAPACITY
MAX_DEPTH = 4096
DIR, INCOMPLETE, EMPTY = 1, 2, 4
DUP, NESTED = 1, 2
TREE_COUNTS = ("entries", "dirs", "complete_dirs", "empty_dirs", "levels", "largest_dir")
TOP_COUNTS = ("entries", "dup_entries", "nested_entries", "top_entries", "kept_classes", "dropped_classes")


class ShapeError(Exception):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def tree_plan(parent, is_dir):
    """-> (depth uint32[n], children uint64[n], levels); ShapeError otherwise"""
    parent = np.asarray(parent, np.int64)
    is_dir = np.asarray(is_dir, np.uint8)
    n = parent.size
    if n > 1 << 30:
        raise ShapeError(CAPACITY, "more than 2^30 entries")
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint64), 0
    if ((parent < -1) | (parent >= n)).any():
        raise ShapeError(INVALID, "a parent outside [-1, n)")
    has = parent >= 0
    if (is_dir[parent[has]] == 0).any():
        raise ShapeError(INVALID, "a parent that is not a directory")
    children = np.bincount(parent[has], minlength=n).astype(np.uint64)
    depth = np.full(n, -1, np.int64)
    depth[~has] = 0
    todo = np.flatnonzero(has)
    while todo.size:  # one level per round
        pd = depth[parent[todo]]
        ready = pd >= 0
        if not ready.any():
            raise ShapeError(INVALID, "an entry that is its own ancestor")
        depth[todo[ready]] = pd[ready] + 1
        todo = todo[~ready]
    levels = int(depth.max()) + 1
    if levels > MAX_DEPTH:
        raise ShapeError(CAPACITY, "more than SDCAS_TREE_MAX_DEPTH levels")
    return depth.astype(np.uint32), children, levels


def child_order(parent, name32):
    """per entry: its direct children, ascending by (name32 as 32 bytes, index)"""
    parent = np.asarray(parent, np.int64)
    n = parent.size
    names = np.asarray(name32, np.uint8).reshape(n, 32)
    nb = [names[i].tobytes() for i in range(n)]
    kids = [[] for _ in range(n)]
    for i in range(n):
        if parent[i] >= 0:
            kids[parent[i]].append(i)
    for k in kids:
        k.sort(key=lambda c: (nb[c], c))
    return kids, nb


def tree_digests(oracle, parent, is_dir, name32, digests, valid=None, sizes=None, keys=None):
    """-> dict: keys, digests, valid (None when none was given), tree_bytes,
    tree_files, flags, counts, and T (hex by directory index, complete ones)"""
    parent = np.asarray(parent, np.int64)
    is_dir = np.asarray(is_dir, np.uint8)
    n = parent.size
    depth, children, levels = tree_plan(parent, is_dir)
    dig = np.array(digests, np.uint8).reshape(n, 32).copy()
    va = None if valid is None else np.array(valid, np.uint8).copy()
    ks = np.zeros(n, np.uint64) if keys is None else np.array(keys, np.uint64).copy()
    sz = np.zeros(n, np.uint64) if sizes is None else np.asarray(sizes, np.uint64)
    kids, nb = child_order(parent, name32)
    tree_bytes = np.zeros(n, np.uint64)
    tree_files = np.zeros(n, np.uint64)
    flags = np.zeros(n, np.uint8)
    complete = np.ones(n, bool)
    T = {}
    order = sorted(range(n), key=lambda i: -int(depth[i]))  # deepest first
    for i in order:
        if not is_dir[i]:
            tree_bytes[i] = sz[i]
            tree_files[i] = 1
            complete[i] = True if va is None else bool(va[i])
            continue
        tb, tf, ok = 0, 0, True
        for c in kids[i]:
            tb = (tb + int(tree_bytes[c])) & 0xFFFFFFFFFFFFFFFF
            tf += int(tree_files[c])
            ok = ok and complete[c]
        tree_bytes[i], tree_files[i], complete[i] = tb, tf, ok
        empty = tf == 0
        flags[i] = DIR | (0 if ok else INCOMPLETE) | (EMPTY if empty else 0)
        if ok:
            msg = b"SDTREE01" + struct.pack("<Q", len(kids[i])) + b"".join(
                nb[c] + dig[c].tobytes() + struct.pack("<Q", 1 if is_dir[c] else 0) for c in kids[i])
            assert len(msg) == 16 + 72 * len(kids[i])
            T[i] = oracle.hash(msg)
            dig[i] = np.frombuffer(bytes.fromhex(T[i]), np.uint8)
            ks[i] = int(T[i][:16], 16)
        else:
            dig[i] = 0
            ks[i] = 0
        if va is not None:
            va[i] = 1 if ok and not empty else 0
    d = is_dir != 0
    counts = {"entries": n, "dirs": int(d.sum()), "complete_dirs": int((d & complete).sum()),
              "empty_dirs": int((d & (tree_files == 0)).sum()), "levels": levels,
              "largest_dir": int(children[d].max()) if d.any() else 0}
    return {"keys": ks, "digests": dig, "valid": va, "tree_bytes": tree_bytes, "tree_files": tree_files,
            "flags": flags, "counts": counts, "T": T}


def tree_top(parent, rep, stray_parent_is_root=False):
    """-> (top_rep int64[n], flags uint8[n], counts). stray_parent_is_root:
    the device call's rule for a parent outside [-1, n)"""
    parent = np.asarray(parent, np.int64)
    rep = np.asarray(rep, np.int64)
    n = rep.size
    if stray_parent_is_root:
        parent = np.where((parent < 0) | (parent >= n), -1, parent)
    part = (rep >= 0) & (rep < n)
    carriers = np.bincount(rep[part], minlength=n) if n else np.zeros(0, np.int64)
    dup = np.zeros(n, bool)
    dup[part] = carriers[rep[part]] >= 2
    nested = np.zeros(n, bool)
    has = dup & (parent >= 0)
    nested[has] = dup[parent[has]]
    loose = np.zeros(n, bool)  # per label: a carrier that is not nested
    loose[rep[dup & ~nested]] = True
    kept = np.zeros(n, bool)
    kept[dup] = loose[rep[dup]]
    top_rep = np.where(kept, rep, -1).astype(np.int64)
    flags = (dup * DUP + nested * NESTED).astype(np.uint8)
    classes = np.unique(rep[dup])
    counts = {"entries": int(part.sum()), "dup_entries": int(dup.sum()), "nested_entries": int(nested.sum()),
              "top_entries": int(kept.sum()), "kept_classes": int(loose[classes].sum()),
              "dropped_classes": int((~loose[classes]).sum())}
    return top_rep, flags, counts


def random_tree(n, seed, dir_share=0.3, max_depth=None):
    """entry i's parent is a random earlier directory (or none), then the
    entries are shuffled, so that children may stand before their parents"""
    rng = np.random.default_rng(seed)
    is_dir = (rng.random(n) < dir_share).astype(np.uint8)
    is_dir[0] = 1
    parent = np.full(n, -1, np.int64)
    depth = np.zeros(n, np.int64)
    dirs = [0]
    for i in range(1, n):
        p = dirs[int(rng.integers(0, len(dirs)))] if rng.random() > 0.01 else -1
        if p >= 0 and max_depth is not None and depth[p] + 1 >= max_depth:
            p = -1
        parent[i] = p
        depth[i] = depth[p] + 1 if p >= 0 else 0
        if is_dir[i]:
            dirs.append(i)
    perm = rng.permutation(n)  # new index of old entry i
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    new_parent = np.where(parent[inv] >= 0, perm[np.maximum(parent[inv], 0)], -1)
    return new_parent.astype(np.int64), is_dir[inv]
