"""Plain Python / numpy reference of the file families (include/sdcas.h, "file
families"): a dict for id -> row, the slot classes with Python
integers (so no product wraps), a sequential union-find and the counts. The
checker of tests/test_gpu_file_families.py and tests/test_gpu_similar_families.py;
tests/test_families_ref.py checks it against a breadth-first search."""
import numpy as np

COUNTS = ("files", "slots", "missing", "self_slots", "weak", "links", "families", "members", "largest", "unsorted")
MISSING, SELF, WEAK, LINK = "missing", "self", "weak", "link"


def passes(b, size_i, size_j, num, den):
    """the threshold, exactly: Python integers do not wrap"""
    return int(b) > 0 and int(b) * int(den) >= int(num) * max(int(size_i), int(size_j))


def classify(row_of, ids, sizes, i, f, b, num, den):
    """the class of slot (i, .) that names file id f with b bytes -> (class, row of f or None)"""
    j = row_of.get(int(f))
    if j is None:
        return MISSING, None
    if int(f) == int(ids[i]):
        return SELF, j
    return (LINK if passes(b, sizes[i], sizes[j], num, den) else WEAK), j


def is_sorted(ids):
    ids = [int(x) for x in ids]
    return all(a < b for a, b in zip(ids, ids[1:]))


def families(ids, sizes, peer_count, peers, peer_bytes, num=1, den=2):
    """-> dict: "family" int64[n], "family_size" uint32[n], "counts" (the device
    form's: unsorted ids give the trivial rows and unsorted = 1)"""
    ids, sizes = np.asarray(ids, np.uint64), np.asarray(sizes, np.uint64)
    n = ids.size
    peers, peer_bytes = np.asarray(peers, np.uint64), np.asarray(peer_bytes, np.uint64)
    k = peers.shape[1] if peers.ndim == 2 else peers.size // max(n, 1)
    peers, peer_bytes = peers.reshape(n, k), peer_bytes.reshape(n, k)
    assert k >= 1 and int(den) >= 1 and 0 <= int(num) <= int(den)
    counts = dict.fromkeys(COUNTS, 0)
    counts["files"] = n
    if not is_sorted(ids):
        counts["unsorted"] = 1
        return {"family": np.arange(n, dtype=np.int64), "family_size": np.ones(n, np.uint32), "counts": counts}
    id_list, size_list = [int(x) for x in ids], [int(x) for x in sizes]
    row_of = {f: i for i, f in enumerate(id_list)}
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    tally = {MISSING: 0, SELF: 0, WEAK: 0, LINK: 0}
    pl, bl = peers.tolist(), peer_bytes.tolist()
    for i in range(n):
        for s in range(min(int(peer_count[i]), k)):
            counts["slots"] += 1
            cls, j = classify(row_of, id_list, size_list, i, pl[i][s], bl[i][s], num, den)
            tally[cls] += 1
            if cls == LINK:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    counts.update(missing=tally[MISSING], self_slots=tally[SELF], weak=tally[WEAK], links=tally[LINK])
    family = np.array([find(i) for i in range(n)], np.int64)
    size = np.bincount(family, minlength=n) if n else np.zeros(0, np.int64)
    fsize = size[family].astype(np.uint32)
    roots = size[size >= 2]
    counts.update(families=int(roots.size), members=int(roots.sum()), largest=int(roots.max()) if roots.size else 0)
    return {"family": family, "family_size": fsize, "counts": counts}


def sets_of(family):
    """duplicate_sets(family, None, SDCAS_SETS_BY_REP)'s answer: the families of
    two rows or more by lowest member -> (set_rep int64[S], set_offsets uint64[S + 1], members int64[M])"""
    family = np.asarray(family, np.int64)
    n = family.size
    size = np.bincount(family, minlength=n) if n else np.zeros(0, np.int64)
    set_rep = np.flatnonzero(size >= 2).astype(np.int64)
    keep = np.flatnonzero(size[family] >= 2) if n else np.zeros(0, np.int64)
    members = keep[np.argsort(family[keep], kind="stable")].astype(np.int64)
    set_offsets = np.concatenate([[0], np.cumsum(size[set_rep])]).astype(np.uint64)
    return set_rep, set_offsets, members


def same(got, want):
    return all(np.array_equal(np.asarray(got[key]), want[key]) and np.asarray(got[key]).dtype == want[key].dtype
               for key in ("family", "family_size")) and got["counts"] == want["counts"]
