"""The family bytes in plain Python, written from the definition in
include/sdcas.h and from nothing in the device code: dicts keyed by the class
(label, class number), Python integers reduced modulo 2^64 at the end."""
import numpy as np

COUNTS = ("files", "chunks", "classes", "total_bytes", "stored_bytes", "sets", "members", "set_reclaimable_bytes",
          "largest_reclaimable")
ROWS = ("file_bytes", "delta_bytes", "self_bytes", "inherited_bytes")
SETS = ("set_rep", "set_files", "set_total", "set_stored")
M64 = (1 << 64) - 1

# the worked example of the header
EXAMPLE = dict(chunk_file=[0, 0, 1, 1, 2, 3, 3], chunk_len=[10, 10, 10, 5, 10, 5, 7], rep=[0, 0, 0, 3, 0, 3, 6],
               family=[0, 0, 2, 0])
EXAMPLE_ROWS = dict(file_bytes=[20, 15, 10, 12], delta_bytes=[10, 5, 10, 7], self_bytes=[10, 0, 0, 0],
                    inherited_bytes=[0, 10, 0, 5])
EXAMPLE_SETS = dict(set_rep=[0], set_files=[3], set_total=[47], set_stored=[22])
EXAMPLE_COUNTS = dict(files=4, chunks=7, classes=4, total_bytes=57, stored_bytes=32, sets=1, members=3,
                      set_reclaimable_bytes=25, largest_reclaimable=25)


def family_bytes(chunk_file, chunk_len, rep, family):
    """-> dict: the four per-row arrays uint64[n], "set_rep" int64[S], "set_files"
    uint32[S], "set_total", "set_stored", "set_reclaimable" uint64[S], "counts"."""
    chunk_file = [int(x) for x in np.asarray(chunk_file).reshape(-1)]
    chunk_len = [int(x) for x in np.asarray(chunk_len, dtype=np.uint64).reshape(-1)]
    rep = [int(x) for x in np.asarray(rep, dtype=np.int64).reshape(-1)]
    family = [int(x) for x in np.asarray(family, dtype=np.int64).reshape(-1)]
    m, n = len(chunk_file), len(family)
    label = {i: family[i] for i in range(n) if 0 <= family[i] < n}
    rows = {name: [0] * n for name in ROWS}
    first = {}  # class -> its lowest participating chunk
    chunks = 0
    for c in range(m):
        f = chunk_file[c]
        if f >= n or f not in label:
            continue
        chunks += 1
        cls = (label[f], rep[c] if 0 <= rep[c] <= c else c)
        rows["file_bytes"][f] += chunk_len[c]
        if cls not in first:
            first[cls] = c
            rows["delta_bytes"][f] += chunk_len[c]
        elif chunk_file[first[cls]] == f:
            rows["self_bytes"][f] += chunk_len[c]
        else:
            rows["inherited_bytes"][f] += chunk_len[c]
    per = {}  # label -> [total, stored, rows, lowest row]
    for i in sorted(label):
        p = per.setdefault(label[i], [0, 0, 0, i])
        p[0] += rows["file_bytes"][i]
        p[1] += rows["delta_bytes"][i]
        p[2] += 1
    sets = [(((p[0] - p[1]) & M64), p[3], p[2], p[0] & M64, p[1] & M64) for p in per.values() if p[2] >= 2]
    sets.sort(key=lambda s: (-s[0], s[1]))
    counts = dict(files=len(label), chunks=chunks, classes=len(first),
                  total_bytes=sum(rows["file_bytes"]) & M64, stored_bytes=sum(rows["delta_bytes"]) & M64,
                  sets=len(sets), members=sum(s[2] for s in sets),
                  set_reclaimable_bytes=sum(s[0] for s in sets) & M64,
                  largest_reclaimable=max((s[0] for s in sets), default=0))
    out = {name: np.array([v & M64 for v in rows[name]], dtype=np.uint64) for name in ROWS}
    out["set_rep"] = np.array([s[1] for s in sets], dtype=np.int64)
    out["set_files"] = np.array([s[2] for s in sets], dtype=np.uint32)
    out["set_total"] = np.array([s[3] for s in sets], dtype=np.uint64)
    out["set_stored"] = np.array([s[4] for s in sets], dtype=np.uint64)
    out["set_reclaimable"] = np.array([s[0] for s in sets], dtype=np.uint64)
    out["counts"] = counts
    return out


def members_of(family, set_rep):
    """(set_offsets uint64[S + 1], members int64[M]): the rows of each set, ascending, in set_rep's order"""
    family = [int(x) for x in np.asarray(family, dtype=np.int64).reshape(-1)]
    n = len(family)
    rows = {}  # label -> its participating rows, ascending
    for i in range(n):
        if 0 <= family[i] < n:
            rows.setdefault(family[i], []).append(i)
    offs, members = [0], []
    for r in set_rep:
        members += rows[family[int(r)]]
        offs.append(len(members))
    return np.array(offs, dtype=np.uint64), np.array(members, dtype=np.int64)


def brute_force(chunk_file, chunk_len, rep, family):
    """the per-row sums and the class count by the definition read literally, O(m^2):
    for every chunk, look through all earlier chunks for one of its class"""
    chunk_file = [int(x) for x in chunk_file]
    chunk_len = [int(x) for x in chunk_len]
    rep = [int(x) for x in rep]
    family = [int(x) for x in family]
    m, n = len(chunk_file), len(family)

    def part(c):
        return chunk_file[c] < n and 0 <= family[chunk_file[c]] < n

    def cls(c):
        return (family[chunk_file[c]], rep[c] if 0 <= rep[c] <= c else c)

    rows = {name: [0] * n for name in ROWS}
    classes = 0
    for c in range(m):
        if not part(c):
            continue
        f = chunk_file[c]
        rows["file_bytes"][f] += chunk_len[c]
        earlier = [d for d in range(c) if part(d) and cls(d) == cls(c)]
        if not earlier:
            classes += 1
            rows["delta_bytes"][f] += chunk_len[c]
        elif chunk_file[earlier[0]] == f:
            rows["self_bytes"][f] += chunk_len[c]
        else:
            rows["inherited_bytes"][f] += chunk_len[c]
    return {name: [v & M64 for v in rows[name]] for name in ROWS}, classes


def sharing(chunk_file, chunk_len, rep, n_files):
    """chunk_sharing's new / self / other bytes per file and its stored bytes, for
    confirm-style reps with every chunk taking part (law 1's right-hand side)"""
    new, own, other = [0] * n_files, [0] * n_files, [0] * n_files
    for c, (f, ln, r) in enumerate(zip(chunk_file, chunk_len, rep)):
        f, ln, r = int(f), int(ln), int(r)
        if r == c:
            new[f] += ln
        elif int(chunk_file[r]) == f:
            own[f] += ln
        else:
            other[f] += ln
    return [v & M64 for v in new], [v & M64 for v in own], [v & M64 for v in other], sum(new) & M64
