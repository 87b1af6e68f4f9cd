"""A family store that forgets rows, in plain Python, written from the definition
in include/sdcas.h ("family store: forget rows") and from nothing in the device
code or in spacedrive_amd/recipes.py: loops over rows and chunks, Python integers
reduced modulo 2^64, a bytearray for the store. keep, moves, the bytes, and the
store of the surviving files built from scratch to compare them with."""
import numpy as np

from tests import _family_recipes_ref as R
from tests import _family_store_ref as S

NONE32 = 0xFFFFFFFF
NONE = (1 << 64) - 1
M64 = NONE
KEEP_COUNTS = ("rows_kept", "rows_removed", "chunks_kept", "chunks_removed", "bytes_kept", "bytes_removed")
MOVES_COUNTS = ("moves", "literal_chunks", "moved_bytes", "lost_chunks", "lost_bytes", "longest_move")
KEEP_ARRAYS = ("row_new", "row_from", "family", "chunk_from", "chunk_file", "chunk_off", "chunk_len", "rep")
MOVE_ARRAYS = ("move_dst", "move_src", "move_len")

# the header's worked example: v1 = A B C, v2 = A B X C (tests/_family_recipes_ref.EXAMPLE) with v1 removed
EXAMPLE_KEEP = [0, 1]
EXAMPLE_OLD_AT = [0, 10, 60, 30]
EXAMPLE_MOVES = dict(move_dst=[0, 30, 35], move_src=[0, 60, 30], move_len=[30, 5, 30])
EXAMPLE_MOVES_COUNTS = dict(moves=3, literal_chunks=4, moved_bytes=65, lost_chunks=0, lost_bytes=0, longest_move=30)


def _ints(a, dtype):
    return [int(x) for x in np.asarray(a, dtype=dtype).reshape(-1)]


def keep(chunk_file, chunk_off, chunk_len, rep, family, keep):
    """-> dict of KEEP_ARRAYS and "counts" """
    fl, off, ln = _ints(chunk_file, np.uint32), _ints(chunk_off, np.uint64), _ints(chunk_len, np.uint64)
    rp, fam = _ints(rep, np.int64), _ints(family, np.int64)
    kp = [bool(x) for x in np.asarray(keep).reshape(-1)]
    m, n = len(fl), len(fam)
    row_new, row_from = [NONE32] * n, []
    for i in range(n):
        if kp[i]:
            row_new[i] = len(row_from)
            row_from.append(i)
    lowest_row = {}
    for i in row_from:
        if 0 <= fam[i] < n:
            lowest_row.setdefault(fam[i], i)
    out_family = [row_new[lowest_row[fam[i]]] if 0 <= fam[i] < n else -1 for i in row_from]
    chunk_from, chunk_new, lowest = [], {}, {}
    kept_bytes = removed_bytes = 0
    for c in range(m):
        if fl[c] < n and kp[fl[c]]:
            chunk_new[c] = len(chunk_from)
            chunk_from.append(c)
            lowest.setdefault(rp[c] if 0 <= rp[c] <= c else c, c)
            kept_bytes += ln[c]
        else:
            removed_bytes += ln[c]
    out_rep = [chunk_new[lowest[rp[c] if 0 <= rp[c] <= c else c]] for c in chunk_from]
    counts = dict(rows_kept=len(row_from), rows_removed=n - len(row_from), chunks_kept=len(chunk_from),
                  chunks_removed=m - len(chunk_from), bytes_kept=kept_bytes & M64, bytes_removed=removed_bytes & M64)
    return {"row_new": np.array(row_new, np.uint32), "row_from": np.array(row_from, np.uint32),
            "family": np.array(out_family, np.int64), "chunk_from": np.array(chunk_from, np.uint32),
            "chunk_file": np.array([row_new[fl[c]] for c in chunk_from], np.uint32),
            "chunk_off": np.array([off[c] for c in chunk_from], np.uint64),
            "chunk_len": np.array([ln[c] for c in chunk_from], np.uint64), "rep": np.array(out_rep, np.int64),
            "counts": counts}


def old_at(chunk_off, chunk_op, op_dst_off, op_store_off, ops, c):
    """where old chunk c's bytes lie in the old store, or NONE"""
    if c >= len(chunk_op):
        return NONE
    o = chunk_op[c]
    if o == NONE32 or o >= ops or op_store_off[o] == NONE or chunk_off[c] < op_dst_off[o]:
        return NONE
    return (op_store_off[o] + (chunk_off[c] - op_dst_off[o])) & M64


def moves(old, new, ops=None, new_ops=None, new_chunks=None):
    """old: chunk_off, chunk_op, op_dst_off, op_store_off; new: chunk_from,
    chunk_off, chunk_len, chunk_op, op_chunk, op_src_chunk, op_dst_off,
    op_store_off. ops / new_ops / new_chunks cap what is looked at. -> dict of
    MOVE_ARRAYS, "counts" and "old_at" (per new chunk, NONE where it has none
    or is no literal)"""
    coff, cop = _ints(old["chunk_off"], np.uint64), _ints(old["chunk_op"], np.uint32)
    odst, ooff = _ints(old["op_dst_off"], np.uint64), _ints(old["op_store_off"], np.uint64)
    k = len(odst) if ops is None else min(int(ops), len(odst))
    nfrom, noff = _ints(new["chunk_from"], np.uint32), _ints(new["chunk_off"], np.uint64)
    nlen, nop = _ints(new["chunk_len"], np.uint64), _ints(new["chunk_op"], np.uint32)
    noc, nosc = _ints(new["op_chunk"], np.uint32), _ints(new["op_src_chunk"], np.uint32)
    ndst, nso = _ints(new["op_dst_off"], np.uint64), _ints(new["op_store_off"], np.uint64)
    k2 = len(noc) if new_ops is None else min(int(new_ops), len(noc))
    m2 = len(nfrom) if new_chunks is None else min(int(new_chunks), len(nfrom))
    lit = [nop[c] < k2 and noc[nop[c]] == nosc[nop[c]] for c in range(m2)]
    at = [old_at(coff, cop, odst, ooff, k, nfrom[c]) if lit[c] else NONE for c in range(m2)]
    dst, src, ln = [], [], []
    lost = lost_bytes = 0
    for c in range(m2):
        if not lit[c]:
            continue
        if at[c] == NONE:
            lost, lost_bytes = lost + 1, lost_bytes + nlen[c]
            continue
        if c >= 1 and lit[c - 1] and nop[c - 1] == nop[c] and at[c - 1] != NONE and \
                at[c] == (at[c - 1] + nlen[c - 1]) & M64:
            ln[-1] = (ln[-1] + nlen[c]) & M64
            continue
        o = nop[c]
        dst.append((nso[o] + (noff[c] - ndst[o])) & M64)
        src.append(at[c])
        ln.append(nlen[c])
    counts = dict(moves=len(dst), literal_chunks=sum(lit), moved_bytes=sum(ln) & M64, lost_chunks=lost,
                  lost_bytes=lost_bytes & M64, longest_move=max(ln, default=0))
    return {"move_dst": np.array(dst, np.uint64), "move_src": np.array(src, np.uint64),
            "move_len": np.array(ln, np.uint64), "counts": counts, "old_at": at}


def apply(mv, old_store, store_bytes):
    """the new store: every move's bytes carried out of place"""
    new = bytearray(int(store_bytes))
    for d, s, n in zip(_ints(mv["move_dst"], np.uint64), _ints(mv["move_src"], np.uint64),
                       _ints(mv["move_len"], np.uint64)):
        assert d + n <= len(new) and s + n <= len(old_store)
        new[d:d + n] = old_store[s:s + n]
    return new


def old_side(rec, lay, chunk_off):
    return dict(chunk_off=chunk_off, chunk_op=rec["chunk_op"], op_dst_off=rec["op_dst_off"],
                op_store_off=lay["op_store_off"])


def new_side(kept, rec, lay):
    return dict(chunk_from=kept["chunk_from"], chunk_off=kept["chunk_off"], chunk_len=kept["chunk_len"],
                chunk_op=rec["chunk_op"], op_chunk=rec["op_chunk"], op_src_chunk=rec["op_src_chunk"],
                op_dst_off=rec["op_dst_off"], op_store_off=lay["op_store_off"])


def from_scratch(contents, chunk_file, chunk_off, chunk_len, family, keep):
    """The store of the surviving files alone, computed without the old one: the
    survivors' chunk arrays, rep as confirm gives it over their bytes (the lowest
    chunk with the same bytes), the labels renumbered by hand -> (contents',
    recipes, layout, store)"""
    fl, off, ln = _ints(chunk_file, np.uint32), _ints(chunk_off, np.uint64), _ints(chunk_len, np.uint64)
    fam = _ints(family, np.int64)
    n = len(fam)
    rows = [i for i in range(n) if keep[i]]
    new = {i: j for j, i in enumerate(rows)}
    lowest = {}
    for i in rows:
        if 0 <= fam[i] < n:
            lowest.setdefault(fam[i], new[i])
    family2 = [lowest[fam[i]] if 0 <= fam[i] < n else -1 for i in rows]
    file2, off2, len2, rep2, seen = [], [], [], [], {}
    for c in range(len(fl)):
        if fl[c] < n and keep[fl[c]]:
            data = contents[fl[c]][off[c]:off[c] + ln[c]]
            rep2.append(seen.setdefault(data, len(rep2)))
            file2.append(new[fl[c]]), off2.append(off[c]), len2.append(ln[c])
    contents2 = [contents[i] for i in rows]
    rec = R.family_recipes(file2, off2, len2, rep2, family2)
    lay = S.layout(rec)
    return contents2, rec, lay, S.pack_all(rec, lay, contents2)


def masks(seed, family):
    """the keep masks of the tests over one corpus: random ones, all, none, the
    first row of every family removed, a whole family removed, only the strays"""
    fam = _ints(family, np.int64)
    n = len(fam)
    rng = np.random.default_rng(1000 + seed)
    part = [0 <= f < n for f in fam]
    heads = sorted({f for f, p in zip(fam, part) if p})
    out = [("random", (rng.random(n) < 0.6).tolist()), ("tenth", (rng.random(n) < 0.9).tolist()),
           ("all", [True] * n), ("none", [False] * n),
           ("firsts", [not (part[i] and fam[i] == i) for i in range(n)]),
           ("family", [not (part[i] and fam[i] == heads[seed % len(heads)]) for i in range(n)]),
           ("strays", [not p for p in part])]
    return [(name, np.array(mask, np.uint8)) for name, mask in out]
