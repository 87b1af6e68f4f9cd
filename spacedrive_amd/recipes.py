"""Apply family recipes (include/sdcas.h, "family recipes") on the host, with no
GPU: every file comes back from the literal ranges alone."""
import bisect

import numpy as np


def rebuild_files(recipes, read):
    """Rebuild every row from what its family stores. `recipes` is
    Engine.family_recipes' dict (or the "recipes" of family_recipes_of /
    similar_recipes); `read(row, off, len) -> bytes` gives len bytes of row at
    off and is called for LITERAL ops only, once each: together they are the
    store. A copy op is served from those bytes; ValueError when its source
    range is not covered by literal ops of its source row (recipes have depth
    one), or when read returns another number of bytes. -> {row: bytes} for
    every row that has an op, and b"" for the other rows of "row_ops" when the
    dict has it. Ops of a row land at their dst_off; bytes no op covers are 0."""
    row, src_row = np.asarray(recipes["op_row"]), np.asarray(recipes["op_src_row"])
    dst, src = np.asarray(recipes["op_dst_off"]), np.asarray(recipes["op_src_off"])
    ln = np.asarray(recipes["op_len"])
    if "op_literal" in recipes:
        lit = np.asarray(recipes["op_literal"], bool)
    else:
        lit = np.asarray(recipes["op_chunk"]) == np.asarray(recipes["op_src_chunk"])
    k = row.size
    if not all(a.size == k for a in (src_row, dst, src, ln, lit)):
        raise ValueError("rebuild_files: the op arrays differ in length")
    # the store: per row the literal ranges, merged where they touch or overlap
    store = {}
    for o in np.flatnonzero(lit):
        r, at, n = int(row[o]), int(dst[o]), int(ln[o])
        data = bytes(read(r, at, n))
        if len(data) != n:
            raise ValueError(f"rebuild_files: read({r}, {at}, {n}) returned {len(data)} bytes")
        store.setdefault(r, []).append((at, data))
    starts = {}
    for r, parts in store.items():
        parts.sort(key=lambda p: p[0])
        merged = []
        for at, data in parts:
            if merged and at <= merged[-1][0] + len(merged[-1][1]):
                m_at, m_data = merged[-1]
                keep = at - m_at
                if keep + len(data) > len(m_data):
                    m_data[keep:] = data
            else:
                merged.append((at, bytearray(data)))
        store[r] = merged
        starts[r] = [at for at, _ in merged]
    size = {}
    for o in range(k):
        r = int(row[o])
        size[r] = max(size.get(r, 0), int(dst[o]) + int(ln[o]))
    out = {r: bytearray(n) for r, n in size.items()}
    for o in range(k):
        r, at, n = int(row[o]), int(dst[o]), int(ln[o])
        sr, sat = int(src_row[o]), int(src[o])
        if n == 0:
            continue
        i = bisect.bisect_right(starts.get(sr, []), sat) - 1
        seg = store[sr][i] if i >= 0 else None
        if seg is None or sat + n > seg[0] + len(seg[1]):
            raise ValueError(f"rebuild_files: op {o} reads [{sat}, {sat + n}) of row {sr}, which literal ops do not cover")
        out[r][at:at + n] = seg[1][sat - seg[0]:sat - seg[0] + n]
    done = {r: bytes(b) for r, b in out.items()}
    if "row_ops" in recipes:
        for r in range(np.asarray(recipes["row_ops"]).size):
            done.setdefault(r, b"")
    return done


STORE_NONE = 0xFFFFFFFFFFFFFFFF  # SDCAS_STORE_NONE: an op without a place in the store


def _ops(recipes):
    u32 = [np.asarray(recipes[k], np.uint32) for k in ("op_chunk", "op_src_chunk", "op_row", "op_src_row")]
    u64 = [np.asarray(recipes[k], np.uint64) for k in ("op_dst_off", "op_src_off", "op_len")]
    k = u32[0].size
    if not all(a.size == k for a in u32 + u64):
        raise ValueError("the op arrays differ in length")
    return u32 + u64


def store_layout(recipes):
    """sdcas_family_store_layout on the host (include/sdcas.h, "family store"):
    where every op's bytes live in the dense store of the literal ranges. ->
    {"op_store_off": uint64[ops] (STORE_NONE for an uncovered copy), "counts":
    sdcas_family_store_counts' six fields}. Arithmetic is modulo 2^64."""
    oc, osc, row, srow, dst, src, ln = _ops(recipes)
    chunk_op = np.asarray(recipes["chunk_op"], np.uint32)
    k, m = oc.size, chunk_op.size
    lit = oc == osc
    lit_len = np.where(lit, ln, np.uint64(0)).astype(np.uint64)
    before = np.cumsum(lit_len, dtype=np.uint64) - lit_len
    off = np.full(k, STORE_NONE, np.uint64)
    off[lit] = before[lit]
    # a copy's literal op, through its source chunk
    ok = ~lit & (osc < m)
    L = np.zeros(k, np.int64)
    if m:
        L[ok] = chunk_op[osc[ok]]
    ok &= L < k
    Ls = np.where(ok, L, 0)
    if k:
        ok &= lit[Ls] & (row[Ls] == srow) & (src >= dst[Ls])
        d = src - dst[Ls]
        ok &= d <= ln[Ls]
        ok &= ln <= ln[Ls] - np.where(ok, d, np.uint64(0))
        at = off[Ls] + d
        ok &= at != np.uint64(STORE_NONE)
        off[ok] = at[ok]
    unc = ~lit & ~ok
    counts = {"ops": k, "literal_ops": int(lit.sum()), "copy_ops": int((~lit).sum()), "uncovered_ops": int(unc.sum()),
              "store_bytes": int(lit_len.sum(dtype=np.uint64)) if k else 0,
              "uncovered_bytes": int(ln[unc].sum(dtype=np.uint64)) if k else 0}
    return {"op_store_off": off, "counts": counts}


def pack_store(recipes, layout, read):
    """The store of `layout`, filled on the host: `read(row, off, len) -> bytes`
    is called once for every literal op, as rebuild_files calls it. -> uint8
    array of store_bytes. ValueError when read returns another number of bytes
    or an op's place is not inside the store."""
    oc, osc, row, _, dst, _, ln = _ops(recipes)
    off = np.asarray(layout["op_store_off"], np.uint64)
    if off.size != oc.size:
        raise ValueError("pack_store: the layout is of other recipes")
    store = np.zeros(int(layout["counts"]["store_bytes"]), np.uint8)
    for o in np.flatnonzero((oc == osc) & (off != np.uint64(STORE_NONE))):
        r, at, n, so = int(row[o]), int(dst[o]), int(ln[o]), int(off[o])
        if so + n > store.size:
            raise ValueError(f"pack_store: op {o} lies at [{so}, {so + n}) of a store of {store.size} bytes")
        data = bytes(read(r, at, n))
        if len(data) != n:
            raise ValueError(f"pack_store: read({r}, {at}, {n}) returned {len(data)} bytes")
        store[so:so + n] = np.frombuffer(data, np.uint8)
    return store


def restore_from_store(recipes, layout, store, rows=None):
    """Every row (or the rows named) from the store alone -> {row: bytes}, as
    rebuild_files gives them: ops land at their dst_off, bytes no op covers
    are 0, a row without ops is b"". ValueError for an uncovered op of a wanted
    row or a place outside the store."""
    _, _, row, _, dst, _, ln = _ops(recipes)
    off = np.asarray(layout["op_store_off"], np.uint64)
    store = np.asarray(store, np.uint8)
    if off.size != row.size:
        raise ValueError("restore_from_store: the layout is of other recipes")
    want = None if rows is None else {int(r) for r in rows}
    sel = np.arange(row.size) if want is None else np.flatnonzero(np.isin(row, sorted(want)))
    size = {}
    for o in sel:
        r = int(row[o])
        size[r] = max(size.get(r, 0), int(dst[o]) + int(ln[o]))
    out = {r: bytearray(n) for r, n in size.items()}
    for o in sel:
        r, at, n, so = int(row[o]), int(dst[o]), int(ln[o]), int(off[o])
        if so == STORE_NONE:
            raise ValueError(f"restore_from_store: op {o} of row {r} has no place in the store")
        if so + n > store.size:
            raise ValueError(f"restore_from_store: op {o} reads [{so}, {so + n}) of a store of {store.size} bytes")
        out[r][at:at + n] = store[so:so + n].tobytes()
    done = {r: bytes(b) for r, b in out.items()}
    if want is not None:
        for r in want:
            done.setdefault(r, b"")
    elif "row_ops" in recipes:
        for r in range(np.asarray(recipes["row_ops"]).size):
            done.setdefault(r, b"")
    return done


_NO32 = 0xFFFFFFFF


def keep_chunks(chunk_file, chunk_off, chunk_len, rep, family, keep):
    """sdcas_family_chunks_keep on the host (include/sdcas.h, "family store:
    forget rows"): the chunk arrays of the rows with keep != 0, rows and chunks
    renumbered densely, classes and labels elected again among the survivors. ->
    {"row_new": uint32[n] (0xFFFFFFFF: removed), "row_from": uint32[n'],
    "family": int64[n'], "chunk_from": uint32[m'], "chunk_file": uint32[m'],
    "chunk_off", "chunk_len": uint64[m'], "rep": int64[m'], "counts":
    sdcas_family_keep_counts' six fields}. The outputs are valid inputs of the
    recipes and of another keep."""
    fl, off = np.asarray(chunk_file, np.uint32).reshape(-1), np.asarray(chunk_off, np.uint64).reshape(-1)
    ln, rp = np.asarray(chunk_len, np.uint64).reshape(-1), np.asarray(rep, np.int64).reshape(-1)
    fam, kp = np.asarray(family, np.int64).reshape(-1), np.asarray(keep).reshape(-1) != 0
    m, n = fl.size, fam.size
    if off.size != m or ln.size != m or rp.size != m:
        raise ValueError(f"keep_chunks: {m} chunk files, {off.size} offsets, {ln.size} lengths, {rp.size} reps")
    if kp.size != n:
        raise ValueError(f"keep_chunks: {n} labels, {kp.size} keep flags")
    row_from = np.flatnonzero(kp)
    row_new = np.full(n, _NO32, np.uint32)
    row_new[row_from] = np.arange(row_from.size, dtype=np.uint32)
    # a label's lowest kept row that takes part
    part = kp & (fam >= 0) & (fam < n)
    low = np.full(n, n, np.int64)
    rows = np.flatnonzero(part)
    np.minimum.at(low, fam[rows], rows)
    out_family = np.full(row_from.size, -1, np.int64)
    sel = part[row_from]
    out_family[sel] = row_new[low[fam[row_from[sel]]]]
    # the chunks of the kept rows
    sv = fl < n
    sv[sv] = kp[fl[sv]]
    chunk_from = np.flatnonzero(sv)
    chunk_new = np.full(m, -1, np.int64)
    chunk_new[chunk_from] = np.arange(chunk_from.size)
    pos = np.arange(m, dtype=np.int64)
    r = np.where((rp >= 0) & (rp <= pos), rp, pos)
    lowc = np.full(m, m, np.int64)
    np.minimum.at(lowc, r[chunk_from], chunk_from)
    counts = {"rows_kept": int(row_from.size), "rows_removed": int(n - row_from.size),
              "chunks_kept": int(chunk_from.size), "chunks_removed": int(m - chunk_from.size),
              "bytes_kept": int(ln[sv].sum(dtype=np.uint64)) if m else 0,
              "bytes_removed": int(ln[~sv].sum(dtype=np.uint64)) if m else 0}
    return {"row_new": row_new, "row_from": row_from.astype(np.uint32), "family": out_family,
            "chunk_from": chunk_from.astype(np.uint32), "chunk_file": row_new[fl[chunk_from]],
            "chunk_off": off[chunk_from], "chunk_len": ln[chunk_from],
            "rep": chunk_new[lowc[r[chunk_from]]].astype(np.int64), "counts": counts}


def store_moves(old_recipes, old_layout, new_recipes, new_layout, chunk_from, chunk_len):
    """sdcas_family_store_moves on the host: where the literal chunks of the new
    recipes lie in the old store, neighbours merged into ranges. The recipes
    carry "chunk_off" and "chunk_op" (Engine.family_recipes' dicts); chunk_from
    and chunk_len are keep_chunks' over the new chunks. -> {"move_dst",
    "move_src", "move_len": uint64[moves], "counts": sdcas_family_moves_counts'
    six fields}. A literal chunk without a place in the old store gets no move
    and is counted as lost."""
    coff, cop = np.asarray(old_recipes["chunk_off"], np.uint64), np.asarray(old_recipes["chunk_op"], np.uint32)
    odst, ooff = np.asarray(old_recipes["op_dst_off"], np.uint64), np.asarray(old_layout["op_store_off"], np.uint64)
    nfrom, nlen = np.asarray(chunk_from, np.uint32).reshape(-1), np.asarray(chunk_len, np.uint64).reshape(-1)
    noff, nop = np.asarray(new_recipes["chunk_off"], np.uint64), np.asarray(new_recipes["chunk_op"], np.uint32)
    noc, nosc = np.asarray(new_recipes["op_chunk"], np.uint32), np.asarray(new_recipes["op_src_chunk"], np.uint32)
    ndst, nso = np.asarray(new_recipes["op_dst_off"], np.uint64), np.asarray(new_layout["op_store_off"], np.uint64)
    m, k, m2, k2 = coff.size, odst.size, nfrom.size, noc.size
    if cop.size != m or ooff.size != k:
        raise ValueError("store_moves: the old layout is of other recipes")
    if nlen.size != m2 or noff.size != m2 or nop.size != m2 or nosc.size != k2 or ndst.size != k2 or nso.size != k2:
        raise ValueError("store_moves: the new arrays differ in length")
    none = np.uint64(STORE_NONE)
    z64, z32 = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    # old_at
    ok = nfrom < m
    c = np.where(ok, nfrom, 0).astype(np.int64)
    o = (cop if m else z32)[c]
    ok &= o < k
    o = np.where(ok, o, 0).astype(np.int64)
    so, d, at_file = (ooff if k else z64)[o], (odst if k else z64)[o], (coff if m else z64)[c]
    ok &= (so != none) & (at_file >= d)
    at = so + (at_file - d)
    ok &= at != none
    # the literal chunks and their places in the new store
    lit = nop < k2
    o2 = np.where(lit, nop, 0).astype(np.int64)
    lit &= (noc if k2 else z32)[o2] == (nosc if k2 else z32)[o2]
    new_at = (nso if k2 else z64)[o2] + (noff - (ndst if k2 else z64)[o2])
    has = lit & ok
    cont = np.zeros(m2, bool)
    if m2 > 1:
        cont[1:] = has[1:] & has[:-1] & (nop[1:] == nop[:-1]) & (at[1:] == at[:-1] + nlen[:-1])
    head = has & ~cont
    move = np.cumsum(head) - 1
    moves = int(head.sum())
    move_len = np.zeros(moves, np.uint64)
    np.add.at(move_len, move[has], nlen[has])
    lost = lit & ~ok
    counts = {"moves": moves, "literal_chunks": int(lit.sum()),
              "moved_bytes": int(move_len.sum(dtype=np.uint64)) if moves else 0, "lost_chunks": int(lost.sum()),
              "lost_bytes": int(nlen[lost].sum(dtype=np.uint64)) if m2 else 0,
              "longest_move": int(move_len.max()) if moves else 0}
    return {"move_dst": new_at[head], "move_src": at[head], "move_len": move_len, "counts": counts}


def apply_moves(moves, old_store, store_bytes=None):
    """The new store: every move's bytes from the old one, out of place ->
    uint8[store_bytes] (None: up to the last move's end; the moves of a
    removal cover the new store). ValueError for a move outside either."""
    dst, src = np.asarray(moves["move_dst"], np.uint64), np.asarray(moves["move_src"], np.uint64)
    ln = np.asarray(moves["move_len"], np.uint64)
    old = np.asarray(old_store, np.uint8).reshape(-1)
    if store_bytes is None:
        store_bytes = max((int(d) + int(n) for d, n in zip(dst, ln)), default=0)
    new = np.zeros(int(store_bytes), np.uint8)
    for d, s, n in zip(dst, src, ln):
        d, s, n = int(d), int(s), int(n)
        if d + n > new.size or s + n > old.size:
            raise ValueError(f"apply_moves: a move of {n} bytes from {s} to {d} leaves a store ({old.size} -> {new.size})")
        new[d:d + n] = old[s:s + n]
    return new
