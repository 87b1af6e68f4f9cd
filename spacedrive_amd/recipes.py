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
