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
