"""The family store in plain Python, written from the definition in
include/sdcas.h ("family store") and from nothing in the device code or in
spacedrive_amd/recipes.py: one loop over the ops, Python integers reduced modulo
2^64, bytearrays for the blob and the store. Layout, pack and restore, with
windows, bad ops and uncovered ops."""
import numpy as np

NONE = (1 << 64) - 1
M64 = NONE
LAYOUT_COUNTS = ("ops", "literal_ops", "copy_ops", "uncovered_ops", "store_bytes", "uncovered_bytes")
MOVE_COUNTS = ("ops_moved", "bytes_moved", "bad_ops", "tiles")
OPS = ("op_chunk", "op_src_chunk", "op_row", "op_src_row", "op_dst_off", "op_src_off", "op_len")

# the header's worked example (tests/_family_recipes_ref.EXAMPLE): v1 = A B C, v2 = A B X C
EXAMPLE_STORE_OFF = [0, 0, 60, 30]
EXAMPLE_STORE_BYTES = 65


def _ops(rec):
    return [[int(x) for x in np.asarray(rec[name], dtype=np.uint64).reshape(-1)] for name in OPS]


def layout(rec, ops=None):
    """-> {"op_store_off": uint64[ops], "counts"}; `ops` caps the ops looked at"""
    oc, osc, row, srow, dst, src, ln = _ops(rec)
    chunk_op = [int(x) for x in np.asarray(rec["chunk_op"], dtype=np.uint64).reshape(-1)]
    k = len(oc) if ops is None else min(int(ops), len(oc))
    m = len(chunk_op)
    off, run, nlit = [NONE] * k, 0, 0
    for o in range(k):
        if oc[o] == osc[o]:
            off[o] = run & M64
            run += ln[o]
            nlit += 1
    unc_ops = unc_bytes = 0
    for o in range(k):
        if oc[o] == osc[o]:
            continue
        s = osc[o]
        if s < m:
            L = chunk_op[s]
            if L < k and oc[L] == osc[L] and row[L] == srow[o] and src[o] >= dst[L]:
                d = src[o] - dst[L]
                if d <= ln[L] and ln[o] <= ln[L] - d:
                    off[o] = (off[L] + d) & M64
        if off[o] == NONE:
            unc_ops += 1
            unc_bytes += ln[o]
    counts = dict(ops=k, literal_ops=nlit, copy_ops=k - nlit, uncovered_ops=unc_ops, store_bytes=run & M64,
                  uncovered_bytes=unc_bytes & M64)
    return {"op_store_off": np.array(off, dtype=np.uint64), "counts": counts}


def tiles_of(addr, nbytes, tile):
    """a clipped op of nbytes to destination offset addr, cut at 16-byte aligned destination addresses"""
    return (addr % 16 + nbytes + tile - 1) // tile if nbytes else 0


def move(rec, store_off, row_at, row_base, row_len, blob, store, restore, tile, blob_bytes=None, store_bytes=None,
         ops=None):
    """pack (restore False: blob -> store, literal ops) or restore (store ->
    blob, every op with an offset) in place on the bytearrays -> counts"""
    oc, osc, row, _, dst, _, ln = _ops(rec)
    u64 = lambda a: [int(x) for x in np.asarray(a, dtype=np.uint64).reshape(-1)]
    off, at, rl = u64(store_off), u64(row_at), u64(row_len)
    base = [0] * len(at) if row_base is None else u64(row_base)
    blob_bytes = len(blob) if blob_bytes is None else blob_bytes
    store_bytes = len(store) if store_bytes is None else store_bytes
    k = len(oc) if ops is None else min(int(ops), len(oc))
    moved = nbytes = bad = tiles = 0
    for o in range(k):
        if off[o] == NONE or not (restore or oc[o] == osc[o]):
            continue
        r = row[o]
        if r >= len(at) or dst[o] + ln[o] > M64 or off[o] > store_bytes or ln[o] > store_bytes - off[o]:
            bad += 1
            continue
        if rl[r] == 0:
            continue
        if at[r] > blob_bytes or rl[r] > blob_bytes - at[r] or base[r] + rl[r] > M64:
            bad += 1
            continue
        lo, hi = max(dst[o], base[r]), min(dst[o] + ln[o], base[r] + rl[r])
        if hi <= lo:
            continue
        b, s, n = at[r] + (lo - base[r]), off[o] + (lo - dst[o]), hi - lo
        if restore:
            blob[b:b + n] = store[s:s + n]
        else:
            store[s:s + n] = blob[b:b + n]
        moved, nbytes, tiles = moved + 1, nbytes + n, tiles + tiles_of(b if restore else s, n, tile)
    return dict(ops_moved=moved, bytes_moved=nbytes, bad_ops=bad, tiles=tiles)


def whole_rows(contents, rows=None, gap=0, align=1):
    """every row (or the rows named) whole in one blob -> (blob bytearray, row_at, row_len)"""
    n = len(contents)
    at, ln, blob = [0] * n, [0] * n, bytearray()
    for r in (range(n) if rows is None else rows):
        blob += bytes(-len(blob) % align)
        at[r], ln[r] = len(blob), len(contents[r])
        blob += contents[r] + bytes(gap)
    return blob, np.array(at, np.uint64), np.array(ln, np.uint64)


def pack_all(rec, lay, contents, tile=8192):
    """the store of the whole corpus"""
    blob, at, ln = whole_rows(contents)
    store = bytearray(lay["counts"]["store_bytes"])
    move(rec, lay["op_store_off"], at, None, ln, blob, store, False, tile)
    return store


def restore_all(rec, lay, store, sizes, tile=8192):
    """-> {row: bytes} for every row, from the store alone"""
    blob, at, ln = whole_rows([bytes(int(s)) for s in sizes])
    move(rec, lay["op_store_off"], at, None, ln, blob, store, True, tile)
    return {r: bytes(blob[int(at[r]):int(at[r] + ln[r])]) for r in range(len(sizes))}


def rows_reading(rec, lay, byte):
    """the rows with an op whose store range holds store byte `byte`"""
    _, _, row, _, _, _, ln = _ops(rec)
    off = [int(x) for x in lay["op_store_off"]]
    return sorted({row[o] for o in range(len(row)) if off[o] != NONE and off[o] <= byte < off[o] + ln[o]})
