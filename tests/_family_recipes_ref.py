"""The family recipes in plain Python, written from the definition in
include/sdcas.h ("family recipes") and from nothing in the device code: a dict
keyed by the class (label, class number), one pass over the chunks, Python
integers reduced modulo 2^64. `literal_reading` is the same definition read
word by word, O(m^2), for small m. `versions` builds corpora of versions with
edits, over real bytes."""
import numpy as np

COUNTS = ("files", "chunks", "ops", "literal_ops", "copy_ops", "literal_bytes", "copy_bytes", "longest_op")
OPS32 = ("op_chunk", "op_src_chunk", "op_row", "op_src_row")
OPS64 = ("op_dst_off", "op_src_off", "op_len")
OPS = OPS32 + OPS64
ROWS = ("row_ops", "row_first_op")
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1

# the worked example of the header: v1 = A B C, v2 = A B X C
EXAMPLE = dict(chunk_file=[0, 0, 0, 1, 1, 1, 1], chunk_off=[0, 10, 30, 0, 10, 30, 35],
               chunk_len=[10, 20, 30, 10, 20, 5, 30], rep=[0, 1, 2, 0, 1, 5, 2], family=[0, 0])
EXAMPLE_OPS = dict(op_chunk=[0, 3, 5, 6], op_src_chunk=[0, 0, 5, 2], op_row=[0, 1, 1, 1], op_src_row=[0, 0, 1, 0],
                   op_dst_off=[0, 0, 30, 35], op_src_off=[0, 0, 30, 30], op_len=[60, 30, 5, 30])
EXAMPLE_REST = dict(chunk_op=[0, 0, 0, 1, 1, 2, 3], row_ops=[1, 3], row_first_op=[0, 1])
EXAMPLE_COUNTS = dict(files=2, chunks=7, ops=4, literal_ops=2, copy_ops=2, literal_bytes=65, copy_bytes=60,
                      longest_op=60)


def _lists(chunk_file, chunk_off, chunk_len, rep, family):
    return ([int(x) for x in np.asarray(chunk_file).reshape(-1)],
            [int(x) for x in np.asarray(chunk_off, dtype=np.uint64).reshape(-1)],
            [int(x) for x in np.asarray(chunk_len, dtype=np.uint64).reshape(-1)],
            [int(x) for x in np.asarray(rep, dtype=np.int64).reshape(-1)],
            [int(x) for x in np.asarray(family, dtype=np.int64).reshape(-1)])


def running_offsets(chunk_file, chunk_len):
    """the per-file running sums of chunk_len in position order"""
    at, off = {}, []
    for f, ln in zip((int(x) for x in chunk_file), (int(x) for x in chunk_len)):
        off.append(at.get(f, 0) & M64)
        at[f] = at.get(f, 0) + ln
    return np.array(off, dtype=np.uint64)


def _finish(m, n, nfiles, first, chunk_file, chunk_off, chunk_len):
    """the ops from f(c) per chunk (None: the chunk takes no part)"""
    ops, chunk_op = [], [NONE] * m
    for c in range(m):
        if first[c] is None:
            continue
        f = first[c]
        cont = False
        if c >= 1 and first[c - 1] is not None:
            g = first[c - 1]
            cont = (chunk_file[c - 1] == chunk_file[c] and (f == c) == (g == c - 1) and
                    chunk_off[c] == (chunk_off[c - 1] + chunk_len[c - 1]) & M64 and
                    chunk_file[f] == chunk_file[g] and chunk_off[f] == (chunk_off[g] + chunk_len[c - 1]) & M64)
        if cont:
            ops[-1]["op_len"] = (ops[-1]["op_len"] + chunk_len[c]) & M64
        else:
            ops.append(dict(op_chunk=c, op_src_chunk=f, op_row=chunk_file[c], op_src_row=chunk_file[f],
                            op_dst_off=chunk_off[c], op_src_off=chunk_off[f], op_len=chunk_len[c]))
        chunk_op[c] = len(ops) - 1
    row_ops, row_first = [0] * n, [NONE] * n
    for o, op in enumerate(ops):
        row_ops[op["op_row"]] += 1
        row_first[op["op_row"]] = min(row_first[op["op_row"]], o)
    lit = [op["op_chunk"] == op["op_src_chunk"] for op in ops]
    out = {name: np.array([op[name] for op in ops], dtype=np.uint32 if name in OPS32 else np.uint64) for name in OPS}
    out["op_literal"] = np.array(lit, dtype=bool)
    out["chunk_op"] = np.array(chunk_op, dtype=np.uint32)
    out["row_ops"] = np.array(row_ops, dtype=np.uint32)
    out["row_first_op"] = np.array(row_first, dtype=np.uint32)
    out["counts"] = dict(files=nfiles, chunks=sum(f is not None for f in first), ops=len(ops),
                         literal_ops=sum(lit), copy_ops=len(ops) - sum(lit),
                         literal_bytes=sum(op["op_len"] for op, x in zip(ops, lit) if x) & M64,
                         copy_bytes=sum(op["op_len"] for op, x in zip(ops, lit) if not x) & M64,
                         longest_op=max((op["op_len"] for op in ops), default=0))
    return out


def family_recipes(chunk_file, chunk_off, chunk_len, rep, family):
    """-> dict: the seven op arrays, "op_literal", "chunk_op", "row_ops", "row_first_op", "counts"; O(m)"""
    chunk_file, chunk_off, chunk_len, rep, family = _lists(chunk_file, chunk_off, chunk_len, rep, family)
    m, n = len(chunk_file), len(family)
    label = {i: family[i] for i in range(n) if 0 <= family[i] < n}
    lowest, first = {}, [None] * m
    for c in range(m):
        if chunk_file[c] not in label:
            continue
        cls = (label[chunk_file[c]], rep[c] if 0 <= rep[c] <= c else c)
        first[c] = lowest.setdefault(cls, c)
    return _finish(m, n, len(label), first, chunk_file, chunk_off, chunk_len)


def literal_reading(chunk_file, chunk_off, chunk_len, rep, family):
    """the same by the definition read literally: for every chunk, look through
    all chunks for the lowest one of its class; O(m^2)"""
    chunk_file, chunk_off, chunk_len, rep, family = _lists(chunk_file, chunk_off, chunk_len, rep, family)
    m, n = len(chunk_file), len(family)

    def part(c):
        return chunk_file[c] < n and 0 <= family[chunk_file[c]] < n

    def cls(c):
        return (family[chunk_file[c]], rep[c] if 0 <= rep[c] <= c else c)

    first = [min(d for d in range(m) if part(d) and cls(d) == cls(c)) if part(c) else None for c in range(m)]
    nfiles = sum(0 <= family[i] < n for i in range(n))
    return _finish(m, n, nfiles, first, chunk_file, chunk_off, chunk_len)


def same(got, want, names=OPS + ("chunk_op",) + ROWS):
    for name in names:
        if not np.array_equal(np.asarray(got[name]), np.asarray(want[name])):
            return False
    return got["counts"] == want["counts"]


def versions(seed, n_families=3, max_versions=4, blocks=12, block_bytes=(1, 40), strays=2):
    """a corpus of versions with edits over real bytes -> (contents: a list of
    bytes per row, chunk_file, chunk_off, chunk_len, rep, family). Every file is
    a list of blocks; a version copies its predecessor and inserts, deletes,
    replaces or repeats blocks. A chunk is a block, rep the lowest chunk with
    the same bytes (confirm's rep), family the file's family; rows of a family
    are adjacent, a few stray files carry an out-of-range label."""
    rng = np.random.default_rng(seed)

    def block():
        return rng.integers(0, 256, int(rng.integers(block_bytes[0], block_bytes[1] + 1)), dtype=np.uint8).tobytes()

    files, family = [], []
    for _ in range(n_families):
        head = len(files)
        cur = [block() for _ in range(int(rng.integers(1, blocks + 1)))]
        for _ in range(int(rng.integers(1, max_versions + 1))):
            files.append(list(cur))
            family.append(head)
            cur = list(cur)
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(0, len(cur) + 1))
                kind = int(rng.integers(0, 4))
                if kind == 0 or not cur:
                    cur.insert(at, block())
                elif kind == 1 and len(cur) > 1:
                    del cur[min(at, len(cur) - 1)]
                elif kind == 2:
                    cur[min(at, len(cur) - 1)] = block()
                else:
                    cur.insert(at, cur[int(rng.integers(0, len(cur)))])  # a block of its own, again
    n = len(files) + strays
    for s in range(strays):
        files.append([block() for _ in range(int(rng.integers(0, 4)))])
        family.append([-1, n, 1 << 40, -(1 << 63)][s % 4])
    chunk_file, chunk_off, chunk_len, rep, seen = [], [], [], [], {}
    for i, blks in enumerate(files):
        at = 0
        for b in blks:
            rep.append(seen.setdefault(b, len(rep)))
            chunk_file.append(i), chunk_off.append(at), chunk_len.append(len(b))
            at += len(b)
    contents = [b"".join(blks) for blks in files]
    return (contents, np.array(chunk_file, np.uint32), np.array(chunk_off, np.uint64), np.array(chunk_len, np.uint64),
            np.array(rep, np.int64), np.array(family, np.int64))
