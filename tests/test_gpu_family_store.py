"""The family store on the GPU (csrc/family_store.hip: the layout, pack and
restore) against the plain reference of tests/_family_store_ref.py, through the
host forms and through the device forms over guarded buffers: inputs unchanged,
guards intact, every output pre-poisoned, every byte between two windows and
between two store ranges still poison. Every comparison is exact equality. No
test hands the device anything meant to fault it: every op is well formed, or
is one the mover must skip, or the call is rejected before launch."""
import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests import _family_recipes_ref as R
from tests import _family_store_ref as S
from tests._guarded import Guarded, guarded_from
from tests.test_gpu_family_recipes import wanted

pytestmark = pytest.mark.gpu

FILL = 0xFE
POISON = 0xA7
M64 = (1 << 64) - 1
DT = {name: np.uint32 for name in R.OPS32}
DT.update({name: np.uint64 for name in R.OPS64})


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def T(eng):
    return eng.family_store_tile_bytes()


def ptr(g, used=True):
    return g.ptr if used and g.nbytes else 0


def op_guards(rec, max_ops):
    """the seven op arrays as guarded inputs of max_ops entries, poison past the ops"""
    out = []
    for name in R.OPS:
        a = np.full(max_ops, 0xFEFEFEFEFEFEFEFE if DT[name] == np.uint64 else 0xFEFEFEFE, DT[name])
        src = np.asarray(rec[name], DT[name]).reshape(-1)[:max_ops]
        a[:src.size] = src
        out.append(guarded_from(a, align=np.dtype(DT[name]).itemsize))
    return out


def dev_layout(eng, rec, max_ops=None, outputs=(True, True)):
    """sdcas_dev_family_store_layout over guarded buffers -> ({"op_store_off", "counts"}, the output guards)"""
    k = np.asarray(rec["op_chunk"]).size
    chunk_op = np.asarray(rec["chunk_op"], np.uint32)
    max_ops = max(k, chunk_op.size) if max_ops is None else max_ops
    ins = op_guards(rec, max_ops) + [guarded_from(chunk_op, align=4), guarded_from(np.array([k], np.uint64), align=8)]
    outs = [Guarded(8 * max_ops, align=8, fill=FILL), Guarded(48, align=8, fill=FILL)]
    torch.cuda.synchronize()
    eng.dev_family_store_layout(*(ptr(g) for g in ins[:7]), ptr(ins[7]), chunk_op.size, ptr(ins[8]), max_ops,
                                ptr(outs[0], outputs[0]), ptr(outs[1], outputs[1]))
    eng.dev_sync()
    torch.cuda.synchronize()
    for x in ins + outs:
        assert x.check() == []
    assert all(x.unchanged() for x in ins)
    for j, o in enumerate(outs):
        assert outputs[j] or o.untouched()
    ops = min(k, max_ops)
    assert outs[0].untouched(lo=8 * ops), "op_store_off was written past the ops"
    counts = dict(zip(S.LAYOUT_COUNTS, (int(x) for x in outs[1].download(np.uint64))))
    return {"op_store_off": outs[0].download(np.uint64)[:ops], "counts": counts}, outs


def same_layout(got, want):
    return np.array_equal(got["op_store_off"], want["op_store_off"]) and got["counts"] == want["counts"]


def layout_both(eng, rec):
    """the reference against the host form and the device form, the device form twice -> the reference's dict"""
    want = S.layout(rec)
    host = eng.family_store_layout(rec)
    assert same_layout(host, want), (host["counts"], want["counts"])
    a, ga = dev_layout(eng, rec)
    assert same_layout(a, want), (a["counts"], want["counts"])
    _, gb = dev_layout(eng, rec)
    assert all((x.download() == y.download()).all() for x, y in zip(ga, gb))  # two calls give the same bytes
    return want


def dev_move(eng, rec, off, at, base, ln, blob, store, restore, blob_bytes=None, store_bytes=None, counts=True):
    """sdcas_dev_family_pack / _restore: blob and store are Guardeds as the call finds them -> the counts"""
    k = np.asarray(rec["op_row"]).size
    n = np.asarray(at).size
    ins = op_guards(rec, k) + [guarded_from(np.asarray(off, np.uint64), align=8),
                               guarded_from(np.array([k], np.uint64), align=8)]
    rows = [guarded_from(np.asarray(a, np.uint64), align=8) if a is not None else None for a in (at, base, ln)]
    cts = Guarded(32, align=8, fill=FILL)
    blob_bytes = blob.nbytes if blob_bytes is None else blob_bytes
    store_bytes = store.nbytes if store_bytes is None else store_bytes
    (store if restore else blob).snapshot()
    torch.cuda.synchronize()
    rp = [ptr(g) if g is not None else 0 for g in rows]
    if restore:
        eng.dev_family_restore(ptr(ins[2]), ptr(ins[4]), ptr(ins[6]), ptr(ins[7]), ptr(ins[8]), k, rp[0], rp[1], rp[2],
                               n, ptr(store), store_bytes, ptr(blob), blob_bytes, ptr(cts, counts))
    else:
        eng.dev_family_pack(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[4]), ptr(ins[6]), ptr(ins[7]), ptr(ins[8]),
                            k, rp[0], rp[1], rp[2], n, ptr(blob), blob_bytes, ptr(store), store_bytes,
                            ptr(cts, counts))
    eng.dev_sync()
    torch.cuda.synchronize()
    for x in ins + [g for g in rows if g is not None] + [cts, blob, store]:
        assert x.check() == []
    assert all(x.unchanged() for x in ins + [g for g in rows if g is not None])
    assert (store if restore else blob).unchanged()
    if not counts:
        assert cts.untouched()
        return None
    return dict(zip(S.MOVE_COUNTS, (int(x) for x in cts.download(np.uint64))))


def poisoned(image):
    """a guarded buffer holding the image, 16 readable bytes kept behind it by the guard"""
    image = np.frombuffer(bytes(image), np.uint8)
    return Guarded(image.size, align=16, fill=POISON).upload(image)


# ---- the layout ---------------------------------------------------------------------------------

def test_the_worked_example(eng):
    want = layout_both(eng, R.family_recipes(**R.EXAMPLE))
    assert want["op_store_off"].tolist() == [0, 0, 60, 30] and want["counts"]["store_bytes"] == 65


@pytest.mark.parametrize("m,n", [(0, 1), (1, 1), (63, 1), (64, 9), (257, 30), (1025, 100), (5000, 300)])
def test_layout_sizes(eng, m, n):
    _, rec = wanted(m, n)
    want = layout_both(eng, rec)
    c = want["counts"]
    assert c["uncovered_ops"] == 0 and c["store_bytes"] == rec["counts"]["literal_bytes"]  # law 2: running sums
    assert c["ops"] == rec["counts"]["ops"] and c["literal_ops"] == rec["counts"]["literal_ops"]


def test_layout_more_workgroup_sums_than_one_pass_of_the_scan(eng):
    _, rec = wanted(262145, 4096)  # max_ops = m: 1025 sums, the one-workgroup scan carries into a second pass
    want = S.layout(rec)
    got, _ = dev_layout(eng, rec, max_ops=262145)
    assert same_layout(got, want) and want["counts"]["uncovered_ops"] == 0 and want["counts"]["copy_ops"] > 0
    assert same_layout(eng.family_store_layout(rec), want)


def test_layout_wrapping_zero_lengths_and_uncovered(eng):
    """the inputs of the recipes' test_interleaved_rows_zero_lengths_and_wrapping, and hand-made ops"""
    m = 700
    pos = np.arange(m)
    big = (1 << 63) + 1
    cases = [(pos & 1, None, np.full(m, 4), pos - (pos & 1), [0, 0]), ([0, 0, 0], [0, 0, 4], [4, 4, 4], [0, 0, 2], [0]),
             ([0, 0], [0, 0], [0, 0], [0, 0], [0]), ([0, 0, 0, 1, 1], [0, 3, 3, 0, 0], [3, 0, 2, 0, 0], [0, 1, 2, 1, 1], [0, 0]),
             (np.zeros(m), None, np.full(m, big, np.uint64), pos, [0]), ([0, 0, 1], [M64, 1, 5], [2, 3, 2], [0, 1, 0], [0, 0])]
    for cf, off, ln, rep, fam in cases:
        cf, ln = np.asarray(cf, np.uint32), np.asarray(ln, np.uint64)
        off = R.running_offsets(cf, ln) if off is None else np.asarray(off, np.uint64)
        layout_both(eng, R.family_recipes(cf, off, ln, rep, fam))
    # hand-made: lengths whose sum wraps, a copy past its literal's end, a source chunk and an op out of range
    rec = dict(op_chunk=[0, 1, 2, 3, 4, 5, 6], op_src_chunk=[0, 1, 0, 1, 9, 2, 3], op_row=[0, 0, 1, 1, 1, 1, 1],
               op_src_row=[0, 0, 0, 0, 0, 1, 0], op_dst_off=[0, M64 - 1, 0, 8, 16, 24, 32],
               op_src_off=[0, M64 - 1, 4, M64, 0, 0, 0], op_len=[M64, 9, M64 - 4, 8, 8, 8, 8],
               chunk_op=[0, 1, 7, 2, 9, 9, 9])
    want = layout_both(eng, rec)
    assert want["op_store_off"].tolist() == [0, M64, 4, (M64 + 1) & M64, S.NONE, S.NONE, S.NONE]
    assert want["counts"] == dict(ops=7, literal_ops=2, copy_ops=5, uncovered_ops=3, store_bytes=8,
                                  uncovered_bytes=24)
    got, _ = dev_layout(eng, rec, max_ops=4)  # fewer ops than the arrays hold: the rest stays as it was
    assert same_layout(got, S.layout(rec, ops=4))
    for outputs in ((False, True), (True, False), (False, False)):  # NULL optional outputs are accepted
        got, _ = dev_layout(eng, rec, outputs=outputs)
        assert not outputs[1] or got["counts"] == want["counts"]
        assert not outputs[0] or np.array_equal(got["op_store_off"], want["op_store_off"])


def test_layout_a_dirty_workspace_changes_nothing(eng):
    _, big = wanted(5000, 300)
    _, small = wanted(257, 30)
    a, ga = dev_layout(eng, big)
    assert same_layout(dev_layout(eng, small)[0], S.layout(small))
    c, gc = dev_layout(eng, big)
    assert same_layout(a, S.layout(big)) and same_layout(c, a)
    assert all((x.download() == y.download()).all() for x, y in zip(ga, gc))


# ---- every byte edge ----------------------------------------------------------------------------

def edge_case(length, rng):
    """256 literal ops of `length` bytes, one per (blob residue, store residue), and a copy of each in a row of
    its own: hand-made store offsets with poisoned gaps between the ranges"""
    rows = 512
    at, ln, off = np.zeros(rows, np.uint64), np.full(rows, length, np.uint64), np.zeros(rows, np.uint64)
    bpos = spos = 0
    for r in range(256):
        sr, dr = r >> 4, r & 15
        bpos += (sr - bpos) % 16 + 32
        at[r], bpos = bpos, bpos + length + 17
        spos += (dr - spos) % 16 + 32
        off[r], spos = spos, spos + length + 17
    for r in range(256):  # the copies: another blob residue for the same store range
        bpos += ((5 * (r >> 4) + 3 + (r & 15)) - bpos) % 16 + 32
        at[256 + r], bpos = bpos, bpos + length + 17
        off[256 + r] = off[r]
    rec = dict(op_chunk=np.arange(rows), op_src_chunk=np.concatenate([np.arange(256), np.arange(256)]),
               op_row=np.arange(rows), op_src_row=np.concatenate([np.arange(256), np.arange(256)]),
               op_dst_off=np.zeros(rows, np.uint64), op_src_off=np.zeros(rows, np.uint64), op_len=ln)
    blob = np.full(bpos + 16, POISON, np.uint8)
    for r in range(256):
        blob[int(at[r]):int(at[r]) + length] = rng.integers(0, 256, length, dtype=np.uint8)
    return rec, off, at, ln, blob, spos + 16


LENGTHS = ("0", "1", "2", "3", "15", "16", "17", "31", "32", "33", "47", "255", "256", "257", "T-1", "T", "T+1", "2*T+5")


@pytest.mark.parametrize("length", LENGTHS)
def test_every_residue_pair(eng, T, length):
    length = int(eval(length, {"T": T}))
    rec, off, at, ln, image, store_bytes = edge_case(length, np.random.default_rng(length))
    # pack: the 256 literal rows into a poisoned store
    want_store = bytearray([POISON]) * store_bytes
    want = S.move(rec, off, at, None, ln, bytearray(image.tobytes()), want_store, False, T)
    blob, store = poisoned(image), poisoned(bytes([POISON]) * store_bytes)
    got = dev_move(eng, rec, off, at, None, ln, blob, store, False)
    assert got == want and got["ops_moved"] == (256 if length else 0) and got["bytes_moved"] == 256 * length
    assert store.download().tobytes() == bytes(want_store)  # every range, and every gap byte still poison
    # restore: all 512 rows from that store into a poisoned blob
    want_blob = bytearray([POISON]) * image.size
    want = S.move(rec, off, at, None, ln, want_blob, want_store, True, T)
    blob2 = poisoned(bytes([POISON]) * image.size)
    got = dev_move(eng, rec, off, at, None, ln, blob2, store, True)
    assert got == want and got["bytes_moved"] == 512 * length and got["bad_ops"] == 0
    assert blob2.download().tobytes() == bytes(want_blob)
    back = blob2.download()
    for r in (0, 17, 255, 256, 511):
        assert back[int(at[r]):int(at[r]) + length].tobytes() == image[int(at[r % 256]):int(at[r % 256]) + length].tobytes()


# ---- windows and pieces ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    contents, fl, off, ln, rep, fam = R.versions(11, n_families=40, max_versions=6, blocks=30)
    rec = R.family_recipes(fl, off, ln, rep, fam)
    lay = S.layout(rec)
    return contents, rec, lay, S.pack_all(rec, lay, contents)


def test_windows_and_pieces(eng, T, corpus):
    contents, rec, lay, whole = corpus
    n, off = len(contents), lay["op_store_off"]
    part = [r for r in range(n) if rec["row_ops"][r]]
    assert lay["counts"]["store_bytes"] == len(whole) == rec["counts"]["literal_bytes"] < sum(len(c) for c in contents)
    # one call, device form
    image, at, ln = S.whole_rows(contents, gap=23)
    blob, store = poisoned(image), poisoned(bytes([POISON]) * len(whole))
    got = dev_move(eng, rec, off, at, None, ln, blob, store, False)
    assert got == S.move(rec, off, at, None, ln, bytearray(image), bytearray(len(whole)), False, T)
    assert got["bad_ops"] == 0 and got["bytes_moved"] == len(whole)
    assert store.download().tobytes() == bytes(whole)
    # windows of three rows, host form: the store carried from call to call
    st = None
    for first in range(0, n, 3):
        image, at, ln = S.whole_rows(contents, range(first, min(first + 3, n)), gap=5)
        st = eng.family_pack(rec, lay, image, at, ln, store=st)
    assert st.tobytes() == bytes(whole)
    # every row in pieces of 1000 bytes, device form into one poisoned store
    store = poisoned(bytes([POISON]) * len(whole))
    for pos in range(0, max(len(c) for c in contents), 1000):
        image, at, ln = S.whole_rows([c[pos:pos + 1000] for c in contents], gap=9, align=1)
        dev_move(eng, rec, off, at, np.full(n, pos, np.uint64), ln, poisoned(image), store, False)
    assert store.download().tobytes() == bytes(whole)
    # restore whole: every file comes back, gaps and absent rows untouched
    present = [r for r in range(n) if r % 5 != 2]
    image, at, ln = S.whole_rows([bytes([POISON]) * len(c) for c in contents], present, gap=23)
    image = bytearray(bytes([POISON]) * len(image))
    want = bytearray(image)
    S.move(rec, off, at, None, ln, want, whole, True, T)
    blob = poisoned(image)
    got = dev_move(eng, rec, off, at, None, ln, blob, store, True)
    back = blob.download()
    assert back.tobytes() == bytes(want) and got["bad_ops"] == 0
    for r in present:
        if r in part:
            assert back[int(at[r]):int(at[r] + ln[r])].tobytes() == contents[r]
    # restore in pieces of 1000 bytes, host form
    out = {r: bytearray() for r in part}
    for pos in range(0, max(len(c) for c in contents), 1000):
        ln = np.array([min(max(len(c) - pos, 0), 1000) for c in contents], np.uint64)
        at = np.arange(n, dtype=np.uint64) * np.uint64(1016)
        piece = eng.family_restore(rec, lay, whole, at, ln, np.full(n, pos, np.uint64), blob_bytes=1016 * n)
        for r in part:
            out[r] += piece[1016 * r:1016 * r + int(ln[r])].tobytes()
            assert not piece[1016 * r + int(ln[r]):1016 * (r + 1)].any()
    assert all(bytes(out[r]) == contents[r] for r in part)


# ---- bad ops, load balance, errors ----------------------------------------------------------------

def test_bad_ops_are_skipped_and_counted(eng, T):
    rec = dict(op_chunk=[0, 1, 2, 3, 4, 5, 6], op_src_chunk=[0, 1, 2, 3, 4, 5, 0], op_row=[0, 9, 1, 2, 3, 1, 2],
               op_src_row=[0, 9, 1, 2, 3, 1, 0], op_dst_off=[0, 0, M64 - 3, 0, 0, 40, 100],
               op_src_off=[0, 0, M64 - 3, 0, 0, 40, 0], op_len=[40, 8, 8, 50, 30, 20, 40])
    off = np.array([0, 40, 48, 200, 56, 86, 0], np.uint64)  # op 3 lies past the store's capacity of 128
    at, ln = np.array([16, 80, 160, 1000], np.uint64), np.array([40, 70, 150, 30], np.uint64)  # row 3 past the blob
    image = np.random.default_rng(5).integers(0, 256, 320, dtype=np.uint8)
    want_store = bytearray([POISON]) * 128
    want = S.move(rec, off, at, None, ln, bytearray(image.tobytes()), want_store, False, T)
    assert want == dict(ops_moved=2, bytes_moved=60, bad_ops=4, tiles=2)  # row 9, the wrap, op 3, row 3's window
    blob, store = poisoned(image), poisoned(bytes([POISON]) * 128)
    assert dev_move(eng, rec, off, at, None, ln, blob, store, False) == want
    assert store.download().tobytes() == bytes(want_store)
    want_blob = bytearray([POISON]) * 320
    want = S.move(rec, off, at, None, ln, want_blob, want_store, True, T)
    assert want == dict(ops_moved=3, bytes_moved=100, bad_ops=4, tiles=3)  # the copy, op 6, moves too
    blob = poisoned(bytes([POISON]) * 320)
    assert dev_move(eng, rec, off, at, None, ln, blob, store, True) == want
    assert blob.download().tobytes() == bytes(want_blob)
    assert dev_move(eng, rec, off, at, None, ln, blob, store, True, counts=False) is None  # NULL counts
    c = {}
    eng.family_restore(rec, {"op_store_off": off}, np.frombuffer(bytes(want_store), np.uint8), at, ln, blob_bytes=320,
                       counts=c)
    assert c == want


def test_one_long_op_beside_many_short_ones(eng, T):
    rng = np.random.default_rng(9)
    lens = np.concatenate([[64 * T + 7], rng.integers(1, 41, 3000)]).astype(np.uint64)
    k = lens.size
    rec = dict(op_chunk=np.arange(k), op_src_chunk=np.arange(k), op_row=np.arange(k), op_src_row=np.arange(k),
               op_dst_off=np.zeros(k, np.uint64), op_src_off=np.zeros(k, np.uint64), op_len=lens,
               chunk_op=np.arange(k))
    lay = S.layout(rec)
    assert same_layout(eng.family_store_layout(rec), lay)
    contents = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    image, at, ln = S.whole_rows(contents, gap=3)
    whole = S.pack_all(rec, lay, contents)
    blob, store = poisoned(image), poisoned(bytes([POISON]) * len(whole))
    got = dev_move(eng, rec, lay["op_store_off"], at, None, ln, blob, store, False)
    assert got == S.move(rec, lay["op_store_off"], at, None, ln, bytearray(image), bytearray(len(whole)), False, T)
    assert got["ops_moved"] == k and got["tiles"] >= 64 + k and store.download().tobytes() == bytes(whole)
    blob = poisoned(bytes([POISON]) * len(image))
    dev_move(eng, rec, lay["op_store_off"], at, None, ln, blob, store, True)
    back = blob.download()
    assert all(back[int(at[r]):int(at[r] + ln[r])].tobytes() == contents[r] for r in range(k))
    gaps = np.ones(len(image), bool)
    for r in range(k):
        gaps[int(at[r]):int(at[r] + ln[r])] = False
    assert (back[gaps] == POISON).all()


def test_errors_leave_the_stream_empty_and_the_outputs_poisoned(eng):
    rec = R.family_recipes(**R.EXAMPLE)
    k, m = 4, 7
    ins = op_guards(rec, k) + [guarded_from(rec["chunk_op"], align=4), guarded_from(np.array([k], np.uint64), align=8)]
    off = guarded_from(np.array([0, 0, 60, 30], np.uint64), align=8)
    rows = [guarded_from(np.array(a, np.uint64), align=8) for a in ([0, 64], [0, 0], [60, 65])]
    blob, store = Guarded(144, align=16, fill=FILL), Guarded(80, align=16, fill=FILL)
    out_off, cts = Guarded(8 * k, align=8, fill=FILL), Guarded(48, align=8, fill=FILL)
    torch.cuda.synchronize()
    E = N.SDCAS_E_INVALID

    def code(fn, *a):
        with pytest.raises(N.SdcasError) as ei:
            fn(*a)
        return ei.value.code

    def layout(max_ops=k, m=m, **at):
        p = [g.ptr for g in ins] + [out_off.ptr, cts.ptr]
        for j, v in at.items():
            p[int(j[1:])] = v
        return code(eng.dev_family_store_layout, *p[:8], m, p[8], max_ops, p[9], p[10])

    for j in range(9):  # every needed pointer NULL, then misaligned
        assert layout(**{f"p{j}": 0}) == E, j
        assert layout(**{f"p{j}": ins[j].ptr + (2 if j in (0, 1, 2, 3, 7) else 4)}) == E, j
    assert layout(p9=out_off.ptr + 4) == E and layout(p10=cts.ptr + 4) == E
    assert layout(max_ops=(1 << 30) + 1) == N.SDCAS_E_CAPACITY and layout(m=(1 << 30) + 1) == N.SDCAS_E_CAPACITY

    def move(restore, max_ops=k, n=2, blob_bytes=144, store_bytes=80, **at):
        p = [ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[4].ptr, ins[6].ptr, off.ptr, ins[8].ptr, rows[0].ptr, rows[1].ptr,
             rows[2].ptr, blob.ptr, store.ptr, cts.ptr]
        for j, v in at.items():
            p[int(j[1:])] = v
        if restore:
            return code(eng.dev_family_restore, p[2], p[3], p[4], p[5], p[6], max_ops, p[7], p[8], p[9], n, p[11],
                        store_bytes, p[10], blob_bytes, p[12])
        return code(eng.dev_family_pack, *p[:7], max_ops, p[7], p[8], p[9], n, p[10], blob_bytes, p[11], store_bytes,
                    p[12])

    for restore in (False, True):
        for j in range(13):
            if j == 8 or j == 12 or (restore and j < 2):  # row_base and the counts may be NULL; restore reads no chunks
                continue
            assert move(restore, **{f"p{j}": 0}) == E, (restore, j)
        for j in range(13):
            if restore and j < 2:
                continue
            step = 2 if j < 3 else 8 if j in (10, 11) else 4
            p = [ins[0], ins[1], ins[2], ins[4], ins[6], off, ins[8], rows[0], rows[1], rows[2], blob, store, cts][j]
            assert move(restore, **{f"p{j}": p.ptr + step}) == E, (restore, j)
        assert move(restore, max_ops=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
        assert move(restore, n=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    eng.dev_sync()
    torch.cuda.synchronize()
    for g in (blob, store, out_off, cts):
        assert g.untouched() and g.check() == []
    assert all(x.unchanged() and x.check() == [] for x in ins + rows + [off])
    # the host forms: needed NULL arrays, and nothing at all
    L = eng.L
    assert L.sdcas_family_store_layout(eng.ctx, *([None] * 7), 4, None, 0, None, None) == E
    assert L.sdcas_family_store_layout(eng.ctx, *([None] * 7), 0, None, 0, None, None) == N.SDCAS_OK
    assert L.sdcas_family_pack(eng.ctx, *([None] * 6), 0, None, None, None, 0, None, 0, None, 0, None) == N.SDCAS_OK
    assert L.sdcas_family_restore(eng.ctx, *([None] * 4), 0, None, None, None, 0, None, 0, None, 0, None) == N.SDCAS_OK
    assert L.sdcas_family_restore(eng.ctx, *([None] * 4), 3, None, None, None, 0, None, 0, None, 0, None) == E
    assert code(eng.family_store_plan, 1, (1 << 30) + 1) == N.SDCAS_E_CAPACITY
