"""A family store that forgets rows, on the GPU (csrc/family_forget.hip: keep and
moves; the bytes through csrc/family_store.hip's mover) against the plain
reference of tests/_family_forget_ref.py, through the host forms and through the
device forms over guarded buffers: inputs unchanged, guards intact, every output
pre-poisoned and untouched past what the call owns. Every comparison is exact
equality. No test hands the device anything meant to fault it: every array is
well formed, or holds values the kernels must treat as numbers only, or the
call is rejected before launch."""
import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from spacedrive_amd.recipes import apply_moves
from tests import _family_forget_ref as F
from tests import _family_recipes_ref as R
from tests import _family_store_ref as S
from tests._guarded import Guarded, guarded_from

pytestmark = pytest.mark.gpu

FILL = 0xFE
POISON = 0xA7
KEEP_DT = {"row_new": np.uint32, "row_from": np.uint32, "family": np.int64, "chunk_from": np.uint32,
           "chunk_file": np.uint32, "chunk_off": np.uint64, "chunk_len": np.uint64, "rep": np.int64}
SEEDS = range(12)


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def ptr(g, used=True):
    return g.ptr if used and g.nbytes else 0


def same(got, want, names):
    for name in names:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert got["counts"] == want["counts"], (got["counts"], want["counts"])


def dev_keep(eng, fl, off, ln, rep, fam, keep, outputs=(True,) * 9):
    """sdcas_dev_family_chunks_keep over guarded buffers -> (the dict, the output guards)"""
    arrays = [np.asarray(fl, np.uint32), np.asarray(off, np.uint64), np.asarray(ln, np.uint64),
              np.asarray(rep, np.int64), np.asarray(fam, np.int64), (np.asarray(keep).reshape(-1) != 0).astype(np.uint8)]
    m, n = arrays[0].size, arrays[4].size
    ins = [guarded_from(a, align=a.dtype.itemsize) for a in arrays]
    outs = [Guarded(np.dtype(KEEP_DT[name]).itemsize * (n if j < 3 else m), align=np.dtype(KEEP_DT[name]).itemsize,
                    fill=FILL) for j, name in enumerate(F.KEEP_ARRAYS)] + [Guarded(48, align=8, fill=FILL)]
    torch.cuda.synchronize()
    eng.dev_family_chunks_keep(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), m, ptr(ins[4]), ptr(ins[5]), n,
                               *(ptr(g, outputs[j]) for j, g in enumerate(outs)))
    eng.dev_sync()
    torch.cuda.synchronize()
    for x in ins + outs:
        assert x.check() == []
    assert all(x.unchanged() for x in ins)
    for j, o in enumerate(outs):
        assert outputs[j] or o.untouched()
    if not outputs[8]:
        return None, outs
    counts = dict(zip(F.KEEP_COUNTS, (int(x) for x in outs[8].download(np.uint64))))
    n2, m2 = counts["rows_kept"], counts["chunks_kept"]
    got = {"counts": counts}
    for j, name in enumerate(F.KEEP_ARRAYS):
        if not outputs[j]:
            continue
        size = np.dtype(KEEP_DT[name]).itemsize
        used = n if name == "row_new" else n2 if j < 3 else m2
        assert outs[j].untouched(lo=size * used), f"{name} was written past what was kept"
        got[name] = outs[j].download(KEEP_DT[name])[:used]
    return got, outs


def keep_both(eng, fl, off, ln, rep, fam, keep):
    """the reference against the host form and the device form, the device form twice -> the reference's dict"""
    want = F.keep(fl, off, ln, rep, fam, keep)
    same(eng.family_chunks_keep(fl, off, ln, rep, fam, keep), want, F.KEEP_ARRAYS)
    a, ga = dev_keep(eng, fl, off, ln, rep, fam, keep)
    same(a, want, F.KEEP_ARRAYS)
    _, gb = dev_keep(eng, fl, off, ln, rep, fam, keep)
    assert all((x.download() == y.download()).all() for x, y in zip(ga, gb))  # two calls give the same bytes
    return want


def dev_moves(eng, old, new, outputs=(True,) * 4, caps=None):
    """sdcas_dev_family_store_moves over guarded buffers -> (the dict, the output guards). caps: (max_ops,
    max_chunks, max_new_ops) above the numbers on the device, the arrays padded with poison"""
    def pad(a, dt, cap):
        out = np.full(cap, 0xFEFEFEFEFEFEFEFE if dt == np.uint64 else 0xFEFEFEFE, dt)
        a = np.asarray(a, dt).reshape(-1)
        out[:a.size] = a
        return out
    m, k = np.asarray(old["chunk_off"]).size, np.asarray(old["op_dst_off"]).size
    m2, k2 = np.asarray(new["chunk_from"]).size, np.asarray(new["op_chunk"]).size
    cap_k, cap_m2, cap_k2 = (k, m2, k2) if caps is None else caps
    arrays = [np.asarray(old["chunk_off"], np.uint64), np.asarray(old["chunk_op"], np.uint32),
              pad(old["op_dst_off"], np.uint64, cap_k), pad(old["op_store_off"], np.uint64, cap_k),
              np.array([k], np.uint64), pad(new["chunk_from"], np.uint32, cap_m2),
              pad(new["chunk_off"], np.uint64, cap_m2), pad(new["chunk_len"], np.uint64, cap_m2),
              pad(new["chunk_op"], np.uint32, cap_m2), np.array([m2], np.uint64), pad(new["op_chunk"], np.uint32, cap_k2),
              pad(new["op_src_chunk"], np.uint32, cap_k2), pad(new["op_dst_off"], np.uint64, cap_k2),
              pad(new["op_store_off"], np.uint64, cap_k2), np.array([k2], np.uint64)]
    ins = [guarded_from(a, align=a.dtype.itemsize) for a in arrays]
    outs = [Guarded(8 * cap_m2, align=8, fill=FILL) for _ in range(3)] + [Guarded(48, align=8, fill=FILL)]
    p = [ptr(g) for g in ins]
    torch.cuda.synchronize()
    eng.dev_family_store_moves(p[0], p[1], m, p[2], p[3], p[4], cap_k, p[5], p[6], p[7], p[8], p[9], cap_m2, p[10],
                               p[11], p[12], p[13], p[14], cap_k2, *(ptr(g, outputs[j]) for j, g in enumerate(outs)))
    eng.dev_sync()
    torch.cuda.synchronize()
    for x in ins + outs:
        assert x.check() == []
    assert all(x.unchanged() for x in ins)
    for j, o in enumerate(outs):
        assert outputs[j] or o.untouched()
    if not outputs[3]:
        return None, outs
    counts = dict(zip(F.MOVES_COUNTS, (int(x) for x in outs[3].download(np.uint64))))
    got = {"counts": counts}
    for j, name in enumerate(F.MOVE_ARRAYS):
        if outputs[j]:
            assert outs[j].untouched(lo=8 * counts["moves"]), f"{name} was written past the moves"
            got[name] = outs[j].download(np.uint64)[:counts["moves"]]
    return got, outs


def host_moves(eng, old, new):
    return eng.family_store_moves({"chunk_off": old["chunk_off"], "chunk_op": old["chunk_op"],
                                   "op_dst_off": old["op_dst_off"]}, {"op_store_off": old["op_store_off"]},
                                  {"chunk_off": new["chunk_off"], "chunk_op": new["chunk_op"],
                                   "op_chunk": new["op_chunk"], "op_src_chunk": new["op_src_chunk"],
                                   "op_dst_off": new["op_dst_off"]}, {"op_store_off": new["op_store_off"]},
                                  new["chunk_from"], new["chunk_len"])


def moves_both(eng, old, new, twice=True):
    want = F.moves(old, new)
    same(host_moves(eng, old, new), want, F.MOVE_ARRAYS)
    a, ga = dev_moves(eng, old, new)
    same(a, want, F.MOVE_ARRAYS)
    if twice:
        _, gb = dev_moves(eng, old, new)
        assert all((x.download() == y.download()).all() for x, y in zip(ga, gb))
    return want


def removal(eng, arrays, mask, twice=True):
    """keep, the reference's recipes and layout over what it leaves, moves -> (old side, kept, rec2, lay2, moves)"""
    fl, off, ln, rep, fam = arrays
    rec = R.family_recipes(fl, off, ln, rep, fam)
    lay = S.layout(rec)
    kept = keep_both(eng, fl, off, ln, rep, fam, mask)
    rec2 = R.family_recipes(kept["chunk_file"], kept["chunk_off"], kept["chunk_len"], kept["rep"], kept["family"])
    lay2 = S.layout(rec2)
    old = F.old_side(rec, lay, off)
    return (rec, lay), kept, rec2, lay2, moves_both(eng, old, F.new_side(kept, rec2, lay2), twice)


@pytest.fixture(scope="module")
def corpora():
    """the reference's corpora, computed once"""
    return {seed: R.versions(seed) for seed in SEEDS}


@pytest.mark.parametrize("seed", SEEDS)
def test_seeds_and_masks(eng, corpora, seed):
    contents, *arrays = corpora[seed]
    for name, mask in F.masks(seed, arrays[4]):
        (rec, lay), kept, rec2, lay2, mv = removal(eng, arrays, mask, twice=name == "random")
        assert mv["counts"]["lost_chunks"] == 0, name
        assert lay2["counts"]["store_bytes"] <= lay["counts"]["store_bytes"]
        assert mv["counts"]["moved_bytes"] == lay2["counts"]["store_bytes"]


def test_the_header_example(eng):
    ex = R.EXAMPLE
    arrays = [np.asarray(ex[k]) for k in ("chunk_file", "chunk_off", "chunk_len", "rep", "family")]
    _, kept, rec2, lay2, mv = removal(eng, arrays, F.EXAMPLE_KEEP)
    assert kept["chunk_from"].tolist() == [3, 4, 5, 6] and kept["rep"].tolist() == [0, 1, 2, 3]
    assert {k: mv[k].tolist() for k in F.MOVE_ARRAYS} == F.EXAMPLE_MOVES and mv["counts"] == F.EXAMPLE_MOVES_COUNTS


def sized(m, n, seed=0, lens=(1, 40)):
    """m chunks over n rows, chunks of a row adjacent, classes shared inside and across families, a few strays"""
    rng = np.random.default_rng(seed + m)
    fl = np.sort(rng.integers(0, n, m)).astype(np.uint32) if n else np.zeros(m, np.uint32)
    ln = rng.integers(lens[0], lens[1] + 1, m).astype(np.uint64)
    pos = np.arange(m, dtype=np.int64)
    own = rng.random(m) < 0.5
    if m:
        own[0] = True
    target = (rng.random(m) * (pos + 1)).astype(np.int64)
    last_own = np.maximum.accumulate(np.where(own, pos, 0))
    rep = np.where(own, pos, last_own[np.minimum(target, pos)]) if m else pos
    ln = np.where(rep == pos, ln, ln[rep]) if m else ln
    fam = np.maximum.accumulate(np.where(rng.random(n) < 0.3, np.arange(n), 0)).astype(np.int64)
    if n > 4:
        fam[rng.integers(1, n, 2)] = [-1, n]
    return fl, R.running_offsets(fl, ln), ln, rep.astype(np.int64), fam


@pytest.mark.parametrize("m,n", [(0, 0), (0, 3), (5, 0), (1, 1), (255, 9), (256, 9), (257, 300), (1025, 257)])
def test_sizes(eng, m, n):
    arrays = sized(m, n)
    rng = np.random.default_rng(m + n)
    for mask in (rng.random(n) < 0.6, np.ones(n, bool), np.zeros(n, bool)):
        removal(eng, arrays, mask, twice=False)


def test_past_one_pass_of_the_scan(eng):
    """1024 workgroup counts of 256 are one pass of the cross-launch scan: 262 144 + 257 chunks of one byte, rows
    and new chunks both past a pass by an odd remainder"""
    m = (1 << 18) + 257
    n = (1 << 18) + 3
    pos = np.arange(m, dtype=np.int64)
    fl = np.minimum(pos, n - 1).astype(np.uint32)
    ln = np.ones(m, np.uint64)
    rep = np.where(pos % 3 == 2, pos - 2, pos).astype(np.int64)  # a third of the chunks repeat the one two below
    fam = (np.arange(n) - np.arange(n) % 4).astype(np.int64)
    off = np.zeros(m, np.uint64)
    off[n - 1:] = np.arange(m - n + 1, dtype=np.uint64)
    keep = np.ones(n, np.uint8)
    keep[::4099] = 0  # few rows go: the new chunks still pass a pass, by 193
    want = F.keep(fl, off, ln, rep, fam, keep)
    assert want["counts"]["chunks_kept"] == (1 << 18) + 193 and want["counts"]["rows_removed"] == 64
    same(eng.family_chunks_keep(fl, off, ln, rep, fam, keep), want, F.KEEP_ARRAYS)
    got, _ = dev_keep(eng, fl, off, ln, rep, fam, keep)
    same(got, want, F.KEEP_ARRAYS)
    # moves over as many new chunks
    rec = R.family_recipes(fl, off, ln, rep, fam)
    lay = S.layout(rec)
    rec2 = R.family_recipes(want["chunk_file"], want["chunk_off"], want["chunk_len"], want["rep"], want["family"])
    lay2 = S.layout(rec2)
    old, new = F.old_side(rec, lay, off), F.new_side(want, rec2, lay2)
    mv = F.moves(old, new)
    assert mv["counts"]["lost_chunks"] == 0 and mv["counts"]["moves"] > 1024
    got, _ = dev_moves(eng, old, new)
    same(got, mv, F.MOVE_ARRAYS)
    same(host_moves(eng, old, new), mv, F.MOVE_ARRAYS)


def test_one_class_and_one_label_under_contention(eng):
    """every row holds the one class and carries the one label; the row of the class's representative and of the
    label's lowest row is removed: every survivor goes for the same two table words"""
    n, per = 3000, 3
    m = n * per
    fl = np.repeat(np.arange(n), per).astype(np.uint32)
    ln = np.full(m, 7, np.uint64)
    rep = np.zeros(m, np.int64)
    fam = np.zeros(n, np.int64)
    off = R.running_offsets(fl, ln)
    keep = np.ones(n, bool)
    keep[0] = False
    (rec, lay), kept, rec2, lay2, mv = removal(eng, (fl, off, ln, rep, fam), keep)
    assert (kept["rep"] == 0).all() and (kept["family"] == 0).all() and kept["chunk_from"][0] == per
    # the one stored chunk was row 0's; it is now row 1's first, found where row 0 left it
    assert lay2["counts"]["store_bytes"] == 7 and mv["move_src"].tolist() == [0] and mv["move_len"].tolist() == [7]
    keep[:] = False
    keep[n - 1] = True
    removal(eng, (fl, off, ln, rep, fam), keep)


def test_odd_values_are_numbers_only(eng):
    """rep outside [0, c], chunk_file >= n, labels -1, n, 2^40 and -2^63; moves over arbitrary arrays"""
    from tests.test_family_forget_host import hand_made, odd_inputs
    for seed in range(3):
        fl, off, ln, rep, fam = odd_inputs(seed)
        rng = np.random.default_rng(seed)
        keep_both(eng, fl, off, ln, rep, fam, rng.random(fam.size) < 0.7)
    old, new = hand_made()
    want = moves_both(eng, old, new)
    assert want["counts"]["lost_chunks"] == 4 and want["counts"]["moves"] == 2
    rng = np.random.default_rng(71)
    m, k, m2, k2 = 600, 70, 700, 90
    wide = lambda n: rng.integers(0, 1 << 64, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64)  # noqa
    old = dict(chunk_off=wide(m), chunk_op=rng.integers(0, k + 5, m).astype(np.uint32), op_dst_off=wide(k),
               op_store_off=np.where(rng.random(k) < 0.2, np.uint64(F.NONE), wide(k)))
    old["chunk_op"][rng.integers(0, m, 6)] = 0xFFFFFFFF
    new = dict(chunk_from=np.sort(rng.integers(0, m + 8, m2)).astype(np.uint32), chunk_off=wide(m2),
               chunk_len=rng.integers(0, 30, m2).astype(np.uint64),
               chunk_op=np.sort(rng.integers(0, k2 + 3, m2)).astype(np.uint32),
               op_chunk=rng.integers(0, m2, k2).astype(np.uint32), op_dst_off=wide(k2), op_store_off=wide(k2))
    new["op_src_chunk"] = np.where(rng.random(k2) < 0.7, new["op_chunk"], 0).astype(np.uint32)
    moves_both(eng, old, new)
    # the numbers on the device below the capacities: what lies past them is not read as ops or chunks
    want = F.moves(old, new)
    got, _ = dev_moves(eng, old, new, caps=(k + 9, m2 + 300, k2 + 5))
    same(got, want, F.MOVE_ARRAYS)


def test_null_outputs(eng, corpora):
    _, *arrays = corpora[1]
    fl, off, ln, rep, fam = arrays
    mask = F.masks(1, fam)[0][1]
    want = F.keep(fl, off, ln, rep, fam, mask)
    for j in range(9):
        outputs = tuple(i != j for i in range(9))
        got, _ = dev_keep(eng, fl, off, ln, rep, fam, mask, outputs)
        if got is not None:
            for name in got:
                if name != "counts":
                    assert np.array_equal(got[name], want[name]), name
    got, _ = dev_keep(eng, fl, off, ln, rep, fam, mask, (False,) * 8 + (True,))
    assert got["counts"] == want["counts"]
    dev_keep(eng, fl, off, ln, rep, fam, mask, (False,) * 9)
    rec, kept = R.family_recipes(fl, off, ln, rep, fam), want
    rec2 = R.family_recipes(kept["chunk_file"], kept["chunk_off"], kept["chunk_len"], kept["rep"], kept["family"])
    old, new = F.old_side(rec, S.layout(rec), off), F.new_side(kept, rec2, S.layout(rec2))
    mv = F.moves(old, new)
    for outputs in ((False, True, True, True), (True, False, True, True), (True, True, False, True),
                    (False, False, False, True), (True, True, True, False), (False,) * 4):
        got, _ = dev_moves(eng, old, new, outputs)
        if got is not None:
            assert got["counts"] == mv["counts"]
            for name in got:
                if name != "counts":
                    assert np.array_equal(got[name], mv[name]), name


def test_errors_leave_the_stream_empty_and_the_outputs_poisoned(eng):
    ex = R.EXAMPLE
    m, n = 7, 2
    ins = [guarded_from(np.asarray(ex[k], dt), align=np.dtype(dt).itemsize) for k, dt in (
        ("chunk_file", np.uint32), ("chunk_off", np.uint64), ("chunk_len", np.uint64), ("rep", np.int64),
        ("family", np.int64))] + [guarded_from(np.array([0, 1], np.uint8), align=1)]
    outs = [Guarded(np.dtype(KEEP_DT[name]).itemsize * 8, align=np.dtype(KEEP_DT[name]).itemsize, fill=FILL)
            for name in F.KEEP_ARRAYS] + [Guarded(48, align=8, fill=FILL)]
    torch.cuda.synchronize()
    E, C = N.SDCAS_E_INVALID, N.SDCAS_E_CAPACITY

    def code(fn, *a):
        with pytest.raises(N.SdcasError) as ei:
            fn(*a)
        return ei.value.code

    def keep(m=m, n=n, **at):
        p = [g.ptr for g in ins + outs]
        for j, v in at.items():
            p[int(j[1:])] = v
        return code(eng.dev_family_chunks_keep, p[0], p[1], p[2], p[3], m, p[4], p[5], n, *p[6:])

    for j in range(6):  # every needed pointer NULL
        assert keep(**{f"p{j}": 0}) == E, j
    for j in range(15):  # every pointer misaligned, but keep's bytes
        if j == 5:
            continue
        four = j in (0, 6, 7, 9, 10)
        assert keep(**{f"p{j}": (ins + outs)[j].ptr + (2 if four else 4)}) == E, j
    assert keep(m=(1 << 30) + 1) == C and keep(n=(1 << 30) + 1) == C

    rec = R.family_recipes(**ex)
    lay = S.layout(rec)
    kept = F.keep(*(ex[k] for k in ("chunk_file", "chunk_off", "chunk_len", "rep", "family")), F.EXAMPLE_KEEP)
    rec2 = R.family_recipes(kept["chunk_file"], kept["chunk_off"], kept["chunk_len"], kept["rep"], kept["family"])
    old, new = F.old_side(rec, lay, ex["chunk_off"]), F.new_side(kept, rec2, S.layout(rec2))
    arrays = [np.asarray(old["chunk_off"], np.uint64), np.asarray(old["chunk_op"], np.uint32),
              np.asarray(old["op_dst_off"], np.uint64), np.asarray(old["op_store_off"], np.uint64),
              np.array([4], np.uint64), np.asarray(new["chunk_from"], np.uint32), np.asarray(new["chunk_off"], np.uint64),
              np.asarray(new["chunk_len"], np.uint64), np.asarray(new["chunk_op"], np.uint32), np.array([4], np.uint64),
              np.asarray(new["op_chunk"], np.uint32), np.asarray(new["op_src_chunk"], np.uint32),
              np.asarray(new["op_dst_off"], np.uint64), np.asarray(new["op_store_off"], np.uint64),
              np.array([1], np.uint64)]
    mins = [guarded_from(a, align=a.dtype.itemsize) for a in arrays]
    mouts = [Guarded(32, align=8, fill=FILL) for _ in range(3)] + [Guarded(48, align=8, fill=FILL)]
    torch.cuda.synchronize()

    def moves(m=7, max_ops=4, max_chunks=4, max_new_ops=1, **at):
        p = [g.ptr for g in mins + mouts]
        for j, v in at.items():
            p[int(j[1:])] = v
        return code(eng.dev_family_store_moves, p[0], p[1], m, p[2], p[3], p[4], max_ops, p[5], p[6], p[7], p[8], p[9],
                    max_chunks, p[10], p[11], p[12], p[13], p[14], max_new_ops, *p[15:])

    for j in range(15):  # every needed pointer NULL, then every pointer misaligned
        assert moves(**{f"p{j}": 0}) == E, j
    for j in range(19):
        four = j in (1, 5, 8, 10, 11)
        assert moves(**{f"p{j}": (mins + mouts)[j].ptr + (2 if four else 4)}) == E, j
    assert moves(m=(1 << 30) + 1) == C and moves(max_ops=(1 << 30) + 1) == C
    assert moves(max_chunks=(1 << 30) + 1) == C and moves(max_new_ops=(1 << 30) + 1) == C
    eng.dev_sync()
    torch.cuda.synchronize()
    for g in outs + mouts:
        assert g.untouched() and g.check() == []
    assert all(x.unchanged() and x.check() == [] for x in ins + mins)
    # the host forms: needed NULL arrays, and nothing at all
    L = eng.L
    assert L.sdcas_family_chunks_keep(eng.ctx, *([None] * 4), 3, None, None, 0, *([None] * 9)) == E
    assert L.sdcas_family_chunks_keep(eng.ctx, *([None] * 4), 0, None, None, 2, *([None] * 9)) == E
    assert L.sdcas_family_chunks_keep(eng.ctx, *([None] * 4), 0, None, None, 0, *([None] * 9)) == N.SDCAS_OK
    assert L.sdcas_family_store_moves(eng.ctx, None, None, 0, None, None, 0, *([None] * 4), 0, *([None] * 4), 0,
                                      *([None] * 4)) == N.SDCAS_OK
    assert L.sdcas_family_store_moves(eng.ctx, None, None, 0, None, None, 0, *([None] * 4), 2, *([None] * 4), 0,
                                      *([None] * 4)) == E
    assert code(eng.family_forget_plan, 1, (1 << 30) + 1) == C


# ---- the bytes: the moves through the mover, old store to new store ------------------------------

def carry(eng, mv, old_store, size2):
    """sdcas_dev_family_restore with the moves as its ops -> the new store's bytes; both stores in guarded, poisoned
    buffers, so every byte of the new one comes from a move"""
    moves = mv["move_dst"].size
    ins = [guarded_from(np.zeros(moves, np.uint32), align=4), guarded_from(mv["move_dst"], align=8),
           guarded_from(mv["move_len"], align=8), guarded_from(mv["move_src"], align=8),
           guarded_from(np.array([moves], np.uint64), align=8), guarded_from(np.zeros(1, np.uint64), align=8),
           guarded_from(np.array([size2], np.uint64), align=8)]
    src = Guarded(len(old_store), align=16, fill=POISON).upload(np.frombuffer(bytes(old_store), np.uint8)).snapshot()
    dst = Guarded(size2 + 5, align=16, fill=POISON)
    cts = Guarded(32, align=8, fill=FILL)
    torch.cuda.synchronize()
    eng.dev_family_restore(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), ptr(ins[4]), moves, ptr(ins[5]), 0,
                           ptr(ins[6]), 1, ptr(src), len(old_store), ptr(dst), size2, ptr(cts))
    eng.dev_sync()
    torch.cuda.synchronize()
    for x in ins + [src, dst, cts]:
        assert x.check() == []
    assert all(x.unchanged() for x in ins) and src.unchanged() and dst.untouched(lo=size2)
    got = dict(zip(S.MOVE_COUNTS, (int(x) for x in cts.download(np.uint64))))
    assert got["bytes_moved"] == size2 and got["bad_ops"] == 0
    return dst.download()[:size2].tobytes()


def test_the_example_and_a_corpus_carried_on_the_device(eng, corpora):
    ex = R.EXAMPLE
    arrays = [np.asarray(ex[k]) for k in ("chunk_file", "chunk_off", "chunk_len", "rep", "family")]
    (rec, lay), kept, rec2, lay2, mv = removal(eng, arrays, F.EXAMPLE_KEEP, twice=False)
    a, b, c, x = b"a" * 10, b"b" * 20, b"c" * 30, b"x" * 5
    assert carry(eng, mv, a + b + c + x, 65) == a + b + x + c  # source residues 0, 12, 14; destinations 0, 14, 3
    seen = set()
    for seed in (2, 7):
        contents, *arrays = corpora[seed]
        for name, mask in F.masks(seed, arrays[4]):
            (rec, lay), kept, rec2, lay2, mv = removal(eng, arrays, mask, twice=False)
            store = S.pack_all(rec, lay, contents)
            size2 = lay2["counts"]["store_bytes"]
            got = carry(eng, mv, store, size2)
            assert got == apply_moves(mv, np.frombuffer(bytes(store), np.uint8), size2).tobytes(), name
            assert got == bytes(F.from_scratch(contents, arrays[0], arrays[1], arrays[2], arrays[4], mask)[3]), name
            seen |= {(int(s) % 16, int(d) % 16) for s, d in zip(mv["move_src"], mv["move_dst"])}
    assert len({s for s, _ in seen if s}) >= 8 and len({d for _, d in seen if d}) >= 8  # residues other than 0 mod 16
