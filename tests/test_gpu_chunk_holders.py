"""The holders index on the GPU (sdcas_chunk_holders_match / _add / _remove and
their device forms, csrc/chunk_holders.hip) against the Python reference of
tests/_chunk_holders_ref.py: through the host call and through the device call
over guarded buffers (inputs unchanged, guards intact, NULL outputs untouched,
new arrays past entries_new still holding their fill). Every comparison is
exact equality. No test hands the device a malformed index."""
import numpy as np
import pytest
import torch

from spacedrive_amd import ChunkHolders, ChunkIndex, _native as N
from tests import _chunk_holders_ref as H
from tests import _chunk_index_ref as R
from tests._guarded import Guarded, guarded_from

pytestmark = pytest.mark.gpu

FILL = 0xFE
MATCH_COUNTS = ("queries", "hits", "misses", "skipped")
ADD_COUNTS = ("queries", "hits", "added", "batch_duplicates", "entries_old", "entries_new")
REMOVE_COUNTS = ("entries_old", "removed", "entries_new", "values")
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool():
    """400 distinct random pairs with real keys"""
    return R.random_pairs(np.random.default_rng(41), 400)


def index_guards(entries, bits):
    keys, dig, values, d, _ = H.arrays(entries, bits)
    return [guarded_from(keys, align=8), guarded_from(dig, align=16), guarded_from(values, align=8),
            guarded_from(d, align=4)]


def batch_guards(keys, dig, valid):
    gs = [guarded_from(np.asarray(keys, np.uint64), align=8), guarded_from(np.asarray(dig, np.uint8), align=16)]
    if valid is not None:
        gs.append(guarded_from(np.asarray(valid, np.uint8), align=1))
    return gs


def ptr(g, used=True):
    return g.ptr if used and g.nbytes else 0


def widths(n):
    return sorted({0, R.dir_bits(n), 3})


def holders_index(pairs_keys, pairs_dig, runs, first_value=100):
    """entries: pair i held by runs[i] values first_value + 7 j (j < runs[i])"""
    return sorted((int(k), d.tobytes(), first_value + 7 * j)
                  for k, d, r in zip(pairs_keys, pairs_dig, runs) for j in range(r))


def assert_index(entries, bits):
    k, d, v, dr, _ = H.arrays(entries, bits)
    from spacedrive_amd import Engine
    assert Engine.chunk_holders_check(k, d, v, dr, bits) == (N.SDCAS_OK, None)


# ---- match ------------------------------------------------------------------------------

def dev_match(eng, entries, bits, keys, dig, valid=None, outputs=(True, True, True, True)):
    m, n = len(keys), len(entries)
    ix, bt = index_guards(entries, bits), batch_guards(keys, dig, valid)
    outs = [Guarded(8 * m, align=8, fill=FILL), Guarded(8 * m, align=8, fill=FILL), Guarded(4 * m, align=4, fill=FILL),
            Guarded(32, align=8, fill=FILL)]
    torch.cuda.synchronize()
    eng.dev_chunk_holders_match(ptr(ix[0]), ptr(ix[1]), ptr(ix[2]), ptr(ix[3], n > 0), n, bits, ptr(bt[0]), ptr(bt[1]),
                                bt[2].ptr if valid is not None and m else 0, m,
                                *(ptr(o, outputs[j]) for j, o in enumerate(outs)))
    eng.dev_sync()
    torch.cuda.synchronize()
    for g in ix + bt + outs:
        assert g.check() == []
    assert all(g.unchanged() for g in ix + bt)
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {j} was written"
    return outs[0].download(np.int64), outs[1].download(np.uint64), outs[2].download(np.uint32), \
        dict(zip(MATCH_COUNTS, (int(x) for x in outs[3].download(np.uint64))))


def match_both(eng, entries, bits, keys, dig, valid=None):
    keys, dig = np.asarray(keys, np.uint64), np.asarray(dig, np.uint8).reshape(-1, 32)
    wpos, wval, whold, wcounts = H.match(entries, keys, dig, valid)
    for pos, val, hold, counts in (eng.chunk_holders_match(H.arrays(entries, bits), keys, dig, valid),
                                   dev_match(eng, entries, bits, keys, dig, valid)):
        assert (pos == wpos).all() and (val == wval).all() and (hold == whold).all() and counts == wcounts
    # pos is the run's first entry and holders its exact length
    for c in np.flatnonzero(wpos >= 0):
        p, h, pair = int(wpos[c]), int(whold[c]), (int(keys[c]), dig[c].tobytes())
        assert all(e[:2] == pair for e in entries[p:p + h])
        assert (p == 0 or entries[p - 1][:2] != pair) and (p + h == len(entries) or entries[p + h][:2] != pair)
    return wpos, whold, wcounts


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9])
def test_match_small_indexes(eng, pool, n):
    """n entries as runs of 1, 2 and 3 holders over the first pairs"""
    keys, dig = pool
    runs, left = [], n
    while left:
        runs.append(min(left, 1 + len(runs) % 3))
        left -= runs[-1]
    entries = holders_index(keys, dig, runs)
    assert len(entries) == n
    rng = np.random.default_rng(n)
    for bits in widths(n):
        assert_index(entries, bits)
        for m in (0, 1, 255, 256, 257):
            pick = np.concatenate([np.arange(len(runs)), 20 + np.arange(max(m - len(runs), 0))])[:m]
            pick = pick[rng.permutation(m)]
            pos, hold, counts = match_both(eng, entries, bits, keys[pick], dig[pick])
            assert counts["hits"] == int((pick < len(runs)).sum()) and int(hold.sum()) == sum(runs[p] for p in pick
                                                                                              if p < len(runs))


def test_match_runs_of_1_2_3_and_1000(eng, pool):
    """runs at the very start and the very end of the index, a run of 1000"""
    keys, dig = pool
    order = np.argsort(keys[:100], kind="stable")
    k, d = keys[:100][order], dig[:100][order]
    runs = [1 + i % 3 for i in range(100)]
    runs[0], runs[-1], runs[50] = 3, 2, 1000
    entries = holders_index(k, d, runs)
    assert entries[0][:2] == entries[2][:2] and entries[-1][:2] == entries[-2][:2]
    pick = np.random.default_rng(42).permutation(np.concatenate([np.arange(100), 200 + np.arange(60)]))
    for bits in (0, 3, R.dir_bits(len(entries))):
        assert_index(entries, bits)
        pos, hold, counts = match_both(eng, entries, bits, keys[:400][np.where(pick < 100, order[pick % 100], pick)],
                                       dig[:400][np.where(pick < 100, order[pick % 100], pick)])
        assert counts == dict(queries=160, hits=100, misses=60, skipped=0)
        assert hold.max() == 1000 and pos.min() == -1 and 0 in pos and len(entries) - 2 in pos
    # NULL outputs, one at a time
    q = np.arange(150)
    for outputs in ((False, True, True, True), (True, False, True, True), (True, True, False, True),
                    (True, True, True, False), (False, False, False, False)):
        dev_match(eng, entries, 3, keys[q], dig[q], None, outputs)


def test_match_a_run_fills_a_bucket_and_extreme_keys_and_values(eng, pool):
    _, dig = pool
    keys = np.array([0, 0, 3 << 61, U64_MAX, U64_MAX], np.uint64)
    # bucket 3 of 8 holds one run and nothing else; keys 0 and 2^64 - 1 hold runs too;
    # values 0 and 2^64 - 1 inside one run: the lowest is 0 only in the unsigned order
    entries = sorted([(0, dig[0].tobytes(), 0), (0, dig[0].tobytes(), U64_MAX), (0, dig[0].tobytes(), 1 << 63),
                      (0, dig[1].tobytes(), 5)] +
                     [(3 << 61, dig[2].tobytes(), v) for v in range(40)] +
                     [(U64_MAX, dig[3].tobytes(), U64_MAX), (U64_MAX, dig[3].tobytes(), 0),
                      (U64_MAX, dig[4].tobytes(), 9)])
    assert [e[2] for e in entries[:3]] == [0, 1 << 63, U64_MAX]
    d8 = H.directory(entries, 3)
    assert d8[4] - d8[3] == 40
    q_keys = np.array([0, 0, 3 << 61, U64_MAX, U64_MAX, 0, U64_MAX, 3 << 61, 1], np.uint64)
    q_dig = np.stack([dig[0], dig[1], dig[2], dig[3], dig[4], dig[9], dig[9], dig[9], dig[0]])
    for bits in (0, 1, 3, 6):
        assert_index(entries, bits)
        pos, hold, counts = match_both(eng, entries, bits, q_keys, q_dig)
        assert hold.tolist() == [3, 1, 40, 2, 1, 0, 0, 0, 0] and counts["hits"] == 5
        _, val, _, _ = eng.chunk_holders_match(H.arrays(entries, bits), q_keys, q_dig)
        assert val[:5].tolist() == [0, 5, 0, 0, 9]


def forged_run(seed, count):
    """`count` digests under one key that differ in their last two bytes only"""
    base = np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)
    dig = np.tile(base, (count, 1))
    v = np.arange(count)
    dig[:, 31], dig[:, 30] = v & 0xFF, v >> 8
    return np.full(count, 0x1234567890ABCDEF, np.uint64), dig


def test_match_one_forged_key(eng):
    """one key shared by 600 distinct digests, each with 1 to 3 holders; the
    digests in between miss"""
    keys, dig = forged_run(43, 1200)
    even = np.arange(1200) % 2 == 0
    runs = [1 + i % 3 for i in range(600)]
    entries = holders_index(keys[even], dig[even], runs)
    pick = np.random.default_rng(44).permutation(1200)
    for bits in (0, 5):
        assert_index(entries, bits)
        pos, hold, counts = match_both(eng, entries, bits, keys[pick], dig[pick])
        assert counts["hits"] == 600 and ((pos >= 0) == even[pick]).all()
        assert (hold[even[pick]] == np.array(runs)[pick[even[pick]] // 2]).all()


def test_match_valid_mask_and_errors(eng, pool):
    keys, dig = pool
    entries = holders_index(keys[:100], dig[:100], [1 + i % 4 for i in range(100)])
    valid = (np.random.default_rng(45).random(150) > 0.4).astype(np.uint8)
    pos, hold, counts = match_both(eng, entries, R.dir_bits(len(entries)), keys[:150], dig[:150], valid)
    assert counts["skipped"] == int((valid == 0).sum()) and (pos[valid == 0] == -1).all() and (hold[valid == 0] == 0).all()
    ix, bt = index_guards(entries, 2), batch_guards(keys[:5], dig[:5], None)
    outs = [Guarded(40, align=8, fill=FILL), Guarded(40, align=8, fill=FILL), Guarded(20, align=4, fill=FILL),
            Guarded(32, align=8, fill=FILL)]
    torch.cuda.synchronize()

    def call(idx_dig=ix[1].ptr, q_dig=bt[1].ptr, n=len(entries), bits=2, m=5, hold=outs[2].ptr):
        with pytest.raises(N.SdcasError) as ei:
            eng.dev_chunk_holders_match(ix[0].ptr, idx_dig, ix[2].ptr, ix[3].ptr, n, bits, bt[0].ptr, q_dig, 0, m,
                                        outs[0].ptr, outs[1].ptr, hold, outs[3].ptr)
        return ei.value.code

    assert call(idx_dig=ix[1].ptr + 8) == N.SDCAS_E_INVALID
    assert call(q_dig=bt[1].ptr + 4) == N.SDCAS_E_INVALID
    assert call(hold=outs[2].ptr + 2) == N.SDCAS_E_INVALID
    assert call(n=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    assert call(m=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    assert call(bits=29) == N.SDCAS_E_CAPACITY
    eng.dev_sync()
    torch.cuda.synchronize()
    assert all(o.untouched() and o.check() == [] for o in outs)


# ---- add --------------------------------------------------------------------------------

def dev_add(eng, entries, bits_old, keys, dig, values, valid, bits_new, outputs=(True, True, True)):
    """sdcas_dev_chunk_holders_add over guarded buffers -> (new arrays, pos, flags, counts)"""
    m, n = len(keys), len(entries)
    cap = n + m
    ix, bt = index_guards(entries, bits_old), batch_guards(keys, dig, valid)
    gv = None if values is None else guarded_from(np.asarray(values, np.uint64), align=8)
    new = [Guarded(8 * cap, align=8, fill=FILL), Guarded(32 * cap, align=16, fill=FILL),
           Guarded(8 * cap, align=8, fill=FILL), Guarded(4 * ((1 << bits_new) + 1), align=4, fill=FILL)]
    outs = [Guarded(8 * m, align=8, fill=FILL), Guarded(m, align=1, fill=FILL), Guarded(48, align=8, fill=FILL)]
    torch.cuda.synchronize()
    eng.dev_chunk_holders_add(ptr(ix[0]), ptr(ix[1]), ptr(ix[2]), ptr(ix[3], n > 0), n, bits_old, ptr(bt[0]),
                              ptr(bt[1]), ptr(gv) if gv is not None else 0,
                              bt[2].ptr if valid is not None and m else 0, m, ptr(new[0]), ptr(new[1]), ptr(new[2]),
                              new[3].ptr, bits_new, *(ptr(o, outputs[j]) for j, o in enumerate(outs)))
    eng.dev_sync()
    torch.cuda.synchronize()
    ins = ix + bt + ([gv] if gv is not None else [])
    for g in ins + new + outs:
        assert g.check() == []
    assert all(g.unchanged() for g in ins)
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {j} was written"
    counts = dict(zip(ADD_COUNTS, (int(x) for x in outs[2].download(np.uint64)))) if outputs[2] else None
    return new, outs[0].download(np.int64), outs[1].download(np.uint8), counts


def add_both(eng, entries, bits_old, keys, dig, values, valid=None, bits_new=None):
    keys, dig = np.asarray(keys, np.uint64), np.asarray(dig, np.uint8).reshape(-1, 32)
    values = None if values is None else np.asarray(values, np.uint64)
    m, n = len(keys), len(entries)
    if bits_new is None:
        bits_new = R.dir_bits(n + m)
    want, wpos, wflags, wcounts = H.add(entries, keys, dig, values, valid)
    wk, wd, wv, wdir, _ = H.arrays(want, bits_new)
    e = len(want)
    (nk, nd, nv, ndir, nb), pos, flags, counts = eng.chunk_holders_add(H.arrays(entries, bits_old), keys, dig, values,
                                                                       valid, bits_new)
    assert counts == wcounts and nb == bits_new
    assert (nk == wk).all() and (nd == wd).all() and (nv == wv).all() and (ndir == wdir).all()
    assert (pos == wpos).all() and (flags == wflags).all()
    new, pos, flags, counts = dev_add(eng, entries, bits_old, keys, dig, values, valid, bits_new)
    assert counts == wcounts
    assert (new[0].download(np.uint64, e) == wk).all() and (new[1].download(np.uint8, 32 * e).reshape(-1, 32) == wd).all()
    assert (new[2].download(np.uint64, e) == wv).all() and (new[3].download(np.uint32) == wdir).all()
    assert (pos == wpos).all() and (flags == wflags).all()
    # entries past entries_new are left as they were
    assert new[0].untouched(8 * e) and new[1].untouched(32 * e) and new[2].untouched(8 * e)
    assert_index(want, bits_new)
    return want, wflags, wcounts


def test_add_to_an_empty_index_and_nothing(eng, pool):
    keys, dig = pool
    pick = np.array([3, 1, 3, 2, 1, 3, 0, 2])
    values = np.array([9, 9, 9, 9, 8, 7, 9, 9], np.uint64)
    want, flags, counts = add_both(eng, [], 0, keys[pick], dig[pick], values)
    # (3, 9) at three positions: ADDED on the lowest, 0 on the rest; (3, 7) and (1, 8) are other triples
    assert flags.tolist() == [2, 2, 0, 2, 2, 2, 2, 0]
    assert counts == dict(queries=8, hits=0, added=6, batch_duplicates=2, entries_old=0, entries_new=6)
    add_both(eng, [], 0, keys[:0], dig[:0], values[:0])  # nothing into nothing
    add_both(eng, want, 0, keys[:0], dig[:0], values[:0], bits_new=3)  # m = 0: copied and re-bucketed
    # a batch that is all hits
    k, d, v = H.batch_arrays(want * 2)
    _, flags, counts = add_both(eng, want, 0, k, d, v)
    assert (flags == H.HIT).all() and counts["hits"] == 12 and counts["entries_new"] == 6


def test_add_one_triple_at_three_positions(eng, pool):
    keys, dig = pool
    entries = holders_index(keys[:20], dig[:20], [2] * 20)
    k = np.concatenate([keys[30:40], keys[[35, 35]], keys[:3]])
    d = np.concatenate([dig[30:40], dig[[35, 35]], dig[:3]])
    v = np.concatenate([np.full(12, 55), [100, 101, 108]]).astype(np.uint64)  # (0, 100) is a hit, the others are new
    p = np.array([5, 0, 1, 10, 2, 3, 11, 4, 6, 7, 8, 9, 12, 13, 14])  # pair 35 at positions 0, 3 and 6
    for bits in (0, 3):
        want, flags, counts = add_both(eng, entries, bits, k[p], d[p], v[p])
        assert flags[[0, 3, 6]].tolist() == [H.ADDED, 0, 0] and counts["batch_duplicates"] == 2 and counts["hits"] == 1
        pos = H.add(entries, k[p], d[p], v[p])[1]
        assert pos[0] == pos[3] == pos[6]


def test_add_300_values_into_a_run_of_1000(eng, pool):
    """one pair with 300 distinct values in one batch, into an index that holds
    1000 other values of that pair, the new values interleaved among the old"""
    keys, dig = pool
    run = [(int(keys[7]), dig[7].tobytes(), 4 * j) for j in range(1000)]
    entries = sorted(run + holders_index(keys[20:60], dig[20:60], [1 + i % 3 for i in range(40)]))
    rng = np.random.default_rng(46)
    new_vals = (4 * rng.permutation(1000)[:300] + 1 + rng.integers(0, 3, 300)).astype(np.uint64)
    k = np.concatenate([np.full(300, keys[7]), keys[50:80]])
    d = np.concatenate([np.tile(dig[7], (300, 1)), dig[50:80]])
    v = np.concatenate([new_vals, np.full(30, 100, np.uint64)])  # pairs 50..59 with value 100 are hits
    p = rng.permutation(330)
    want, flags, counts = add_both(eng, entries, R.dir_bits(len(entries)), k[p], d[p], v[p])
    assert counts["added"] == 300 - (300 - np.unique(new_vals).size) + 20 and counts["hits"] == 10
    mine = [e[2] for e in want if e[:2] == run[0][:2]]
    assert mine == sorted(mine) and len(mine) == 1000 + np.unique(new_vals).size


def test_add_splits_a_forged_run(eng):
    keys, dig = forged_run(47, 1200)
    even = np.arange(1200) % 2 == 0
    entries = holders_index(keys[even], dig[even], [1 + i % 3 for i in range(600)])
    rng = np.random.default_rng(48)
    other_k, other_d = R.random_pairs(rng, 50)
    # the odd digests arrive, each once or twice with values of their own; some old triples hit
    k = np.concatenate([keys[~even], keys[~even][:200], keys[even][:100], other_k])
    d = np.concatenate([dig[~even], dig[~even][:200], dig[even][:100], other_d])
    v = np.concatenate([np.full(600, 3), np.full(200, 2), np.full(100, 100), np.arange(50)]).astype(np.uint64)
    p = rng.permutation(len(k))
    want, flags, counts = add_both(eng, entries, 4, k[p], d[p], v[p])
    assert counts["added"] == 850 and counts["hits"] == 100
    run = [e for e in want if e[0] == 0x1234567890ABCDEF]
    assert sorted({e[1][30] * 256 + e[1][31] for e in run}) == list(range(1200))


@pytest.mark.parametrize("bits", [(3, 6), (6, 0), (0, 9)])
def test_add_grows_across_a_re_bucket(eng, pool, bits):
    keys, dig = pool
    entries = holders_index(keys[:60], dig[:60], [2] * 60)
    k, d = np.concatenate([keys[50:250], keys[:30]]), np.concatenate([dig[50:250], dig[:30]])
    add_both(eng, entries, bits[0], k, d, np.full(230, 103, np.uint64), None, bits[1])


def test_add_values_null_and_valid_with_holes(eng, pool):
    keys, dig = pool
    entries = sorted((int(k), d.tobytes(), 0) for k, d in zip(keys[:30], dig[:30]))
    pick = np.random.default_rng(49).integers(0, 80, 200)
    want, flags, counts = add_both(eng, entries, 2, keys[pick], dig[pick], None)  # values NULL: every value is 0
    assert all(e[2] == 0 for e in want) and counts["hits"] == int((pick < 30).sum())
    valid = (np.random.default_rng(50).random(200) > 0.3).astype(np.uint8)
    valid[:3] = 0
    want, flags, counts = add_both(eng, entries, 2, keys[pick], dig[pick], pick.astype(np.uint64) % 3, valid)
    assert (flags[valid == 0] == H.SKIPPED).all() and counts["queries"] == int(valid.sum())
    add_both(eng, entries, 2, keys[pick], dig[pick], pick.astype(np.uint64), np.zeros(200, np.uint8))  # none valid


@pytest.mark.parametrize("n_old", [255, 256, 257])
@pytest.mark.parametrize("m", [1, 256])
def test_add_around_a_workgroup(eng, pool, n_old, m):
    keys, dig = pool
    runs = [1 + i % 2 for i in range(200)]
    entries = holders_index(keys[:200], dig[:200], runs)[:n_old]
    pick = np.random.default_rng(n_old + m).integers(0, 400, m)
    add_both(eng, entries, R.dir_bits(n_old), keys[pick], dig[pick], 100 + 7 * (pick % 3).astype(np.uint64))


def test_add_null_outputs_and_errors(eng, pool):
    keys, dig = pool
    entries = holders_index(keys[:25], dig[:25], [2] * 25)
    for outputs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        dev_add(eng, entries, 3, keys[10:70], dig[10:70], np.full(60, 107), None, 4, outputs)
    ix = index_guards(entries, 3)
    bt = batch_guards(keys[:8], dig[:8], None)
    new = [Guarded(8 * 58, align=8, fill=FILL), Guarded(32 * 58, align=16, fill=FILL),
           Guarded(8 * 58, align=8, fill=FILL), Guarded(4 * 9, align=4, fill=FILL)]
    torch.cuda.synchronize()

    def call(new_keys=new[0].ptr, new_dig=new[1].ptr, new_dir=new[3].ptr, m=8):
        with pytest.raises(N.SdcasError) as ei:
            eng.dev_chunk_holders_add(ix[0].ptr, ix[1].ptr, ix[2].ptr, ix[3].ptr, 50, 3, bt[0].ptr, bt[1].ptr, 0, 0, m,
                                      new_keys, new_dig, new[2].ptr, new_dir, 3)
        return ei.value.code

    assert call(new_keys=ix[0].ptr) == N.SDCAS_E_INVALID
    assert call(new_keys=ix[0].ptr + 8 * 49) == N.SDCAS_E_INVALID
    assert call(new_dig=ix[1].ptr) == N.SDCAS_E_INVALID
    assert call(new_dir=ix[3].ptr + 4 * 8) == N.SDCAS_E_INVALID
    assert call(new_dig=new[1].ptr + 8) == N.SDCAS_E_INVALID
    assert call(m=(1 << 30) - 49) == N.SDCAS_E_CAPACITY
    eng.dev_sync()
    torch.cuda.synchronize()
    assert all(g.untouched() and g.check() == [] for g in new)
    assert all(g.unchanged() for g in ix + bt)


# ---- remove -----------------------------------------------------------------------------

def dev_remove(eng, entries, bits_old, removed, bits_new, counts_out=True):
    n, r = len(entries), len(removed)
    ix = index_guards(entries, bits_old)
    gr = guarded_from(np.asarray(removed, np.uint64), align=8)
    new = [Guarded(8 * n, align=8, fill=FILL), Guarded(32 * n, align=16, fill=FILL),
           Guarded(8 * n, align=8, fill=FILL), Guarded(4 * ((1 << bits_new) + 1), align=4, fill=FILL)]
    gc = Guarded(32, align=8, fill=FILL)
    torch.cuda.synchronize()
    eng.dev_chunk_holders_remove(ptr(ix[0]), ptr(ix[1]), ptr(ix[2]), ptr(ix[3], n > 0), n, bits_old, ptr(gr), r,
                                 ptr(new[0]), ptr(new[1]), ptr(new[2]), new[3].ptr, bits_new, ptr(gc, counts_out))
    eng.dev_sync()
    torch.cuda.synchronize()
    for g in ix + [gr, gc] + new:
        assert g.check() == []
    assert all(g.unchanged() for g in ix + [gr])
    if not counts_out:
        assert gc.untouched()
    return new, dict(zip(REMOVE_COUNTS, (int(x) for x in gc.download(np.uint64)))) if counts_out else None


def remove_both(eng, entries, bits_old, removed, bits_new=None):
    removed = np.asarray(removed, np.uint64)
    bits_new = bits_old if bits_new is None else bits_new
    want, wcounts = H.remove(entries, removed)
    wk, wd, wv, wdir, _ = H.arrays(want, bits_new)
    e = len(want)
    (nk, nd, nv, ndir, nb), counts = eng.chunk_holders_remove(H.arrays(entries, bits_old), removed, bits_new)
    assert counts == wcounts and nb == bits_new
    assert (nk == wk).all() and (nd == wd).all() and (nv == wv).all() and (ndir == wdir).all()
    new, counts = dev_remove(eng, entries, bits_old, removed, bits_new)
    assert counts == wcounts
    assert (new[0].download(np.uint64, e) == wk).all() and (new[1].download(np.uint8, 32 * e).reshape(-1, 32) == wd).all()
    assert (new[2].download(np.uint64, e) == wv).all() and (new[3].download(np.uint32) == wdir).all()
    assert new[0].untouched(8 * e) and new[1].untouched(32 * e) and new[2].untouched(8 * e)
    assert_index(want, bits_new)
    return want, wcounts


def shared_index(pool, n, n_files=9, seed=0):
    """n entries: pairs held by 1 to n_files files with ids 10, 20, ..."""
    keys, dig = pool
    rng = np.random.default_rng(seed)
    entries = set()
    i = 0
    while len(entries) < n:
        for f in rng.permutation(n_files)[:rng.integers(1, n_files + 1)]:
            if len(entries) < n:
                entries.add((int(keys[i % 400]), dig[i % 400].tobytes(), 10 * (int(f) + 1) + 1000 * (i // 400)))
        i += 1
    return sorted(entries)


@pytest.mark.parametrize("n_old", [1, 255, 256, 257, 513])
def test_remove_around_a_workgroup(eng, pool, n_old):
    entries = shared_index(pool, n_old, seed=n_old)
    ids = sorted({e[2] for e in entries})
    bits = R.dir_bits(n_old)
    remove_both(eng, entries, bits, [])  # r = 0: copied
    want, counts = remove_both(eng, entries, bits, ids)  # everything removed
    assert want == [] and counts["entries_new"] == 0
    # nothing removed: ids that are absent, below the lowest value and above the highest
    want, _ = remove_both(eng, entries, bits, [0, 5, 15, 25, 10 ** 6, U64_MAX])
    assert want == entries
    want, _ = remove_both(eng, entries, bits, [7] + ids[::2])
    assert len(want) < n_old or n_old == 1
    # only the first entry, only the last: an id below every other and one above
    for at, victim in ((0, 1), (n_old - 1, 10 ** 7)):
        one = [(k, d, victim if i == at else v) for i, (k, d, v) in enumerate(entries)]
        assert H.check(one) == (0, None)
        want, counts = remove_both(eng, one, bits, [victim])
        assert counts["removed"] == 1 and want == one[:at] + one[at + 1:]


def test_remove_crosses_the_second_scan_level(eng, pool):
    """70 000 entries are 274 workgroups of 256: more than the 256 counts one
    workgroup scans, so the second level of the block scan carries a sum"""
    keys, dig = R.random_pairs(np.random.default_rng(51), 10000)
    rng = np.random.default_rng(52)
    runs = rng.integers(2, 14, 10000)
    vals = [np.sort(rng.permutation(40)[:r]) for r in runs]
    order = np.lexsort([dig[:, j] for j in range(31, -1, -1)] + [keys])
    n = 70000
    ks = np.repeat(keys[order], runs[order])[:n]
    ds = np.repeat(dig[order], runs[order], axis=0)[:n]
    vs = np.concatenate([vals[i] for i in order]).astype(np.uint64)[:n]
    assert ks.size == n
    removed = np.sort(rng.permutation(40)[:17]).astype(np.uint64)
    keep = ~np.isin(vs, removed)
    entries = R.from_arrays(ks, ds, vs)
    for bits_old, bits_new in ((R.dir_bits(n), R.dir_bits(n)), (0, 12)):
        want, counts = remove_both(eng, entries, bits_old, removed, bits_new)
        e = int(keep.sum())
        assert counts == dict(entries_old=n, removed=n - e, entries_new=e, values=17)
        k, d, v, _, _ = H.arrays(want, bits_new)
        assert (k == ks[keep]).all() and (d == ds[keep]).all() and (v == vs[keep]).all()


def test_remove_shifts_the_lowest_holder(eng, pool):
    """id 20 is the lowest holder of some pairs and a later holder of others: a
    following match returns the next survivor and a count one lower"""
    keys, dig = pool
    entries = sorted([(int(keys[i]), dig[i].tobytes(), v) for i in range(40)
                      for v in ([20, 30, 40] if i % 3 == 0 else [10, 20, 30] if i % 3 == 1 else [10, 30])])
    bits = R.dir_bits(len(entries))
    _, val0, hold0, _ = H.match(entries, keys[:40], dig[:40])
    want, _ = remove_both(eng, entries, bits, [20])
    pos, hold, _ = match_both(eng, want, bits, keys[:40], dig[:40])
    _, val, _, _ = eng.chunk_holders_match(H.arrays(want, bits), keys[:40], dig[:40])
    i = np.arange(40)
    assert (val == np.where(i % 3 == 0, 30, 10)).all() and (val0 == np.where(i % 3 == 0, 20, 10)).all()
    assert (hold == hold0 - (i % 3 != 2)).all()


def test_remove_every_second_of_a_run_of_1000_and_across_a_boundary(eng, pool):
    keys, dig = pool
    order = np.argsort(keys[:10], kind="stable")
    run = [(int(keys[order[5]]), dig[order[5]].tobytes(), v) for v in range(1000)]
    entries = sorted(run + holders_index(keys[order[:5]], dig[order[:5]], [50] * 5, first_value=0))
    # the 250 entries before the run put it across the boundaries at 256, 512, 768 and 1024
    assert entries[250] == run[0] and entries[255][:2] == entries[256][:2]
    want, counts = remove_both(eng, entries, 3, np.arange(0, 1000, 2))
    assert counts["removed"] == 500 + sum(1 for e in entries[:250] if e[2] % 2 == 0)
    # removals on both sides of the boundary at 256 only
    want, counts = remove_both(eng, entries, 3, [3, 4, 5, 6, 7, 8])  # entries 253..258
    assert counts["removed"] == 6 + 5 and entries[255] not in want and entries[256] not in want


def test_remove_extreme_ids_and_widths(eng, pool):
    keys, dig = pool
    entries = sorted((int(k), d.tobytes(), v) for k, d in zip(keys[:50], dig[:50]) for v in (0, 77, U64_MAX))
    for removed in ([0], [U64_MAX], [0, U64_MAX], [0, 77, U64_MAX]):
        want, counts = remove_both(eng, entries, 4, removed)
        assert counts["removed"] == 50 * len(removed)
    for bits_old, bits_new in ((5, 2), (5, 5), (5, 9), (3, 0), (0, 0), (0, 6)):
        remove_both(eng, entries, bits_old, [77], bits_new)
    # the counts NULL; an empty index
    dev_remove(eng, entries, 4, [77], 4, counts_out=False)
    want, counts = remove_both(eng, [], 0, [1, 2, 3], 2)
    assert want == [] and counts == dict(entries_old=0, removed=0, entries_new=0, values=3)


def test_remove_errors_before_anything_is_enqueued(eng, pool):
    entries = shared_index(pool, 60)
    ix = index_guards(entries, 3)
    gr = guarded_from(np.array([10, 20, 30], np.uint64), align=8)
    new = [Guarded(8 * 60, align=8, fill=FILL), Guarded(32 * 60, align=16, fill=FILL),
           Guarded(8 * 60, align=8, fill=FILL), Guarded(4 * 9, align=4, fill=FILL)]
    torch.cuda.synchronize()

    def call(new_keys=new[0].ptr, new_dig=new[1].ptr, new_vals=new[2].ptr, new_dir=new[3].ptr, removed=gr.ptr, r=3,
             n=60, bits_new=3):
        with pytest.raises(N.SdcasError) as ei:
            eng.dev_chunk_holders_remove(ix[0].ptr, ix[1].ptr, ix[2].ptr, ix[3].ptr, n, 3, removed, r, new_keys,
                                         new_dig, new_vals, new_dir, bits_new)
        return ei.value.code

    assert call(new_keys=ix[0].ptr) == N.SDCAS_E_INVALID
    assert call(new_vals=ix[2].ptr + 8 * 59) == N.SDCAS_E_INVALID
    assert call(new_dig=ix[1].ptr) == N.SDCAS_E_INVALID
    assert call(new_dir=ix[3].ptr + 4 * 8) == N.SDCAS_E_INVALID
    assert call(new_keys=gr.ptr + 16) == N.SDCAS_E_INVALID  # `removed` under the new keys
    assert call(new_dig=new[1].ptr + 8) == N.SDCAS_E_INVALID
    assert call(removed=gr.ptr + 4) == N.SDCAS_E_INVALID
    assert call(removed=0) == N.SDCAS_E_INVALID
    assert call(r=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    assert call(n=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    assert call(bits_new=29) == N.SDCAS_E_CAPACITY
    eng.dev_sync()
    torch.cuda.synchronize()
    assert all(g.untouched() and g.check() == [] for g in new)
    assert all(g.unchanged() for g in ix + [gr])


# ---- laws on the device -------------------------------------------------------------------

def law_corpus(seed, n_files=10):
    rng = np.random.default_rng(seed)
    keys, dig = R.random_pairs(rng, 120)
    keys[:30] = keys[0]  # a forged run among them
    files = {}
    for f in range(n_files):
        pick = list(rng.integers(0, 120, rng.integers(1, 60))) + [0, 1, 0, 40]
        files[5 + 2 * f] = H.batch_arrays([(int(keys[c]), dig[c].tobytes(), 5 + 2 * f) for c in pick])
    return files


def batch_of(files, ids):
    if not ids:
        return np.zeros(0, np.uint64), np.zeros((0, 32), np.uint8), np.zeros(0, np.uint64)
    return tuple(np.concatenate([files[f][j] for f in ids]) for j in range(3))


def index_bytes(ix):
    k, d, v, dr, bits = ix.arrays()
    return k.tobytes(), d.tobytes(), v.tobytes(), dr.tobytes(), bits


@pytest.mark.parametrize("cuts", [[0, 4, 10], [0, 1, 2, 7, 10]])
def test_remove_after_adds_equals_the_index_of_the_rest(eng, tmp_path, cuts):
    """law (a) through real adds in two batch splits, with a save and a load in
    the middle, and law (b) as a bytes-equal round trip"""
    files = law_corpus(61)
    ids = sorted(files)
    ix = ChunkHolders(eng)
    ref = []
    for step, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        k, d, v = batch_of(files, ids[lo:hi])
        ref, wpos, wflags, wcounts = H.add(ref, k, d, v)
        pos, flags, counts = ix.add(k, d, v)
        assert (pos == wpos).all() and (flags == wflags).all() and counts == wcounts and ix.n == len(ref)
        if step == 0:
            ix.save(tmp_path / "holders.npz")
            ix = ChunkHolders.load(eng, tmp_path / "holders.npz")
    gone = [ids[0], ids[3], ids[4], ids[9]]
    counts = ix.remove(gone[::-1] + gone[:1])  # unsorted, one id twice: remove sorts them and makes them distinct
    want, wcounts = H.remove(ref, gone)
    assert counts == wcounts
    k, d, v, dr, bits = ix.arrays()
    assert R.from_arrays(k, d, v) == want == H.build(*batch_of(files, [f for f in ids if f not in gone]))
    assert dr.tolist() == H.directory(want, bits)
    rebuilt = ChunkHolders(eng)
    rebuilt.add(*batch_of(files, [f for f in ids if f not in gone]))
    assert index_bytes(ix)[:3] == index_bytes(rebuilt)[:3]
    # law (b): a new file's triples added, then that file removed, at the same width
    before = index_bytes(ix)
    extra = H.batch_arrays([(int(k[0]), d[0].tobytes(), 999), (int(k[-1]), d[-1].tobytes(), 999), (77, bytes(32), 999)])
    _, flags, counts = ix.add(*extra)
    assert counts["added"] == 3
    ix.remove([999], bits_new=before[4])
    assert index_bytes(ix) == before
    # match on the resident index after all that
    qk, qd, _ = batch_of(files, ids)
    pos, val, hold, counts = ix.match(qk, qd)
    wpos, wval, whold, wcounts = H.match(want, qk, qd)
    assert (pos == wpos).all() and (val == wval).all() and (hold == whold).all() and counts == wcounts


def test_load_refuses_what_is_not_a_holders_index(eng, tmp_path):
    keys, dig = R.random_pairs(np.random.default_rng(62), 20)
    entries = holders_index(keys, dig, [2] * 20)
    k, d, v, dr, bits = H.arrays(entries, 2)
    v[5], v[4] = v[4], v[5]  # a run's values descend
    np.savez(tmp_path / "bad.npz", keys=k, digests=d, values=v, dir=dr, bits=np.uint32(bits))
    with pytest.raises(ValueError, match="not a holders index"):
        ChunkHolders.load(eng, tmp_path / "bad.npz")


def test_from_index_adopts_a_chunk_index(eng, tmp_path):
    """a ChunkIndex filled by similar_files_indexed, matched with both kinds:
    the same pos and value, and every pair has one holder"""
    rng = np.random.default_rng(63)
    base = rng.integers(0, 256, 60000, dtype=np.uint8)
    blobs = [base, np.concatenate([base[:30000], rng.integers(0, 256, 9000, dtype=np.uint8)]),
             rng.integers(0, 256, 25000, dtype=np.uint8)]
    paths = []
    for i, b in enumerate(blobs):
        paths.append(str(tmp_path / f"f{i}.bin"))
        open(paths[-1], "wb").write(b.tobytes())
    params = (64, 8, 1024)
    ci = ChunkIndex(eng)
    eng.similar_files_indexed(paths[:2], [11, 12], ci, params)
    ch = ChunkHolders.from_index(ci)
    assert ch.n == ci.n > 0 and ch.bits == ci.bits
    for a, b in zip(ci.arrays(), ch.arrays()):
        assert np.array_equal(a, b)
    chunks = [w for w in eng.chunk_stream(paths, 1 << 20, params)]
    qk = np.concatenate([w["keys"] for w in chunks])
    qd = np.concatenate([w["digests"] for w in chunks])
    pos, val, counts = ci.match(qk, qd)
    hpos, hval, hold, hcounts = ch.match(qk, qd)
    assert (pos == hpos).all() and (val == hval).all() and counts == hcounts
    assert counts["hits"] > 0 and counts["misses"] > 0 and (hold == (pos >= 0)).all()
    # the copy is its own: the chunk index going on leaves it alone
    eng.similar_files_indexed(paths[2:], [13], ci, params)
    assert ch.n < ci.n
