"""The chunk index on the GPU (sdcas_chunk_index_match / _add and their device
forms, csrc/chunk_index.hip) against the Python reference of
tests/_chunk_index_ref.py: through the host call and through the device call
over guarded buffers (inputs unchanged, guards intact, NULL outputs untouched).
Every comparison is exact equality. No test hands the device a malformed
index."""
import numpy as np
import pytest
import torch

from spacedrive_amd import ChunkIndex, _native as N
from tests import _chunk_index_ref as R
from tests._guarded import Guarded, guarded_from

pytestmark = pytest.mark.gpu

FILL = 0xFE
MATCH_COUNTS = ("queries", "hits", "misses", "skipped")
ADD_COUNTS = ("queries", "hits", "added", "batch_duplicates", "entries_old", "entries_new")
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def index_guards(entries, bits):
    """the four arrays of an index as guarded device inputs (None for an empty one)"""
    keys, dig, values, d, _ = R.arrays(entries, bits)
    return [guarded_from(keys, align=8), guarded_from(dig, align=16), guarded_from(values, align=8),
            guarded_from(d, align=4)]


def batch_guards(keys, dig, valid):
    gs = [guarded_from(np.asarray(keys, np.uint64), align=8), guarded_from(np.asarray(dig, np.uint8), align=16)]
    if valid is not None:
        gs.append(guarded_from(np.asarray(valid, np.uint8), align=1))
    return gs


def ptr(g, used=True):
    return g.ptr if used and g.nbytes else 0


def dev_match(eng, entries, bits, keys, dig, valid=None, outputs=(True, True, True)):
    m, n = len(keys), len(entries)
    ix, bt = index_guards(entries, bits), batch_guards(keys, dig, valid)
    outs = [Guarded(8 * m, align=8, fill=FILL), Guarded(8 * m, align=8, fill=FILL), Guarded(32, align=8, fill=FILL)]
    torch.cuda.synchronize()
    eng.dev_chunk_index_match(ptr(ix[0]), ptr(ix[1]), ptr(ix[2]), ptr(ix[3], n > 0), n, bits, ptr(bt[0]), ptr(bt[1]),
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
    return outs[0].download(np.int64), outs[1].download(np.uint64), \
        dict(zip(MATCH_COUNTS, (int(x) for x in outs[2].download(np.uint64))))


def match_both(eng, entries, bits, keys, dig, valid=None):
    keys, dig = np.asarray(keys, np.uint64), np.asarray(dig, np.uint8).reshape(-1, 32)
    wpos, wval, wcounts = R.match(entries, keys, dig, valid)
    pos, val, counts = eng.chunk_index_match(R.arrays(entries, bits), keys, dig, valid)
    assert (pos == wpos).all() and (val == wval).all() and counts == wcounts
    pos, val, counts = dev_match(eng, entries, bits, keys, dig, valid)
    assert (pos == wpos).all() and (val == wval).all() and counts == wcounts
    return wpos, wcounts


def widths(n):
    return sorted({0, R.dir_bits(n), 3})


def entries_of(keys, dig, first_value=100):
    return R.build(keys, dig, np.arange(first_value, first_value + len(keys), dtype=np.uint64))


# ---- match ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pool():
    """300 distinct random pairs with real keys: entries come from the front, misses from the back"""
    return R.random_pairs(np.random.default_rng(11), 300)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 8, 9])
def test_match_small_indexes(eng, pool, n):
    keys, dig = pool
    entries = entries_of(keys[:n], dig[:n])
    rng = np.random.default_rng(n)
    for bits in widths(n):
        for m in (0, 1, 255, 256, 257):
            # every entry queried (when m allows), the rest misses, shuffled
            pick = np.concatenate([np.arange(n), 20 + np.arange(max(m - n, 0))])[:m]
            pick = pick[rng.permutation(m)]
            pos, counts = match_both(eng, entries, bits, keys[pick], dig[pick])
            assert counts["hits"] == int((pick < n).sum()) and (pos >= 0).sum() == counts["hits"]


def test_match_1000_entries_at_8_bits(eng):
    keys, dig = R.random_pairs(np.random.default_rng(12), 1350)
    entries = entries_of(keys[:1000], dig[:1000])
    d = R.directory(entries, 8)
    sizes = np.diff(d)
    assert (sizes == 0).any() and (sizes >= 2).any()  # empty and multi-entry buckets
    pick = np.random.default_rng(13).permutation(np.concatenate([np.arange(350), 1000 + np.arange(350)]))
    _, counts = match_both(eng, entries, 8, keys[pick], dig[pick])
    assert counts == dict(queries=700, hits=350, misses=350, skipped=0)
    # NULL outputs, one at a time
    for outputs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        dev_match(eng, entries, 8, keys[pick], dig[pick], None, outputs)


def test_match_extreme_keys(eng, pool):
    _, dig = pool
    keys = np.array([0, 0, U64_MAX, U64_MAX, 1, U64_MAX - 1], np.uint64)
    entries = entries_of(keys, dig[:6])
    q_keys = np.array([0, U64_MAX, 0, U64_MAX, 1, 2, U64_MAX - 1, U64_MAX - 2], np.uint64)
    q_dig = np.stack([dig[0], dig[2], dig[9], dig[9], dig[4], dig[4], dig[5], dig[5]])
    for bits in (0, 1, 3, 6):
        pos, counts = match_both(eng, entries, bits, q_keys, q_dig)
        assert counts["hits"] == 4 and (pos >= 0).tolist() == [True, True, False, False, True, False, True, False]
    # as misses against an index that holds neither
    entries = entries_of(np.array([5, 1 << 63], np.uint64), dig[:2])
    match_both(eng, entries, 3, np.array([0, U64_MAX], np.uint64), dig[:2])


def test_match_one_bucket_holds_everything(eng):
    rng = np.random.default_rng(14)
    _, dig = R.random_pairs(rng, 600)
    keys = (np.uint64(0xA) << np.uint64(60)) | rng.integers(0, 1 << 59, 600).astype(np.uint64)  # top 4 bits 1010
    entries = entries_of(keys[:500], dig[:500])
    d = R.directory(entries, 4)
    assert d[10] == 0 and d[11] == 500
    pick = rng.permutation(600)
    _, counts = match_both(eng, entries, 4, keys[pick], dig[pick])
    assert counts["hits"] == 500


@pytest.mark.parametrize("byte", [31, 0])
def test_match_one_forged_key(eng, byte):
    """300 entries under one key, their digests differing in one byte only
    (even values); the odd values in between miss"""
    base = np.random.default_rng(15).integers(0, 256, 32, dtype=np.uint8)
    # 300 even values need more than one byte: bytes `byte` and its neighbour
    other = 30 if byte == 31 else 1
    dig = np.tile(base, (600, 1))
    v = np.arange(600)
    if byte == 31:
        dig[:, 31], dig[:, other] = v & 0xFF, v >> 8
    else:
        dig[:, 0], dig[:, other] = v >> 8, v & 0xFF
    keys = np.full(600, 0x1234567890ABCDEF, np.uint64)
    even = v % 2 == 0
    entries = entries_of(keys[even], dig[even])
    assert len(entries) == 300
    pick = np.random.default_rng(16).permutation(600)
    for bits in (0, 5):
        pos, counts = match_both(eng, entries, bits, keys[pick], dig[pick])
        assert counts["hits"] == 300 and ((pos >= 0) == even[pick]).all()


def test_match_orders_digests_by_bytes(eng):
    a, b = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    a[3], b[0] = 1, 1  # 00 00 00 01 orders before 01 00 00 00
    keys = np.array([5, 5], np.uint64)
    entries = R.build(keys, np.stack([b, a]), [7, 8])
    assert [e[2] for e in entries] == [8, 7]
    pos, _ = match_both(eng, entries, 0, keys, np.stack([a, b]))
    assert pos.tolist() == [0, 1]
    # with more entries around them, so that the search has to order them
    rng = np.random.default_rng(17)
    dig = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    dig[:, :3] = 0
    dig[:20, 3], dig[20:, 0] = np.arange(1, 21), np.arange(1, 21)
    dig[20:, 3] = 0
    keys = np.full(40, 5, np.uint64)
    entries = entries_of(keys[::2], dig[::2])
    pos, counts = match_both(eng, entries, 0, keys, dig)
    assert counts["hits"] == 20 and ((pos >= 0) == (np.arange(40) % 2 == 0)).all()


def test_match_valid_mask(eng, pool):
    keys, dig = pool
    entries = entries_of(keys[:100], dig[:100])
    valid = (np.random.default_rng(18).random(150) > 0.4).astype(np.uint8)
    pos, counts = match_both(eng, entries, R.dir_bits(100), keys[:150], dig[:150], valid)
    assert counts["skipped"] == int((valid == 0).sum()) and (pos[valid == 0] == -1).all()


def test_match_errors_before_anything_is_enqueued(eng, pool):
    keys, dig = pool
    entries = entries_of(keys[:10], dig[:10])
    ix, bt = index_guards(entries, 2), batch_guards(keys[:5], dig[:5], None)
    outs = [Guarded(40, align=8, fill=FILL), Guarded(40, align=8, fill=FILL), Guarded(32, align=8, fill=FILL)]
    torch.cuda.synchronize()

    def call(idx_dig=ix[1].ptr, q_dig=bt[1].ptr, n=10, bits=2, m=5):
        with pytest.raises(N.SdcasError) as ei:
            eng.dev_chunk_index_match(ix[0].ptr, idx_dig, ix[2].ptr, ix[3].ptr, n, bits, bt[0].ptr, q_dig, 0, m,
                                      outs[0].ptr, outs[1].ptr, outs[2].ptr)
        return ei.value.code

    assert call(idx_dig=ix[1].ptr + 8) == N.SDCAS_E_INVALID
    assert call(q_dig=bt[1].ptr + 4) == N.SDCAS_E_INVALID
    assert call(n=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    assert call(m=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    assert call(bits=29) == N.SDCAS_E_CAPACITY
    eng.dev_sync()
    torch.cuda.synchronize()
    assert all(o.untouched() and o.check() == [] for o in outs)


# ---- add --------------------------------------------------------------------------------

def dev_add(eng, entries, bits_old, keys, dig, values, valid, bits_new, outputs=(True, True, True)):
    """sdcas_dev_chunk_index_add over guarded buffers -> (new entries, pos, flags, counts)"""
    m, n = len(keys), len(entries)
    cap = n + m
    ix, bt = index_guards(entries, bits_old), batch_guards(keys, dig, valid)
    gv = guarded_from(np.asarray(values, np.uint64), align=8)
    new = [Guarded(8 * cap, align=8, fill=FILL), Guarded(32 * cap, align=16, fill=FILL),
           Guarded(8 * cap, align=8, fill=FILL), Guarded(4 * ((1 << bits_new) + 1), align=4, fill=FILL)]
    outs = [Guarded(8 * m, align=8, fill=FILL), Guarded(m, align=1, fill=FILL), Guarded(48, align=8, fill=FILL)]
    torch.cuda.synchronize()
    eng.dev_chunk_index_add(ptr(ix[0]), ptr(ix[1]), ptr(ix[2]), ptr(ix[3], n > 0), n, bits_old, ptr(bt[0]), ptr(bt[1]),
                            ptr(gv), bt[2].ptr if valid is not None and m else 0, m, ptr(new[0]), ptr(new[1]),
                            ptr(new[2]), new[3].ptr, bits_new, *(ptr(o, outputs[j]) for j, o in enumerate(outs)))
    eng.dev_sync()
    torch.cuda.synchronize()
    for g in ix + bt + [gv] + new + outs:
        assert g.check() == []
    assert all(g.unchanged() for g in ix + bt + [gv])
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {j} was written"
    counts = dict(zip(ADD_COUNTS, (int(x) for x in outs[2].download(np.uint64)))) if outputs[2] else None
    return new, outs[0].download(np.int64), outs[1].download(np.uint8), counts


def add_both(eng, entries, bits_old, keys, dig, values, valid=None, bits_new=None):
    keys, dig = np.asarray(keys, np.uint64), np.asarray(dig, np.uint8).reshape(-1, 32)
    values = np.asarray(values, np.uint64)
    m, n = len(keys), len(entries)
    if bits_new is None:
        bits_new = R.dir_bits(n + m)
    want, wpos, wflags, wcounts = R.add(entries, keys, dig, values, valid)
    wk, wd, wv, wdir, _ = R.arrays(want, bits_new)
    e = len(want)
    # the host call
    (nk, nd, nv, ndir, nb), pos, flags, counts = eng.chunk_index_add(R.arrays(entries, bits_old), keys, dig, values,
                                                                     valid, bits_new)
    assert counts == wcounts and nb == bits_new
    assert (nk == wk).all() and (nd == wd).all() and (nv == wv).all() and (ndir == wdir).all()
    assert (pos == wpos).all() and (flags == wflags).all()
    # the device call
    new, pos, flags, counts = dev_add(eng, entries, bits_old, keys, dig, values, valid, bits_new)
    assert counts == wcounts
    assert (new[0].download(np.uint64, e) == wk).all() and (new[1].download(np.uint8, 32 * e).reshape(-1, 32) == wd).all()
    assert (new[2].download(np.uint64, e) == wv).all() and (new[3].download(np.uint32) == wdir).all()
    assert (pos == wpos).all() and (flags == wflags).all()
    # entries past entries_new are left as they were
    assert new[0].untouched(8 * e) and new[1].untouched(32 * e) and new[2].untouched(8 * e)
    ok = wpos >= 0
    assert (wk[wpos[ok]] == keys[ok]).all()  # new.keys[out_pos[c]] == keys[c] for every valid c
    assert (N.load().sdcas_chunk_index_check(wk.ctypes.data if e else None, wd.ctypes.data if e else None,
                                             wdir.ctypes.data, e, bits_new, None)) == N.SDCAS_OK
    return want, wflags, wcounts


def test_add_to_an_empty_index(eng, pool):
    keys, dig = pool
    pick = np.array([3, 1, 3, 2, 1, 3, 0, 2])
    values = np.arange(50, 58, dtype=np.uint64)
    want, flags, counts = add_both(eng, [], 0, keys[pick], dig[pick], values)
    assert flags.tolist() == [2, 2, 0, 2, 0, 0, 2, 0]
    assert sorted(e[2] for e in want) == [50, 51, 53, 56]  # the lowest position's value
    assert counts == dict(queries=8, hits=0, added=4, batch_duplicates=4, entries_old=0, entries_new=4)
    add_both(eng, [], 0, keys[:0], dig[:0], values[:0])  # nothing into nothing
    add_both(eng, want, 0, keys[:0], dig[:0], values[:0], bits_new=3)  # nothing added: re-bucketed


def batch_600(rng, old_keys, old_dig, new_keys, new_dig):
    """200 hits, 300 positions over 200 new pairs (100 of them later copies),
    100 invalid (hits and new pairs among them), shuffled"""
    hits = rng.permutation(len(old_keys))[:200]
    keys = np.concatenate([old_keys[hits], new_keys[:200], new_keys[:100], old_keys[:50], new_keys[200:250]])
    dig = np.concatenate([old_dig[hits], new_dig[:200], new_dig[:100], old_dig[:50], new_dig[200:250]])
    valid = np.concatenate([np.ones(500, np.uint8), np.zeros(100, np.uint8)])
    p = rng.permutation(600)
    return keys[p], dig[p], valid[p], (9000 + np.arange(600)).astype(np.uint64)


@pytest.mark.parametrize("where", ["interleaved", "below", "above"])
def test_add_600_to_1000(eng, where):
    rng = np.random.default_rng(21)
    keys, dig = R.random_pairs(rng, 1250)
    old, new = np.arange(1000), 1000 + np.arange(250)
    if where != "interleaved":  # every new key below (above) every old one
        top = np.uint64(1) << np.uint64(63)
        keys = keys >> np.uint64(1)
        keys[old if where == "below" else new] |= top
    entries = entries_of(keys[old], dig[old])
    bk, bd, valid, values = batch_600(rng, keys[old], dig[old], keys[new], dig[new])
    want, flags, counts = add_both(eng, entries, R.dir_bits(1000), bk, bd, values, valid)
    assert counts == dict(queries=500, hits=200, added=200, batch_duplicates=100, entries_old=1000, entries_new=1200)
    if where == "below":
        assert all(e[2] >= 9000 for e in want[:200])
    if where == "above":
        assert all(e[2] >= 9000 for e in want[1000:])


def test_add_splits_a_forged_run(eng):
    """one key, 300 digests that differ in the last bytes: the even ones are in
    the old index, the odd ones arrive (a run above the in-place cap of 64)"""
    base = np.random.default_rng(22).integers(0, 256, 32, dtype=np.uint8)
    dig = np.tile(base, (300, 1))
    v = np.arange(300)
    dig[:, 31], dig[:, 30] = v & 0xFF, v >> 8
    keys = np.full(300, 0xFEEDFACECAFEBEEF, np.uint64)
    rng = np.random.default_rng(23)
    other_k, other_d = R.random_pairs(rng, 100)
    even, odd = v % 2 == 0, v % 2 == 1
    entries = entries_of(np.concatenate([keys[even], other_k[:50]]), np.concatenate([dig[even], other_d[:50]]))
    p = rng.permutation(250)
    bk = np.concatenate([keys[odd], other_k])[p]
    bd = np.concatenate([dig[odd], other_d])[p]
    want, flags, counts = add_both(eng, entries, 4, bk, bd, 500 + np.arange(250))
    assert counts["added"] == 200 and counts["hits"] == 50
    run = [e for e in want if e[0] == 0xFEEDFACECAFEBEEF]
    assert [e[1][30] * 256 + e[1][31] for e in run] == list(range(300))
    # a run of 70, just above the cap, alone in a batch of 70: an odd number of merge passes
    some = v < 140
    entries = entries_of(keys[even & some], dig[even & some])
    p = rng.permutation(70)
    add_both(eng, entries, 2, keys[odd & some][p], dig[odd & some][p], np.arange(70))
    # a short run (below the cap) with the same shape
    few = v < 40
    entries = entries_of(keys[even & few], dig[even & few])
    add_both(eng, entries, 0, keys[odd & few], dig[odd & few], np.arange(20))


@pytest.mark.parametrize("bits", [(3, 6), (6, 0), (0, 9)])
def test_add_changes_the_width(eng, pool, bits):
    keys, dig = pool
    entries = entries_of(keys[:120], dig[:120])
    add_both(eng, entries, bits[0], keys[100:300], dig[100:300], np.arange(200), None, bits[1])


def test_add_null_outputs_and_errors(eng, pool):
    keys, dig = pool
    entries = entries_of(keys[:50], dig[:50])
    for outputs in ((False, True, True), (True, False, True), (False, False, False)):
        dev_add(eng, entries, 3, keys[30:90], dig[30:90], np.arange(60), None, 4, outputs)
    # overlapping old and new arrays, a batch beyond the limit, misaligned digests
    ix = index_guards(entries, 3)
    bt = batch_guards(keys[:8], dig[:8], None)
    new = [Guarded(8 * 58, align=8, fill=FILL), Guarded(32 * 58, align=16, fill=FILL),
           Guarded(8 * 58, align=8, fill=FILL), Guarded(4 * 9, align=4, fill=FILL)]
    torch.cuda.synchronize()

    def call(new_keys=new[0].ptr, new_dig=new[1].ptr, new_dir=new[3].ptr, m=8):
        with pytest.raises(N.SdcasError) as ei:
            eng.dev_chunk_index_add(ix[0].ptr, ix[1].ptr, ix[2].ptr, ix[3].ptr, 50, 3, bt[0].ptr, bt[1].ptr, 0, 0, m,
                                    new_keys, new_dig, new[2].ptr, new_dir, 3)
        return ei.value.code

    assert call(new_keys=ix[0].ptr) == N.SDCAS_E_INVALID
    assert call(new_keys=ix[0].ptr + 8 * 49) == N.SDCAS_E_INVALID  # the last old key under the first new one
    assert call(new_dig=ix[1].ptr) == N.SDCAS_E_INVALID
    assert call(new_dir=ix[3].ptr + 4 * 8) == N.SDCAS_E_INVALID
    assert call(new_dig=new[1].ptr + 8) == N.SDCAS_E_INVALID
    assert call(m=(1 << 30) - 49) == N.SDCAS_E_CAPACITY
    eng.dev_sync()
    torch.cuda.synchronize()
    assert all(g.untouched() and g.check() == [] for g in new)
    assert all(g.unchanged() for g in ix + bt)


def test_five_adds_equal_one(eng):
    rng = np.random.default_rng(24)
    keys, dig = R.random_pairs(rng, 700)
    keys[:90] = keys[0]  # a long run under one key, split over the batches
    pick = rng.integers(0, 700, 1500)
    bk, bd, values = keys[pick], dig[pick], (1 + np.arange(1500)).astype(np.uint64)
    valid = (rng.random(1500) > 0.1).astype(np.uint8)
    want = R.build(bk, bd, values, valid)
    # through ChunkIndex, in five uneven batches
    ix = ChunkIndex(eng)
    cuts = [0, 1, 300, 301, 900, 1500]
    ref = []
    for lo, hi in zip(cuts, cuts[1:]):
        before = len(ref)
        ref, wpos, wflags, wcounts = R.add(ref, bk[lo:hi], bd[lo:hi], values[lo:hi], valid[lo:hi])
        pos, flags, counts = ix.add(bk[lo:hi], bd[lo:hi], values[lo:hi], valid[lo:hi])
        assert (pos == wpos).all() and (flags == wflags).all() and counts == wcounts
        assert ix.n == len(ref) and ix.bits == R.dir_bits(before + hi - lo)
    assert ref == want
    k, d, v, dr, bits = ix.arrays()
    assert R.from_arrays(k, d, v) == want
    assert dr.tolist() == R.directory(want, bits) and len(dr) == (1 << bits) + 1
    # one add of everything
    one = ChunkIndex(eng)
    one.add(bk, bd, values, valid)
    k1, d1, v1, dr1, _ = one.arrays()
    assert R.from_arrays(k1, d1, v1) == want
    # and the match through the resident index
    pos, val, counts = ix.match(bk, bd, valid)
    wpos, wval, wcounts = R.match(want, bk, bd, valid)
    assert (pos == wpos).all() and (val == wval).all() and counts == wcounts


def test_same_add_twice_gives_identical_bytes(eng):
    rng = np.random.default_rng(25)
    keys, dig = R.random_pairs(rng, 900)
    keys[100:200] = keys[100]
    entries = entries_of(keys[:500], dig[:500])
    pick = rng.integers(200, 900, 1200)
    runs = []
    for _ in range(2):
        new, pos, flags, counts = dev_add(eng, entries, 7, keys[pick], dig[pick], np.arange(1200), None, 9)
        runs.append([g.download() for g in new] + [pos, flags, counts])
    for a, b in zip(runs[0][:6], runs[1][:6]):
        assert (a == b).all()
    assert runs[0][6] == runs[1][6]


def test_chunk_confirm_match_on_one_stream(eng):
    """dev_chunk -> dev_confirm_duplicates -> dev_chunk_index_match enqueued on
    one stream with no wait in between (dev_chunk's own wait aside)"""
    rng = np.random.default_rng(26)
    params = (64, 8, 1024)
    block = rng.integers(0, 256, 30000, dtype=np.uint8)  # a multiple of 16: the second file starts aligned
    files = [block.tobytes(), block[:20000].tobytes() + rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()]
    blob, offs, lens = eng.pack(files)
    fc, off, ln, fl, ckeys, cdig, _ = eng.chunk_messages(blob, offs, lens, params)
    first = fl == 0
    entries = R.build(ckeys[first], cdig[first], np.full(int(first.sum()), 77, np.uint64))
    bits = R.dir_bits(len(entries))
    mc, ms = eng.chunk_plan(lens, params)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_blob = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()
        d_offs, d_lens = torch.from_numpy(offs.view(np.int64)).cuda(), torch.from_numpy(lens.view(np.int64)).cuda()
        ik, idg, iv, idr, _ = R.arrays(entries, bits)
        d_ix = [torch.from_numpy(a.view(t).reshape(-1)).cuda()
                for a, t in ((ik, np.int64), (idg, np.uint8), (iv, np.int64), (idr, np.int32))]
        d_keys = torch.zeros(mc, dtype=torch.int64, device="cuda")
        d_dig = torch.zeros(32 * mc, dtype=torch.uint8, device="cuda")
        d_counts = torch.zeros(6, dtype=torch.int64, device="cuda")
        d_rep = torch.zeros(mc, dtype=torch.int64, device="cuda")
        d_pos = torch.zeros(mc, dtype=torch.int64, device="cuda")
        d_val = torch.zeros(mc, dtype=torch.int64, device="cuda")
        d_mc = torch.zeros(4, dtype=torch.int64, device="cuda")
        m = len(ckeys)
        h = s.cuda_stream
        eng.dev_chunk(d_blob.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), 2, mc, ms, params,
                      keys=d_keys.data_ptr(), digests=d_dig.data_ptr(), counts=d_counts.data_ptr(), stream=h)
        eng.dev_confirm_duplicates(d_keys.data_ptr(), d_dig.data_ptr(), 0, m, rep=d_rep.data_ptr(), stream=h)
        eng.dev_chunk_index_match(*(t.data_ptr() for t in d_ix), len(entries), bits, d_keys.data_ptr(),
                                  d_dig.data_ptr(), 0, m, pos=d_pos.data_ptr(), value=d_val.data_ptr(),
                                  counts=d_mc.data_ptr(), stream=h)
        eng.dev_sync(h)
        pos, val = d_pos.cpu().numpy()[:m], d_val.cpu().numpy()[:m].view(np.uint64)
        counts = dict(zip(MATCH_COUNTS, (int(x) for x in d_mc.cpu())))
    assert int(d_counts.cpu()[1]) == m
    wpos, wval, wcounts = R.match(entries, ckeys, cdig)
    assert (pos == wpos).all() and (val == wval).all() and counts == wcounts
    assert counts["hits"] > 0 and counts["misses"] > 0 and (pos[first] >= 0).all()
