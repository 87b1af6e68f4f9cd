"""The index kernels past 2^24 entries and pairs: the third level of the block
scan (csrc/holders_device.h: k_ch_scan, ch_base; csrc/chunk_peers.hip:
k_cp_scan64, cp_before).

A place is l1[b] + l2[b >> 8] + l3[b >> 16] + the rank in workgroup b = item /
256, a byte sum run[p] + s1[p >> 8] + s2[p >> 16] + s3[p >> 24]: l3 and s3 have
an index above 0 only from item T = 2^24 on, and below it l3[0] = s3[0] = 0. The
sizes here are the smallest at which those indexes become 1 and 2, with T itself
as the control; they are conditions, not tunables. Every case first shows from
the reference alone that it uses the level, then compares every output element
on the device, exactly: the inputs are generated on the device and the
references are tests/_index_scale.py's, pinned on the CPU by
tests/test_index_scale_ref.py. Only counts come down."""
import gc

import pytest
import torch

from tests import _index_scale as S

pytestmark = pytest.mark.gpu

T = S.T
BIG = 2 * T + 257
POISON = 0xA5
DEV = "cuda"


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def memory(request):
    """each case's tensors are gone before the next one; its peak is printed"""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"\n{request.node.name}: peak torch memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big():
    """the holders index of 2 T + 257 entries: runs of 1 to 8 holders, one across
    entry T and one across 2 T; the removes take its first n entries"""
    ix = S.gen_index(BIG, S.dir_bits(BIG), DEV)
    assert bool((ix.keys[T - 1] == ix.keys[T]) & (ix.keys[2 * T - 1] == ix.keys[2 * T]))
    assert torch.equal(ix.digests[T - 1], ix.digests[T]) and torch.equal(ix.digests[2 * T - 1], ix.digests[2 * T])
    yield ix
    del ix
    gc.collect()
    torch.cuda.empty_cache()


def poisoned(count, dtype):
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full((count * size,), POISON, dtype=torch.uint8, device=DEV).view(dtype)


def still_poisoned(t, start):
    return bool((t[start:].contiguous().view(torch.uint8) == POISON).all())


def ptr(t):
    return t.data_ptr() if t.numel() else 0


def run(eng, call, *args):
    torch.cuda.synchronize()
    call(*args)
    eng.dev_sync()
    torch.cuda.synchronize()


def same(name, got, want, per_file=False):
    """torch.equal, or the first entry that differs and where it lies in the scan
    (per_file: the rows are files, which no scan places)"""
    assert got.shape == want.shape and got.dtype == want.dtype, name
    if torch.equal(got, want):
        return
    bad = (got != want).reshape(got.shape[0], -1).any(1)
    i = int(torch.nonzero(bad)[0])
    b = i >> 8
    where = f"file {i}" if per_file else (f"entry {i}, {'before' if i < T else 'at or after'} 2^24: "
                                          f"b = i >> 8 = {b}, b >> 8 = {b >> 8}, b >> 16 = {b >> 16}")
    pytest.fail(f"{name}: {int(bad.sum())} of {got.shape[0]} differ, the first at {where}")


def same_index(got, e, want):
    """got: (keys, digests, values, dir) with their poison; want: an Index of e entries"""
    same("keys", got[0][:e], want.keys)
    same("digests", got[1][:e], want.digests)
    same("values", got[2][:e], want.values)
    same("dir", got[3], want.dir)
    assert all(still_poisoned(t, e) for t in got[:3]), "an entry past entries_new was written"


def uses_the_third_level(flag, n, control=False):
    """the reference's flags by place: the flagged among [0, T) are neither none
    nor all, and unless the case is the control some flagged place lies at or
    after T — so l3[1] is a sum that is neither 0 nor a place's own number"""
    below = int(flag[:T].sum())
    assert 0 < below < T, "generator bug: the first 2^24 places hold nothing to count, or everything"
    if control:
        assert n == T
    else:
        assert n > T and bool(flag[T:].any()), "generator bug: nothing is placed from place 2^24 on"


# ---- remove -----------------------------------------------------------------------------------

def removed_values(ix, n):
    """every (z + 2)th id of zone z: a half, a third, a quarter of the holders of
    the runs that begin in [z T, (z + 1) T) — without entry T's own value, so
    that the first entry that reads l3[1] stays"""
    ids = S.holder_ids(DEV)
    removed = torch.cat([ids[::z + 2] + z * S.ZONE_STEP for z in range(3)])
    return removed[removed != ix.values[T]] if n > T else removed


@pytest.mark.parametrize("n", [T, T + 1, T + 769, BIG], ids=["T", "T+1", "T+769", "2T+257"])
def test_remove(eng, big, n):
    """T: the control, l3 stays unused; T + 1: one entry reads l3[1]; 2 T + 257:
    l3[2] is a sum of two, the third launch really scans"""
    bits_old = S.dir_bits(n)
    old = S.Index(big.keys[:n], big.digests[:n], big.values[:n], S.directory(big.keys, n, bits_old), bits_old)
    removed = removed_values(big, n)
    keep, want, wcounts = S.remove(old, removed, bits_old)
    uses_the_third_level(keep, n, control=n == T)
    if n == BIG:  # the keep density differs between the two halves
        assert int(keep[T:2 * T].sum()) > int(keep[:T].sum()) + T // 10
    for bits_new in (bits_old, 12):
        if bits_new != bits_old:
            want = S.Index(want.keys, want.digests, want.values, S.directory(want.keys, want.keys.shape[0], bits_new),
                           bits_new)
        new = (poisoned(n, torch.int64), poisoned(32 * n, torch.uint8).reshape(n, 32), poisoned(n, torch.int64),
               poisoned((1 << bits_new) + 1, torch.int32))
        counts = poisoned(4, torch.int64)
        run(eng, eng.dev_chunk_holders_remove, ptr(old.keys), ptr(old.digests), ptr(old.values), ptr(old.dir), n,
            bits_old, ptr(removed), removed.shape[0], ptr(new[0]), ptr(new[1]), ptr(new[2]), ptr(new[3]), bits_new,
            ptr(counts))
        assert dict(zip(S.REMOVE_COUNTS, counts.tolist())) == wcounts
        same_index(new, wcounts["entries_new"], want)
        del new


# ---- add --------------------------------------------------------------------------------------

def dev_add(eng, call, old, batch, bits_new):
    """-> ((keys, digests, values, dir) with their poison, pos, flags, the six counts)"""
    n_old, m = old.keys.shape[0], batch.keys.shape[0]
    cap = n_old + m
    new = (poisoned(cap, torch.int64), poisoned(32 * cap, torch.uint8).reshape(cap, 32), poisoned(cap, torch.int64),
           poisoned((1 << bits_new) + 1, torch.int32))
    pos, flags, counts = poisoned(m, torch.int64), poisoned(m, torch.uint8), poisoned(6, torch.int64)
    run(eng, call, ptr(old.keys), ptr(old.digests), ptr(old.values), ptr(old.dir) if n_old else 0, n_old, old.bits,
        ptr(batch.keys), ptr(batch.digests), ptr(batch.values), 0, m, ptr(new[0]), ptr(new[1]), ptr(new[2]),
        ptr(new[3]), bits_new, ptr(pos), ptr(flags), ptr(counts))
    return new, pos, flags, dict(zip(S.ADD_COUNTS, counts.tolist()))


def check_add(got, want):
    new, pos, flags, counts = got
    windex, wpos, wflags, wcounts = want
    assert counts == wcounts
    same_index(new, wcounts["entries_new"], windex)
    same("pos", pos, wpos)
    same("flags", flags, wflags)


@pytest.mark.parametrize("m,n_old", [(T + 257, 0), (T + 257, 70001), (BIG, 0)],
                         ids=["T+257_into_0", "T+257_into_70001", "2T+257_into_0"])
def test_add(eng, m, n_old):
    """about 1/2 new triples, 1/4 hits and 1/4 later copies, shuffled: the new
    firsts are counted over the m places of the batch's own order"""
    old = S.gen_index(n_old, S.dir_bits(n_old), DEV)
    batch = S.gen_batch(old, m, DEV)
    bits_new = S.dir_bits(n_old + m)
    *want, fresh = S.add(old, batch, bits_new)
    uses_the_third_level(fresh, m)
    wcounts = want[3]
    assert wcounts["hits"] == (m // 4 if n_old else 0) and wcounts["batch_duplicates"] == m // 4
    check_add(dev_add(eng, eng.dev_chunk_holders_add, old, batch, bits_new), want)


def test_the_two_adds_agree(eng):
    """tests/test_gpu_index_shared.py's law at scale: distinct pairs, the hits
    carry the stored value; the chunk index's add and the holders index's give
    the same bytes, the reference's"""
    m, n_old = T + 257, 70001
    old = S.gen_index(n_old, S.dir_bits(n_old), DEV, runs=(1, 1))
    batch = S.gen_batch(old, m, DEV, distinct_pairs=True)
    bits_new = S.dir_bits(n_old + m)
    *want, fresh = S.add(old, batch, bits_new)
    uses_the_third_level(fresh, m)
    windex, wcounts = want[0], want[3]
    # the preconditions: no triple twice in the batch, no pair twice in old ++ batch
    assert wcounts["batch_duplicates"] == 0 and wcounts["hits"] == n_old  # every old entry once
    assert S.run_starts(windex.keys, windex.digests).shape[0] == wcounts["entries_new"]
    pairs = dev_add(eng, eng.dev_chunk_index_add, old, batch, bits_new)
    check_add(pairs, want)
    triples = dev_add(eng, eng.dev_chunk_holders_add, old, batch, bits_new)
    check_add(triples, want)
    for name, a, b in zip(("keys", "digests", "values", "dir"), pairs[0], triples[0]):
        same(name, a, b)  # with the poison past entries_new: byte for byte


# ---- match ------------------------------------------------------------------------------------

def check_match(eng, ix, holders_too):
    m = 1 << 20
    n = ix.keys.shape[0]
    keys, dig = S.gen_queries(ix, m, DEV)
    wpos, wvalue, wholders, wcounts = S.match(ix, keys, dig)
    assert wcounts["misses"] == m // 4 and int(wpos.min()) == -1
    # the hits lie on both sides of entry T and of entry 2 T, the first and the last run among them
    assert int(wpos.max()) == int(S.run_starts(ix.keys[-64:], ix.digests[-64:])[-1]) + n - 64
    assert bool((wpos == 0).any()) and int(((wpos >= T) & (wpos < 2 * T)).sum()) > m // 8
    pos, value, counts = poisoned(m, torch.int64), poisoned(m, torch.int64), poisoned(4, torch.int64)
    if holders_too:
        holders = poisoned(m, torch.int32)
        run(eng, eng.dev_chunk_holders_match, ptr(ix.keys), ptr(ix.digests), ptr(ix.values), ptr(ix.dir), n, ix.bits,
            ptr(keys), ptr(dig), 0, m, ptr(pos), ptr(value), ptr(holders), ptr(counts))
        same("holders", holders, wholders)
        assert int(wholders.max()) >= 8
    else:
        run(eng, eng.dev_chunk_index_match, ptr(ix.keys), ptr(ix.digests), ptr(ix.values), ptr(ix.dir), n, ix.bits,
            ptr(keys), ptr(dig), 0, m, ptr(pos), ptr(value), ptr(counts))
        assert int(wholders.max()) == 1
    assert dict(zip(S.MATCH_COUNTS, counts.tolist())) == wcounts
    same("pos", pos, wpos)
    same("value", value, wvalue)


def test_holders_match(eng, big):
    """2^20 queries against 2 T + 257 entries: entry numbers need 26 bits"""
    check_match(eng, big, True)


def test_index_match(eng):
    check_match(eng, S.gen_index(BIG, S.dir_bits(BIG), DEV, runs=(1, 1)), False)


# ---- peers ------------------------------------------------------------------------------------

def check_peers(eng, ix, chunks, k, max_holders, mode, max_pairs, want):
    keys, dig, chunk_file, chunk_len, file_ids = chunks
    m, n_files, n = keys.shape[0], file_ids.shape[0], ix.keys.shape[0]
    out = dict(peer_count=poisoned(n_files, torch.int32), peers=poisoned(n_files * k, torch.int64).reshape(n_files, k),
               peer_bytes=poisoned(n_files * k, torch.int64).reshape(n_files, k), shared=poisoned(n_files, torch.int64),
               unique=poisoned(n_files, torch.int64), common=poisoned(n_files, torch.int64))
    counts = poisoned(7, torch.int64)
    run(eng, eng.dev_chunk_peers, ptr(ix.keys), ptr(ix.digests), ptr(ix.values), ptr(ix.dir), n, ix.bits, ptr(keys),
        ptr(dig), 0, ptr(chunk_file), ptr(chunk_len), m, ptr(file_ids), n_files, k, max_holders, mode, max_pairs,
        *(ptr(t) for t in out.values()), ptr(counts))
    assert dict(zip(S.PEERS_COUNTS, counts.tolist())) == want["counts"]
    for name, t in out.items():
        same(name, t, want[name], per_file=True)


@pytest.mark.parametrize("mode", [S.EARLIER, S.ALL], ids=["earlier", "all"])
def test_peers_chunk_side(eng, mode):
    """T + 257 chunks, about one in 64 a hit and every chunk from T on: the
    counted holders are scanned over the chunks (the cscan), so the chunks from
    T on take their offsets through l3[1]"""
    m, n_files, k, max_holders = T + 257, 4099, 4, 64
    ix = S.gen_index(100001, S.dir_bits(100001), DEV, boundary=1 << 30)
    chunks = S.gen_chunks(ix, m, n_files, DEV, hit_one_in=64, hit_all_from=T, len_bits=40)
    ids = S.holder_ids(DEV)
    want = S.peers(ix, *chunks, k, max_holders, mode, 1 << 30, ids)
    pairs = want["counts"]["pairs"]
    assert (1 << 20) - (1 << 18) < pairs < (1 << 21) and want["counts"]["overflow"] == 0
    counted = want.pop("counted")
    uses_the_third_level(counted > 0, m)
    # the chunks from T on with pairs belong to at least two files that have a non-zero edge
    late = torch.unique(chunks[2][T:][counted[T:] > 0].to(torch.int64))
    assert int((want["edge_bytes"][late] > 0).any(1).sum()) >= 2
    check_peers(eng, ix, chunks, k, max_holders, mode, pairs + 257, want)


@pytest.mark.parametrize("mode", [S.EARLIER, S.ALL], ids=["earlier", "all"])
def test_peers_pair_side(eng, mode):
    """2^20 + 2^17 + 257 chunks with up to 17 counted holders each: more than
    T + 2^20 pair places, so the heads' ranks (the hscan's l3) and the byte sums
    before a place (the u64 scan's s3) carry a third level; lengths up to 2^40
    make the scanned sums pass 2^63"""
    m, n_files, k, max_holders = (1 << 20) + (1 << 17) + 257, 1021, 4, 17
    ix = S.gen_index(70001, S.dir_bits(70001), DEV, boundary=1 << 30, runs=(17, 17))
    chunks = S.gen_chunks(ix, m, n_files, DEV, len_bits=40)
    ids = S.holder_ids(DEV)
    max_pairs = eng.chunk_peers_plan(m, n_files, k, max_holders)[0]
    assert max_pairs == m * max_holders
    want = S.peers(ix, *chunks, k, max_holders, mode, max_pairs, ids)
    pairs = want["counts"]["pairs"]
    assert T + (1 << 20) < pairs <= max_pairs and want["counts"]["overflow"] == 0
    # the scan of the lengths over all places ends above 2^63: it needs all 64 bits
    assert sum(want["edge_bytes"].sum(1).tolist()) > 1 << 63 and int(chunks[3].max()) >> 39 == 1
    # the places are ordered by file: those from T on belong to at least two files with a non-zero edge
    ends = torch.cumsum(want["pairs_per_file"], 0)
    late = ends > T
    assert int(late.sum()) < n_files and int((late & (want["edge_bytes"] > 0).any(1)).sum()) >= 2
    assert want["counts"]["edges"] > n_files * 32
    want.pop("counted")
    check_peers(eng, ix, chunks, k, max_holders, mode, max_pairs, want)
