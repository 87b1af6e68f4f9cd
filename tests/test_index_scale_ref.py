"""The generator and the vectorised references of tests/_index_scale.py on the
CPU, at sizes the list references handle: exact equality, field by field and
count by count, with tests/_chunk_holders_ref.py, _chunk_index_ref.py and
_chunk_peers_ref.py, and the library's GPU-free check of a generated index.
What passes here is what tests/test_gpu_index_scale.py trusts at 2^24 entries
and beyond."""
import numpy as np
import pytest
import torch

from tests import _chunk_holders_ref as H
from tests import _chunk_index_ref as R
from tests import _chunk_peers_ref as P
from tests import _index_scale as S

SIZES = (0, 1, 255, 257, 5000)
BATCHES = (1, 257, 3000)
CPU = "cpu"


def u64(t):
    return t.numpy().view(np.uint64)


def entries(ix):
    """an Index or a Batch as the list references' tuples"""
    return R.from_arrays(u64(ix.keys), ix.digests.numpy(), u64(ix.values))


def widths(n):
    return sorted({0, 3, S.dir_bits(n)})


def same_index(ix, want, bits):
    assert entries(ix) == want
    assert ix.dir.numpy().view(np.uint32).tolist() == R.directory(want, bits) and ix.bits == bits


@pytest.mark.parametrize("n", SIZES + (7, 8, 9, 1 << 20, (1 << 20) + 1))
def test_dir_bits(n):
    from spacedrive_amd import Engine
    assert S.dir_bits(n) == R.dir_bits(n) == Engine.chunk_index_dir_bits(n)


@pytest.mark.parametrize("runs", [(1, 8), (1, 1), (17, 17)])
@pytest.mark.parametrize("n", SIZES)
def test_a_generated_index_is_a_holders_index(n, runs):
    from spacedrive_amd import Engine, _native as N
    for bits in widths(n):
        ix = S.gen_index(n, bits, CPU, runs=runs)
        assert ix.keys.shape == (n,) and ix.digests.shape == (n, 32) and ix.values.shape == (n,)
        assert ix.dir.shape == ((1 << bits) + 1,) and ix.dir.dtype == torch.int32
        assert n == 0 or (int(ix.keys.min()) >= 0 and int(ix.values.min()) >= 0)  # below 2^63
        es = entries(ix)
        assert H.check(es, ix.dir.numpy().view(np.uint32), bits) == (0, None)
        assert ix.dir.numpy().view(np.uint32).tolist() == R.directory(es, bits)
        assert Engine.chunk_holders_check(u64(ix.keys), ix.digests.numpy(), u64(ix.values),
                                          ix.dir.numpy().view(np.uint32), bits) == (N.SDCAS_OK, None)
        if runs == (1, 1):  # every pair once: a chunk index too
            assert Engine.chunk_index_check(u64(ix.keys), ix.digests.numpy(), ix.dir.numpy().view(np.uint32),
                                            bits) == (N.SDCAS_OK, None)


def test_the_generators_promises_at_a_scaled_down_boundary():
    n, boundary = 5000, 1000
    ix = S.gen_index(n, 5, CPU, boundary=boundary)
    es = entries(ix)
    for b in range(boundary, n, boundary):  # a run straddles every multiple of the boundary
        assert es[b - 1][:2] == es[b][:2] and es[b - 1][2] < es[b][2]
    runs = {}
    for k, d, _ in es:
        runs[(k, d)] = runs.get((k, d), 0) + 1
    assert set(runs.values()) >= set(range(1, 9))                       # the run lengths vary
    by_key = {}
    for k, d in runs:
        by_key.setdefault(k, []).append(d)
    double = [ds for ds in by_key.values() if len(ds) == 2]
    assert 0 < len(double) < len(by_key) / 8 and all(a < b for a, b in double)  # two digests, in memcmp order
    assert max(len(ds) for ds in by_key.values()) == 2
    # a digest uses all its 32 bytes, and the salt changes it
    dig = ix.digests.numpy()
    assert all(len(set(dig[:, j].tolist())) > 200 for j in range(32))
    other = S.gen_index(n, 5, CPU, boundary=boundary, salt=1)
    assert not set(d for _, d, _ in es) & set(d for _, d, _ in entries(other))
    # a value says which stretch of `boundary` entries its run begins in
    ids = set(S.holder_ids(CPU).tolist())
    first = 0
    for i, (k, d, v) in enumerate(es):
        if i and es[i - 1][:2] != (k, d):
            first = i
        assert v - S.ZONE_STEP * (first // boundary) in ids


def removed_sets(ix):
    ids = S.holder_ids(CPU)
    zones = torch.cat([ids[::z + 2] + z * S.ZONE_STEP for z in range(5)])
    return [torch.zeros(0, dtype=torch.int64), ids[:1], zones, torch.unique(ix.values), ids[-1:] + 1]


@pytest.mark.parametrize("n", SIZES)
def test_remove(n):
    ix = S.gen_index(n, S.dir_bits(n), CPU, boundary=1000)
    es = entries(ix)
    for removed in removed_sets(ix):
        for bits_new in widths(n):
            keep, new, counts = S.remove(ix, removed, bits_new)
            want, wcounts = H.remove(es, u64(removed))
            same_index(new, want, bits_new)
            assert counts == wcounts and int(keep.sum()) == len(want)
    if n == 5000:  # the zones' removed values keep another share of every stretch
        keep = S.remove(ix, removed_sets(ix)[2], 0)[0]
        shares = [int(keep[z * 1000:(z + 1) * 1000].sum()) for z in range(5)]
        assert shares == sorted(shares) and shares[0] > 300 and shares[-1] < 900 and len(set(shares)) == 5


@pytest.mark.parametrize("m", BATCHES)
@pytest.mark.parametrize("n_old", SIZES)
def test_add(n_old, m):
    old = S.gen_index(n_old, S.dir_bits(n_old), CPU, boundary=1000)
    batch = S.gen_batch(old, m, CPU)
    es = entries(old)
    want, wpos, wflags, wcounts = H.add(es, u64(batch.keys), batch.digests.numpy(), u64(batch.values))
    for bits_new in widths(n_old + m):
        new, pos, flags, counts, fresh = S.add(old, batch, bits_new)
        same_index(new, want, bits_new)
        assert (pos.numpy() == wpos).all() and (flags.numpy() == wflags).all() and counts == wcounts
    # fresh: the ADDED flags in the batch's own (triple, position) order
    bt = entries(batch)
    order = sorted(range(m), key=lambda c: (bt[c], c))
    assert fresh.tolist() == [bool(wflags[c] == H.ADDED) for c in order]
    # the batch is what gen_batch promises
    assert wcounts["hits"] == (m // 4 if n_old else 0) and wcounts["batch_duplicates"] == m // 4
    assert m < 4 or not S.distinct_pairs(old, batch)  # it holds copies


@pytest.mark.parametrize("m", BATCHES)
@pytest.mark.parametrize("n_old", SIZES)
def test_add_of_distinct_pairs_is_the_chunk_indexs_add(n_old, m):
    old = S.gen_index(n_old, S.dir_bits(n_old), CPU, runs=(1, 1))
    batch = S.gen_batch(old, m, CPU, distinct_pairs=True)
    assert S.distinct_pairs(old, batch)
    bits_new = S.dir_bits(n_old + m)
    new, pos, flags, counts, _ = S.add(old, batch, bits_new)
    for ref in (R, H):
        want, wpos, wflags, wcounts = ref.add(entries(old), u64(batch.keys), batch.digests.numpy(), u64(batch.values))
        same_index(new, want, bits_new)
        assert (pos.numpy() == wpos).all() and (flags.numpy() == wflags).all() and counts == wcounts
    assert counts["hits"] == min(m // 4, n_old) and counts["batch_duplicates"] == 0


def test_distinct_pairs_sees_what_breaks_it():
    old = S.gen_index(257, 3, CPU, runs=(1, 1))
    batch = S.gen_batch(old, 257, CPU, distinct_pairs=True)
    assert S.distinct_pairs(old, batch)
    twice = S.Batch(*(torch.cat([t, t[:1]]) for t in batch))
    assert not S.distinct_pairs(old, twice)                    # a pair twice in the batch
    hit = int(torch.nonzero(S.add(old, batch, 0)[2] == S.HIT)[0])
    values = batch.values.clone()
    values[hit] += 1
    assert not S.distinct_pairs(old, S.Batch(batch.keys, batch.digests, values))  # a hit with another value
    assert not S.distinct_pairs(S.gen_index(257, 3, CPU), batch)                  # old holds a pair twice


@pytest.mark.parametrize("m", BATCHES)
@pytest.mark.parametrize("n", SIZES)
def test_match(n, m):
    for runs, ref in (((1, 8), H), ((1, 1), R)):
        ix = S.gen_index(n, 3, CPU, boundary=1000, runs=runs)
        keys, dig = S.gen_queries(ix, m, CPU)
        pos, value, holders, counts = S.match(ix, keys, dig)
        want = ref.match(entries(ix), u64(keys), dig.numpy())
        assert (pos.numpy() == want[0]).all() and (u64(value) == want[1]).all() and counts == want[-1]
        if ref is H:
            assert (holders.numpy().view(np.uint32) == want[2]).all()
        else:
            assert (holders.numpy() == (want[0] >= 0)).all()
        if n:
            assert counts["misses"] == m // 4
            if m > 1:  # the first and the last run are asked for
                assert 0 in pos.tolist() and int(S.run_starts(ix.keys, ix.digests)[-1]) in pos.tolist()


PEERS = [  # n, runs, m, n_files, hit_one_in, max_holders, k, len_bits
    (5000, (1, 8), 3000, 37, 2, 5, 4, 40),
    (5000, (1, 8), 257, 300, 3, 64, 1, 16),
    (257, (17, 17), 3000, 8, 1, 17, 4, 40),
    (255, (17, 17), 257, 9, 1, 16, 64, 40),
    (1, (1, 8), 1, 1, 1, 1, 2, 8),
    (0, (1, 8), 257, 5, 1, 3, 3, 8),
]


@pytest.mark.parametrize("mode", [S.EARLIER, S.ALL])
@pytest.mark.parametrize("case", PEERS)
def test_peers(case, mode):
    n, runs, m, n_files, hit_one_in, max_holders, k, len_bits = case
    ix = S.gen_index(n, S.dir_bits(n), CPU, runs=runs, boundary=max(n, 1))
    ids = S.holder_ids(CPU)
    if n:
        keys, dig, chunk_file, chunk_len, file_ids = S.gen_chunks(ix, m, n_files, CPU, hit_one_in, m - 5, len_bits)
    else:
        one = S.gen_index(1, 0, CPU, salt=5)
        keys, dig, chunk_file, chunk_len, file_ids = S.gen_chunks(one, m, n_files, CPU, hit_one_in, None, len_bits)
    unbounded = P.peers(entries(ix), u64(keys), dig.numpy(), chunk_file.numpy(), u64(chunk_len), u64(file_ids), k,
                        max_holders, mode)
    pairs = unbounded["counts"]["pairs"]
    for max_pairs in sorted({pairs, pairs + 7, max(pairs - 1, 0), 0}):
        got = S.peers(ix, keys, dig, chunk_file, chunk_len, file_ids, k, max_holders, mode, max_pairs, ids)
        want = P.peers(entries(ix), u64(keys), dig.numpy(), chunk_file.numpy(), u64(chunk_len), u64(file_ids), k,
                       max_holders, mode, max_pairs=max_pairs)
        assert got["counts"] == want["counts"]
        assert (got["peer_count"].numpy().view(np.uint32) == want["peer_count"]).all()
        assert (u64(got["peers"]) == want["peers"]).all() and (u64(got["peer_bytes"]) == want["peers_bytes"]).all()
        for mine, theirs in (("shared", "shared_bytes"), ("unique", "unique_bytes"), ("common", "common_bytes")):
            assert (u64(got[mine]) == want[theirs]).all()
        assert int(got["pairs_per_file"].sum()) == pairs
    if n >= 255:  # the case has what it is there for
        c = unbounded["counts"]
        assert c["pairs"] >= c["edges"] >= c["files_with_peer"] > 0 and c["chunks"] == m
        if max_holders >= runs[1] and m > n_files:  # a file meets a holder in several chunks, and several holders
            assert c["pairs"] > c["edges"] > c["files_with_peer"]
        if max_holders < runs[1]:
            assert c["common_chunks"] > 0
        if mode == S.ALL and n_files >= 8:  # some file is its own holder somewhere
            earlier = P.peers(entries(ix), u64(keys), dig.numpy(), chunk_file.numpy(), u64(chunk_len), u64(file_ids),
                              k, 10 ** 6, S.EARLIER)
            every = P.peers(entries(ix), u64(keys), dig.numpy(), chunk_file.numpy(), u64(chunk_len), u64(file_ids),
                            k, 10 ** 6, S.ALL)
            assert earlier["counts"]["pairs"] < every["counts"]["pairs"]
