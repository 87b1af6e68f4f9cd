"""The chunk peers on the GPU (sdcas_chunk_peers and sdcas_dev_chunk_peers,
csrc/chunk_peers.hip) against the Python reference of tests/_chunk_peers_ref.py:
through the host call and through the device call over guarded buffers (inputs
unchanged, guards intact, NULL outputs untouched, every output pre-poisoned).
Every comparison is exact equality. No test hands the device a malformed
index."""
import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests import _chunk_holders_ref as H
from tests import _chunk_index_ref as R
from tests import _chunk_peers_ref as P
from tests._guarded import Guarded, guarded_from

pytestmark = pytest.mark.gpu

FILL = 0xFE
U64_MAX = (1 << 64) - 1
OUTS = ("peer_count", "peers", "peers_bytes", "shared_bytes", "unique_bytes", "common_bytes")
MODES = (P.EARLIER, P.ALL)


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool():
    """400 distinct random pairs with real keys"""
    return R.random_pairs(np.random.default_rng(71), 400)


def ptr(g, used=True):
    return g.ptr if used and g.nbytes else 0


def index_of(keys, dig, holders):
    """holders[i]: the file ids that hold pair i"""
    return sorted((int(keys[i]), dig[i].tobytes(), int(v)) for i, hs in enumerate(holders) for v in hs)


def dev_peers(eng, entries, bits, keys, dig, chunk_file, chunk_len, ids, k, h, mode, valid=None, max_pairs=None,
              outputs=(True,) * 7):
    """sdcas_dev_chunk_peers over guarded buffers -> (the reference's dict, guards of the outputs)"""
    m, n, nf = len(keys), len(entries), len(ids)
    if max_pairs is None:
        max_pairs = min(m * h, 1 << 30)
    ik, idg, iv, idr, _ = H.arrays(entries, bits)
    ins = [guarded_from(ik, align=8), guarded_from(idg, align=16), guarded_from(iv, align=8), guarded_from(idr, align=4),
           guarded_from(np.asarray(keys, np.uint64), align=8), guarded_from(np.asarray(dig, np.uint8), align=16),
           guarded_from(np.asarray(chunk_file, np.uint32), align=4),
           guarded_from(np.asarray(chunk_len, np.uint64), align=8), guarded_from(np.asarray(ids, np.uint64), align=8)]
    gv = None if valid is None else guarded_from(np.asarray(valid, np.uint8), align=1)
    outs = [Guarded(4 * nf, align=4, fill=FILL), Guarded(8 * nf * k, align=8, fill=FILL),
            Guarded(8 * nf * k, align=8, fill=FILL), Guarded(8 * nf, align=8, fill=FILL),
            Guarded(8 * nf, align=8, fill=FILL), Guarded(8 * nf, align=8, fill=FILL), Guarded(56, align=8, fill=FILL)]
    torch.cuda.synchronize()
    eng.dev_chunk_peers(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3], n > 0), n, bits, ptr(ins[4]), ptr(ins[5]),
                        gv.ptr if gv is not None and m else 0, ptr(ins[6]), ptr(ins[7]), m, ptr(ins[8]), nf, k, h, mode,
                        max_pairs, *(ptr(o, outputs[j]) for j, o in enumerate(outs)))
    eng.dev_sync()
    torch.cuda.synchronize()
    every = ins + outs + ([gv] if gv is not None else [])
    for g in every:
        assert g.check() == []
    assert all(g.unchanged() for g in ins + ([gv] if gv is not None else []))
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {j} was written"
    got = {"peer_count": outs[0].download(np.uint32), "peers": outs[1].download(np.uint64).reshape(nf, k),
           "peers_bytes": outs[2].download(np.uint64).reshape(nf, k), "shared_bytes": outs[3].download(np.uint64),
           "unique_bytes": outs[4].download(np.uint64), "common_bytes": outs[5].download(np.uint64),
           "counts": dict(zip(P.COUNTS, (int(x) for x in outs[6].download(np.uint64))))}
    return got, outs


def both(eng, entries, bits, keys, dig, chunk_file, chunk_len, ids, k, h, mode=P.EARLIER, valid=None, max_pairs=None):
    """the reference against the host form and the device form -> the reference's dict"""
    keys, dig = np.asarray(keys, np.uint64), np.asarray(dig, np.uint8).reshape(-1, 32)
    chunk_file, chunk_len = np.asarray(chunk_file, np.uint32), np.asarray(chunk_len, np.uint64)
    ids = np.asarray(ids, np.uint64)
    want = P.peers(entries, keys, dig, chunk_file, chunk_len, ids, k, h, mode, valid, max_pairs)
    if want["counts"]["overflow"]:
        with pytest.raises(N.SdcasError) as ei:
            eng.chunk_peers(H.arrays(entries, bits), keys, dig, chunk_file, chunk_len, ids, k, h, mode, valid,
                            max_pairs)
        assert ei.value.code == N.SDCAS_E_CAPACITY
    else:
        got = eng.chunk_peers(H.arrays(entries, bits), keys, dig, chunk_file, chunk_len, ids, k, h, mode, valid,
                              max_pairs or 0)
        assert P.same(got, want), (got["counts"], want["counts"])
    got, _ = dev_peers(eng, entries, bits, keys, dig, chunk_file, chunk_len, ids, k, h, mode, valid, max_pairs)
    assert P.same(got, want), (got["counts"], want["counts"])
    with np.errstate(over="ignore"):
        total = np.zeros(len(ids), np.uint64)
        take = (chunk_file < len(ids)) & (np.ones(len(keys), bool) if valid is None else np.asarray(valid) != 0)
        np.add.at(total, chunk_file[take], chunk_len[take])
        assert ((want["shared_bytes"] + want["unique_bytes"] + want["common_bytes"]) == total).all()
    return want


def shared_corpus(pool, n_pairs, n_holders, seed):
    """pairs held by 0 to 11 of the ids 10, 20, ..., and a batch of chunks over them"""
    keys, dig = pool
    rng = np.random.default_rng(seed)
    holders = [10 * (1 + rng.permutation(n_holders)[:rng.integers(0, 12)]) for _ in range(n_pairs)]
    return index_of(keys, dig, holders)


def batch(pool, rng, m, n_pairs, n_files):
    keys, dig = pool
    pick = rng.integers(0, n_pairs, m)
    return keys[pick], dig[pick], np.sort(rng.integers(0, n_files, m)).astype(np.uint32), \
        rng.integers(1, 70000, m).astype(np.uint64)


def test_empty_things(eng, pool):
    keys, dig = pool
    entries = shared_corpus(pool, 80, 30, 1)
    rng = np.random.default_rng(2)
    k_, d_, fl, ln = batch(pool, rng, 50, 120, 4)
    ids = [55, 155, 255, 355]
    for mode in MODES:
        want = both(eng, [], 0, k_, d_, fl, ln, ids, 3, 8, mode)  # n = 0: everything is unique
        assert want["counts"]["pairs"] == 0 and int(want["unique_bytes"].sum()) == int(ln.sum())
        want = both(eng, entries, 3, k_[:0], d_[:0], fl[:0], ln[:0], ids, 3, 8, mode)  # m = 0
        assert want["counts"] == dict(files=4, chunks=0, common_chunks=0, pairs=0, edges=0, files_with_peer=0, overflow=0)
        want = both(eng, entries, 3, k_, d_, fl, ln, [], 3, 8, mode)  # n_files = 0: no chunk takes part
        assert want["counts"]["chunks"] == 0
        both(eng, [], 0, k_[:0], d_[:0], fl[:0], ln[:0], [], 1, 1, mode)  # nothing at all
        # file 1 has no chunk, file 3 only chunks nobody else holds
        fl2 = np.where(fl == 1, 2, fl).astype(np.uint32)
        k2, d2 = k_.copy(), d_.copy()
        k2[fl2 == 3], d2[fl2 == 3] = keys[300:300 + int((fl2 == 3).sum())], dig[300:300 + int((fl2 == 3).sum())]
        want = both(eng, entries, 3, k2, d2, fl2, ln, ids, 3, 8, mode)
        assert want["peer_count"][1] == want["peer_count"][3] == 0 and want["shared_bytes"][1] == 0
        assert want["unique_bytes"][3] == ln[fl2 == 3].sum() and want["peer_count"][0] > 0


@pytest.mark.parametrize("m", [255, 256, 257])
def test_around_a_workgroup(eng, pool, m):
    entries = shared_corpus(pool, 150, 40, m)
    k_, d_, fl, ln = batch(pool, np.random.default_rng(m), m, 200, 7)
    ids = [5, 105, 205, 305, 405, 1000, 0]
    for mode in MODES:
        for bits in (0, R.dir_bits(len(entries))):
            want = both(eng, entries, bits, k_, d_, fl, ln, ids, 4, 6, mode)
    assert want["counts"]["common_chunks"] > 0 and want["counts"]["edges"] > 20


def test_runs_of_1_2_3_and_1000_on_both_sides_of_the_common_rule(eng, pool):
    keys, dig = pool
    order = np.argsort(keys[:40], kind="stable")
    k40, d40 = keys[:40][order], dig[:40][order]
    holders = [list(range(100, 100 + 1 + i % 3)) for i in range(40)]
    holders[0], holders[-1] = [100, 101, 102], [100, 101]  # runs at the index's two ends
    holders[20] = list(range(50, 1050))
    entries = index_of(k40, d40, holders)
    assert len(entries) == sum(len(h) for h in holders) and entries[0][:2] == entries[2][:2]
    rng = np.random.default_rng(3)
    pick = np.concatenate([rng.permutation(40), [20, 20], 300 + np.arange(10)])
    kk = np.concatenate([k40, keys[40:]])[np.where(pick < 40, pick, pick - 260)]
    dd = np.concatenate([d40, dig[40:]])[np.where(pick < 40, pick, pick - 260)]
    fl = np.sort(rng.integers(0, 3, pick.size)).astype(np.uint32)
    ln = rng.integers(1, 9000, pick.size).astype(np.uint64)
    ids = [2000, 3000, 4000]
    for bits in (0, 3, R.dir_bits(len(entries)), 12):  # 12: a directory far wider than the index needs
        for mode in MODES:
            a = both(eng, entries, bits, kk, dd, fl, ln, ids, 8, 999, mode)
            b = both(eng, entries, bits, kk, dd, fl, ln, ids, 8, 1000, mode)
            assert a["counts"]["common_chunks"] == 3 and b["counts"]["common_chunks"] == 0
            assert b["counts"]["pairs"] == a["counts"]["pairs"] + 3000
            assert int(a["common_bytes"].sum()) == int(ln[pick == 20].sum()) and not b["common_bytes"].any()


def test_a_run_fills_its_bucket_and_extreme_keys(eng, pool):
    _, dig = pool
    entries = sorted([(0, dig[0].tobytes(), 0), (0, dig[0].tobytes(), U64_MAX), (0, dig[0].tobytes(), 1 << 63),
                      (0, dig[1].tobytes(), 5)] +
                     [(3 << 61, dig[2].tobytes(), v) for v in range(40)] +
                     [(U64_MAX, dig[3].tobytes(), U64_MAX), (U64_MAX, dig[3].tobytes(), 0),
                      (U64_MAX, dig[4].tobytes(), 9)])
    assert H.directory(entries, 3)[4] - H.directory(entries, 3)[3] == 40  # bucket 3 of 8 holds one run and nothing else
    q_keys = np.array([0, 0, 3 << 61, U64_MAX, U64_MAX, 0, U64_MAX, 3 << 61, 1], np.uint64)
    q_dig = np.stack([dig[0], dig[1], dig[2], dig[3], dig[4], dig[9], dig[9], dig[9], dig[0]])
    fl = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], np.uint32)
    ln = np.arange(1, 10, dtype=np.uint64) * np.uint64(1000)
    for ids in ([20, 1 << 63, U64_MAX], [0, 5, 40], [U64_MAX, 0, 1]):  # file ids 0 and 2^64 - 1 among them
        for bits in (0, 1, 3, 6):
            for mode in MODES:
                for h in (39, 40, 64):
                    want = both(eng, entries, bits, q_keys, q_dig, fl, ln, ids, 64, h, mode)
    # ids [2^64 - 1, 0, 1], ALL mode, H = 64: file 0 has 0 .. 39 and 2^63, file 1 has 2^64 - 1 and 9, file 2 misses
    assert want["peer_count"].tolist() == [41, 2, 0]


def test_self_at_the_first_a_middle_and_the_last_place_and_absent(eng, pool):
    keys, dig = pool
    run = [10, 20, 30, 40, 50]
    entries = index_of(keys, dig, [run, run, [7], run])
    fl = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4], np.uint32)
    pick = np.array([0, 1, 2, 0, 3, 1, 2, 0, 1, 3, 2])
    ln = (np.arange(11, dtype=np.uint64) + np.uint64(1)) * np.uint64(100)
    ids = [10, 30, 50, 35, U64_MAX]  # first, middle, last, absent inside the run, absent above it
    for mode in MODES:
        want = both(eng, entries, 2, keys[pick], dig[pick], fl, ln, ids, 5, 4, mode)
        if mode == P.EARLIER:
            assert want["peer_count"].tolist() == [1, 2, 5, 3, 1]  # file 4: its run of 5 is common, 7 is left
            assert want["peers"][0].tolist() == [7, 0, 0, 0, 0] and want["peers"][3].tolist() == [10, 20, 30, 0, 0]
        else:
            assert want["peer_count"].tolist() == [5, 4, 5, 0, 1]  # self taken out; absent: 5 > H is common
            assert want["peers"][0].tolist() == [7, 20, 30, 40, 50] and want["peers"][1].tolist() == [10, 20, 40, 50, 0]
    for ids in ([0, 0, 0, 0, 0], [U64_MAX] * 5, [0, U64_MAX, 20, 7, 40]):
        for mode in MODES:
            both(eng, entries, 0, keys[pick], dig[pick], fl, ln, ids, 3, 5, mode)


@pytest.mark.parametrize("k", [1, 2, 64])
def test_top_k_with_0_k_minus_1_k_and_k_plus_1_peers(eng, pool, k):
    keys, dig = pool
    # pair j is held by file id 100 + j alone: a file with chunks 0 .. p - 1 has p peers
    entries = index_of(keys, dig, [[100 + j] for j in range(k + 1)])
    want_peers = [0, k - 1, k, k + 1]
    pick = np.concatenate([np.arange(p) for p in want_peers] + [[200]]).astype(np.int64)
    fl = np.concatenate([np.full(p, i) for i, p in enumerate(want_peers)] + [[0]]).astype(np.uint32)
    ln = (1000 + 3 * np.arange(pick.size)).astype(np.uint64)  # later chunks are larger: the order is by bytes
    for mode in MODES:
        want = both(eng, entries, 2, keys[pick], dig[pick], fl, ln, [500, 501, 502, 503], k, 4, mode)
        assert want["peer_count"].tolist() == [min(k, p) for p in want_peers]
        for i, p in enumerate(want_peers):
            row = want["peers"][i]
            assert row[:min(k, p)].tolist() == [100 + j for j in range(p - 1, -1, -1)][:k] and not row[min(k, p):].any()
        assert want["counts"]["edges"] == sum(want_peers) and want["counts"]["files_with_peer"] == (3 if k > 1 else 2)


def test_ties_go_to_the_lowest_id(eng, pool):
    keys, dig = pool
    entries = index_of(keys, dig, [[9, 1 << 63, 300], [5, 9], [5, 1 << 63], [300, 7], [7]])
    ln = np.array([10, 10, 10, 4, 6, 1], np.uint64)
    want = both(eng, entries, 1, keys[[0, 1, 2, 3, 4, 50]], dig[[0, 1, 2, 3, 4, 50]], np.zeros(6, np.uint32), ln,
                [U64_MAX], 5, 64)
    # 5, 9 and 2^63 hold 20 bytes each, 7 holds 10, 300 holds 14
    assert want["peers"].tolist() == [[5, 9, 1 << 63, 300, 7]] and want["peers_bytes"].tolist() == [[20, 20, 20, 14, 10]]
    both(eng, entries, 1, keys[[0, 1, 2, 3, 4, 50]], dig[[0, 1, 2, 3, 4, 50]], np.zeros(6, np.uint32), ln, [9], 5, 64,
         P.ALL)


def test_sums_wrap_modulo_2_64(eng, pool):
    keys, dig = pool
    entries = index_of(keys, dig, [[1, 2], [1], [2, 3]])
    pick = np.array([0, 0, 1, 2, 0, 1, 60, 60])
    ln = np.array([U64_MAX, 5, 1 << 63, 1 << 63, (1 << 63) + 7, U64_MAX - 1, U64_MAX, 3], np.uint64)
    fl = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.uint32)
    for mode in MODES:
        want = both(eng, entries, 0, keys[pick], dig[pick], fl, ln, [10, 2], 3, 64, mode)
    assert want["peers_bytes"][0].tolist() == [(1 << 63) + 4, (1 << 63) + 4, 1 << 63]  # ids 1, 2, 3
    assert want["unique_bytes"][1] == 2


def test_one_long_run_of_equal_pairs_crosses_the_second_scan_level(eng, pool):
    """70 000 copies of one chunk held by 3 files: 210 000 pairs are 821
    workgroups, more than one workgroup scans, and three (file, holder) runs
    of 70 000 places each"""
    keys, dig = pool
    entries = index_of(keys, dig, [[4, 5, 6], [4], [9]])
    m = 70000
    k_, d_ = np.repeat(keys[:1], m), np.repeat(dig[:1], m, axis=0)
    k_[[0, m // 2, m - 1]], d_[[0, m // 2, m - 1]] = keys[[1, 2, 1]], dig[[1, 2, 1]]
    ln = (np.arange(m, dtype=np.uint64) % np.uint64(977)) + np.uint64(1)
    want = both(eng, entries, 0, k_, d_, np.zeros(m, np.uint32), ln, [100], 4, 3)
    assert want["counts"]["pairs"] == 3 * (m - 3) + 3 and want["counts"]["edges"] == 4
    assert want["peers"].tolist() == [[4, 5, 6, 9]]
    # the same chunks spread over 300 files, some of them holders themselves
    fl = np.sort(np.random.default_rng(5).integers(0, 300, m)).astype(np.uint32)
    for mode in MODES:
        want = both(eng, entries, 0, k_, d_, fl, ln, np.arange(300) + 5, 2, 3, mode)
    assert want["counts"]["edges"] > 800


def test_one_file_with_70_000_peers(eng, pool):
    """one chunk held by 70 000 files: 70 000 edges of one file, ordered by the
    second merge and ranked by one halving each"""
    keys, dig = pool
    entries = index_of(keys, dig, [range(1000, 71000), [5, 1001]])
    pick = np.array([0, 1, 1, 7])
    ln = np.array([500, 20, 30, 9], np.uint64)
    for k in (1, 64):
        want = both(eng, entries, R.dir_bits(len(entries)), keys[pick], dig[pick], np.zeros(4, np.uint32), ln,
                    [U64_MAX], k, 70000)
        assert want["counts"]["edges"] == 70001 and want["peers"][0, 0] == 1001 and want["peers_bytes"][0, 0] == 550
    assert want["peers"][0, 1:4].tolist() == [1000, 1002, 1003] and want["peers"][0, 63] == 1063
    want = both(eng, entries, 3, keys[pick], dig[pick], np.zeros(4, np.uint32), ln, [U64_MAX], 3, 69999)
    assert want["common_bytes"].tolist() == [500] and want["peers"].tolist() == [[5, 1001, 0]]


def test_capacity_exact_and_one_short(eng, pool):
    entries = shared_corpus(pool, 100, 25, 8)
    k_, d_, fl, ln = batch(pool, np.random.default_rng(9), 700, 130, 9)
    ids = 5 + 30 * np.arange(9)
    for mode in MODES:
        free = both(eng, entries, 4, k_, d_, fl, ln, ids, 3, 7, mode)
        pairs = free["counts"]["pairs"]
        assert pairs > 500
        exact = both(eng, entries, 4, k_, d_, fl, ln, ids, 3, 7, mode, max_pairs=pairs)
        assert P.same(exact, free)
        over = both(eng, entries, 4, k_, d_, fl, ln, ids, 3, 7, mode, max_pairs=pairs - 1)
        assert over["counts"] == dict(free["counts"], edges=0, files_with_peer=0, overflow=1)
        assert not over["peers"].any() and not over["peers_bytes"].any() and not over["peer_count"].any()
        for key in ("shared_bytes", "unique_bytes", "common_bytes"):
            assert (over[key] == free[key]).all()
        # the device form without any room, as ChunkHolders.peers' counting call passes it
        got, _ = dev_peers(eng, entries, 4, k_, d_, fl, ln, ids, 3, 7, mode, max_pairs=0, outputs=(False,) * 6 + (True,))
        assert got["counts"] == over["counts"]


def test_one_forged_key_a_valid_mask_and_files_out_of_range(eng):
    base = np.random.default_rng(10).integers(0, 256, 32, dtype=np.uint8)
    dig = np.tile(base, (600, 1))
    v = np.arange(600)
    dig[:, 31], dig[:, 30] = v & 0xFF, v >> 8
    keys = np.full(600, 0x1234567890ABCDEF, np.uint64)
    even = np.arange(600) % 2 == 0
    entries = index_of(keys[even], dig[even], [[10 * (1 + (i + j) % 9) for j in range(1 + i % 4)] for i in range(300)])
    rng = np.random.default_rng(11)
    pick = rng.permutation(600)
    fl = rng.integers(0, 8, 600).astype(np.uint32)  # files 6 and 7 are out of range
    ln = rng.integers(1, 5000, 600).astype(np.uint64)
    valid = (rng.random(600) > 0.3).astype(np.uint8)
    valid[:3] = 0
    ids = [15, 35, 55, 95, 20, 0]
    for mode in MODES:
        for bits in (0, 5):
            want = both(eng, entries, bits, keys[pick], dig[pick], fl, ln, ids, 4, 3, mode, valid)
            assert want["counts"]["chunks"] == int(((valid != 0) & (fl < 6)).sum())
        both(eng, entries, 5, keys[pick], dig[pick], fl, ln, ids, 4, 3, mode, np.zeros(600, np.uint8))  # none valid
        both(eng, entries, 5, keys[pick], dig[pick], np.full(600, 0xFFFFFFFF, np.uint32), ln, ids, 4, 3, mode)


def test_two_calls_write_the_same_bytes_and_null_outputs(eng, pool):
    entries = shared_corpus(pool, 200, 50, 12)
    k_, d_, fl, ln = batch(pool, np.random.default_rng(13), 3000, 260, 40)
    ids = 7 + 11 * np.arange(40)
    args = (eng, entries, R.dir_bits(len(entries)), k_, d_, fl, ln, ids, 4, 5, P.ALL)
    a, ga = dev_peers(*args)
    b, gb = dev_peers(*args)
    assert all((x.download() == y.download()).all() for x, y in zip(ga, gb)) and a["counts"]["edges"] > 100
    for j in range(7):  # every single NULL output is accepted, and then all of them
        got, _ = dev_peers(*args, outputs=tuple(i != j for i in range(7)))
        for i, key in enumerate(OUTS):
            assert i == j or np.array_equal(got[key], a[key]), (j, key)
        assert j == 6 or got["counts"] == a["counts"]
    dev_peers(*args, outputs=(False,) * 7)


def test_errors_leave_the_stream_empty_and_the_outputs_poisoned(eng, pool):
    keys, dig = pool
    entries = shared_corpus(pool, 30, 10, 14)
    n = len(entries)
    ik, idg, iv, idr, _ = H.arrays(entries, 2)
    ix = [guarded_from(ik, align=8), guarded_from(idg, align=16), guarded_from(iv, align=8), guarded_from(idr, align=4)]
    bt = [guarded_from(keys[:8], align=8), guarded_from(dig[:8], align=16),
          guarded_from(np.zeros(8, np.uint32), align=4), guarded_from(np.full(8, 9, np.uint64), align=8),
          guarded_from(np.array([500, 600], np.uint64), align=8)]
    outs = [Guarded(8, align=4, fill=FILL), Guarded(64, align=8, fill=FILL), Guarded(64, align=8, fill=FILL),
            Guarded(16, align=8, fill=FILL), Guarded(16, align=8, fill=FILL), Guarded(16, align=8, fill=FILL),
            Guarded(56, align=8, fill=FILL)]
    torch.cuda.synchronize()

    def call(idx_dig=ix[1].ptr, q_dig=bt[1].ptr, files=bt[2].ptr, lens=bt[3].ptr, ids=bt[4].ptr, n=n, bits=2, m=8, k=4,
             h=8, mode=0, max_pairs=64, count=outs[0].ptr, peers=outs[1].ptr, keys_=bt[0].ptr):
        with pytest.raises(N.SdcasError) as ei:
            eng.dev_chunk_peers(ix[0].ptr, idx_dig, ix[2].ptr, ix[3].ptr, n, bits, keys_, q_dig, 0, files, lens, m, ids,
                                2, k, h, mode, max_pairs, count, peers, *(o.ptr for o in outs[2:]))
        return ei.value.code

    for bad in (dict(idx_dig=ix[1].ptr + 8), dict(q_dig=bt[1].ptr + 4), dict(files=bt[2].ptr + 2),
                dict(lens=bt[3].ptr + 4), dict(ids=bt[4].ptr + 4), dict(count=outs[0].ptr + 2),
                dict(peers=outs[1].ptr + 4), dict(k=0), dict(k=65), dict(h=0), dict(h=(1 << 20) + 1), dict(mode=2),
                dict(files=0), dict(lens=0), dict(ids=0), dict(keys_=0)):
        assert call(**bad) == N.SDCAS_E_INVALID, bad
    for bad in (dict(n=(1 << 30) + 1), dict(m=(1 << 30) + 1), dict(bits=29), dict(max_pairs=(1 << 30) + 1)):
        assert call(**bad) == N.SDCAS_E_CAPACITY, bad
    eng.dev_sync()
    torch.cuda.synchronize()
    assert all(o.untouched() and o.check() == [] for o in outs)
    assert all(g.unchanged() for g in ix + bt)
    # the host form's refusals, with the context's message
    with pytest.raises(N.SdcasError) as ei:
        eng.chunk_peers((ik, idg, iv, idr, 2), keys[:8], dig[:8], np.zeros(8, np.uint32), np.ones(8, np.uint64),
                        [500, 600], 4, 8, 7)
    assert ei.value.code == N.SDCAS_E_INVALID and "mode" in str(ei.value)


def test_the_resident_index_answers_as_the_host_form(eng, pool):
    """ChunkHolders.peers on the index's stream, with its counting call first"""
    from spacedrive_amd import ChunkHolders
    keys, dig = pool
    entries = shared_corpus(pool, 150, 30, 15)
    ek, ed, ev = H.batch_arrays(entries)
    ix = ChunkHolders(eng)
    ix.add(ek, ed, ev)
    k_, d_, fl, ln = batch(pool, np.random.default_rng(16), 900, 200, 12)
    ids = 5 + 25 * np.arange(12)
    before = [a.tobytes() if hasattr(a, "tobytes") else a for a in ix.arrays()]
    for mode, name in zip(MODES, ("earlier", "all")):
        want = P.peers(entries, k_, d_, fl, ln, ids, 4, 6, mode)
        assert P.same(ix.peers(k_, d_, fl, ln, ids, 4, 6, name), want)
        assert P.same(ix.peers(k_, d_, fl, ln, ids, 4, 6, mode, max_pairs=900 * 6), want)
        with pytest.raises(N.SdcasError) as ei:
            ix.peers(k_, d_, fl, ln, ids, 4, 6, mode, max_pairs=want["counts"]["pairs"] - 1)
        assert ei.value.code == N.SDCAS_E_CAPACITY
    assert [a.tobytes() if hasattr(a, "tobytes") else a for a in ix.arrays()] == before  # the index is not changed
