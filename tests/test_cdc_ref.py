"""The checker of the chunking tests (tests/_cdc_ref.py) against the values
pinned with the definition: table entries, window hashes, cut
lists, the chunk bound and the sharing pass on a hand-made case. No GPU."""
import numpy as np
import pytest

from tests import _cdc_ref as R
from tests._oracle import content, content_key

P = R.TEST_PARAMS


def test_gear_table_pinned():
    g = R.gear_table()
    assert g.dtype == np.uint32 and g.size == 256
    assert [int(g[i]) for i in (0, 1, 2, 3, 255)] == [0x835fea9c, 0xd1f33d4f, 0x7ccba815, 0xeef448a7, 0x4b42e713]


def test_window_hash_pinned_and_recurrence():
    x = content("pattern251", 0, 4096)
    h = R.window_hash(x)
    assert [int(h[p]) for p in (0, 1, 31, 32, 4095)] == [0x835fea9c, 0xd8b31287, 0x46b4ea47, 0x1462871a,
                                                        0x2e89ec30]
    # the running form h = (h << 1) + G[x[p]] from the start of the file
    g = R.gear_table()
    run = 0
    for p in range(200):
        run = ((run << 1) + int(g[x[p]])) & 0xFFFFFFFF
        assert run == int(h[p])
    # a position depends on the 32 bytes ending at it and on nothing older
    y = x.copy()
    y[:100] ^= 0x5A
    assert (R.window_hash(y)[131:] == h[131:]).all()
    assert R.window_hash(np.zeros(0, np.uint8)).size == 0


def test_window_with_hash_gives_the_hash_anywhere():
    rng = np.random.default_rng(32)
    targets = [0, 127, 128, 511, 512, 1 << 25, (1 << 27) - 1, (1 << 32) - 1]
    targets += [int(t) for t in rng.integers(0, 1 << 32, 200, dtype=np.uint64)]
    seen = set()
    for t in targets:
        w = R.window_with_hash(t, rng)
        assert w.dtype == np.uint8 and w.size == 32
        seen.add(w.tobytes())
        assert int(R.window_hash(w)[31]) == t  # at the start of a file
        for lead in (1, 31, 32, 77):  # and after any bytes
            x = np.concatenate([rng.integers(0, 256, lead, dtype=np.uint8), w, rng.integers(0, 256, 5, dtype=np.uint8)])
            assert int(R.window_hash(x)[lead + 31]) == t, (t, lead)
    assert len(seen) == len(targets)  # the free choices are drawn, not fixed
    # the last byte given: the same hash, or refused where its parity cannot give it
    g = R.gear_table()
    for b in (0, 138, 255):
        t = 0x12345678 ^ (int(g[b]) & 1)
        w = R.window_with_hash(t, rng, last=b)
        assert w[31] == b and int(R.window_hash(w)[31]) == t
        with pytest.raises(AssertionError):
            R.window_with_hash(t ^ 1, rng, last=b)


def test_cuts_pattern251_pinned():
    ends, kinds = R.cuts(content("pattern251", 0, 4096), P)
    assert ends.tolist() == [263, 560, 835, 1205, 1487, 1769, 2066, 2341, 2711, 2993, 3275, 3572, 3847, 4096]
    assert (kinds != R.KIND_MAX).all() and kinds[-1] == R.KIND_END and (kinds[:-1] == R.KIND_HASH).all()


def test_cuts_synth_pinned():
    x = content("synth", 0, 20000, content_key(0x5D, 1))
    ends, _ = R.cuts(x, P)
    assert ends.size == 67 and ends[:6].tolist() == [542, 799, 1059, 1209, 1594, 1958]
    ends, _ = R.cuts(x, (1024, 12, 16384))
    assert ends.tolist() == [1209, 5448, 7028, 10324, 12777, 14628, 20000]


def test_cuts_dense_and_empty_candidates():
    # every position a LOOSE candidate and none STRICT: a cut every avg bytes
    x = np.full(5000, 138, np.uint8)
    h = R.window_hash(x)
    assert (h[31:] == h[31]).all() and (int(h[31]) >> (32 - 7)) == 0 and (int(h[31]) >> (32 - 9)) != 0
    ends, kinds = R.cuts(x, P)
    assert ends.size == 20 and ends[:19].tolist() == list(range(256, 256 * 20, 256)) and ends[-1] == 5000
    assert (kinds[:-1] == R.KIND_HASH).all()
    # no candidate anywhere: cuts at max_len
    ends, kinds = R.cuts(np.zeros(100000, np.uint8), P)
    assert ends.size == 98 and int((kinds == R.KIND_MAX).sum()) == 97 and (np.diff(ends)[:96] == 1024).all()
    # 1025 zero bytes: one MAX cut, then a 1-byte end chunk
    ends, kinds = R.cuts(np.zeros(1025, np.uint8), P)
    assert ends.tolist() == [1024, 1025] and kinds.tolist() == [R.KIND_MAX, R.KIND_END]
    assert R.cuts(np.zeros(0, np.uint8), P)[0].size == 0


def test_cuts_small_lengths_and_bound():
    rng = np.random.default_rng(5)
    for L in (1, 31, 32, 33, 63, 64, 65, 1024):
        ends, kinds = R.cuts(rng.integers(0, 256, L, dtype=np.uint8), P)
        assert ends[-1] == L and kinds[-1] == R.KIND_END and ends.size <= -(-L // P[0])
    for L in rng.integers(1, 40000, 40):
        x = content("synth", 0, int(L), content_key(0xCDC, int(L)))
        for params in (P, (32, 6, 65), (1024, 12, 16384)):
            ends, _ = R.cuts(x, params)
            lens = np.diff(np.concatenate([[0], ends]))
            assert ends[-1] == L and (lens > 0).all() and ends.size <= -(-int(L) // params[0])
            assert (lens[:-1] >= params[0]).all() and (lens <= params[2]).all()


def test_equal_content_after_a_common_cut_gives_equal_chunks():
    a = content("synth", 0, 30000, content_key(0xCDC, 77))
    b = np.concatenate([a[:1000], np.array([7], np.uint8), a[1000:]])
    ea, _ = R.cuts(a, P)
    eb, _ = R.cuts(b, P)
    tail_a = {int(e) for e in ea if e > 2100}
    tail_b = {int(e) - 1 for e in eb if e > 2101}
    assert tail_a and tail_a == tail_b


def test_params_and_plan():
    assert R.params_valid(R.DEFAULT_PARAMS) and R.params_valid(P) and R.params_valid((32, 6, 65))
    for bad in ((31, 8, 1024), (64, 5, 1024), (64, 25, 1 << 26), (256, 8, 1024), (64, 8, 256), (64, 8, (1 << 28) + 1)):
        assert not R.params_valid(bad)
    assert R.chunk_plan([0, 1, 64, 65, 5000], P) == (0 + 1 + 1 + 2 + 79, (0 + 1 + 1 + 1 + 5) + 83)


def test_sharing_reference_with_a_tie():
    # file 0: chunks 0, 1 (new). file 1: chunk 2 new, chunk 3 = chunk 2 (self).
    # file 2: 100 bytes from file 0, 100 from file 1 (a tie: file 0 wins), 7 new.
    chunk_file = [0, 0, 1, 1, 2, 2, 2]
    chunk_len = [100, 50, 100, 100, 100, 100, 7]
    rep = [0, 1, 2, 2, 0, 2, 6]
    s = R.sharing(chunk_file, chunk_len, rep, 4)
    assert s["new_bytes"].tolist() == [150, 100, 7, 0]
    assert s["self_bytes"].tolist() == [0, 100, 0, 0]
    assert s["other_bytes"].tolist() == [0, 0, 200, 0]
    assert s["peer"].tolist() == [-1, -1, 0, -1] and s["peer_bytes"].tolist() == [0, 0, 100, 0]
    assert s["counts"] == {"files": 4, "chunks": 7, "distinct_chunks": 4, "total_bytes": 557, "stored_bytes": 257,
                           "files_with_peer": 1}
    # a stray rep counts as a first occurrence
    s = R.sharing([0, 1], [5, 6], [-1, 2], 2)
    assert s["new_bytes"].tolist() == [5, 6] and s["counts"]["distinct_chunks"] == 2
