"""The chunk peers' reference (tests/_chunk_peers_ref.py) against cases worked by
hand: what the definition in include/sdcas.h says, before any kernel is asked."""
import numpy as np

from tests import _cdc_ref as C
from tests import _chunk_holders_ref as H
from tests import _chunk_index_ref as R
from tests import _chunk_peers_ref as P

U64_MAX = (1 << 64) - 1


def pool(n, seed=7):
    return R.random_pairs(np.random.default_rng(seed), n)


def index_of(keys, dig, holders):
    """holders[i]: the file ids that hold pair i"""
    return sorted((int(keys[i]), dig[i].tobytes(), int(v)) for i, hs in enumerate(holders) for v in hs)


def test_three_versions_of_a_log():
    """v1 = A, v2 = A B, v3 = A B C with ids 1 < 2 < 3 and A large: the peer of
    v3 is v2 with |A| + |B|, where the sharing reference says v1 with |A|"""
    keys, dig = pool(3)
    A, B, Cc = 50000, 3000, 700
    pick = np.array([0, 0, 1, 0, 1, 2])
    chunk_file = np.array([0, 1, 1, 2, 2, 2], np.uint32)
    chunk_len = np.array([A, A, B, A, B, Cc], np.uint64)
    ids = np.array([1, 2, 3], np.uint64)
    entries = H.build(keys[pick], dig[pick], ids[chunk_file])
    assert len(entries) == 6
    got = P.peers(entries, keys[pick], dig[pick], chunk_file, chunk_len, ids, 2, 64)
    assert got["peer_count"].tolist() == [0, 1, 2]
    assert got["peers"].tolist() == [[0, 0], [1, 0], [2, 1]]
    assert got["peers_bytes"].tolist() == [[0, 0], [A, 0], [A + B, A]]
    assert got["shared_bytes"].tolist() == [0, A, A + B] and got["unique_bytes"].tolist() == [A, B, Cc]
    assert got["counts"] == dict(files=3, chunks=6, common_chunks=0, pairs=1 + 2 + 1, edges=3, files_with_peer=2,
                                 overflow=0)
    # what the feature changes: the lowest-holder answer for the same chunks
    share = C.sharing(chunk_file, chunk_len, np.array([0, 0, 2, 0, 2, 5], np.int64), 3)
    assert share["peer"].tolist() == [-1, 0, 0] and int(share["peer_bytes"][2]) == A
    # ALL mode sees the later versions too: v1's nearest are v2 and v3, tied at |A|: the lower id first
    got = P.peers(entries, keys[pick], dig[pick], chunk_file, chunk_len, ids, 2, 64, P.ALL)
    assert got["peers"].tolist() == [[2, 3], [3, 1], [2, 1]]
    assert got["peers_bytes"].tolist() == [[A, A], [A + B, A], [A + B, A]]
    # after v1 is removed the nearest file of v3 is still v2
    left, _ = H.remove(entries, [1])
    got = P.peers(left, keys[pick], dig[pick], chunk_file, chunk_len, ids, 2, 64)
    assert got["peers"][2].tolist() == [2, 0] and got["peers_bytes"][2].tolist() == [A + B, 0]


def test_a_tie_goes_to_the_lowest_id_as_u64():
    keys, dig = pool(4)
    entries = index_of(keys, dig, [[9, 1 << 63], [5, 9], [5, 1 << 63], []])
    got = P.peers(entries, keys[:4], dig[:4], np.zeros(4, np.uint32), np.array([10, 10, 10, 1], np.uint64),
                  [U64_MAX], 3, 64)
    # 5, 9 and 2^63 all hold 20 bytes: ascending as unsigned
    assert got["peers"].tolist() == [[5, 9, 1 << 63]] and got["peers_bytes"].tolist() == [[20, 20, 20]]
    assert got["unique_bytes"].tolist() == [1] and got["counts"]["edges"] == 3


def test_earlier_ignores_later_holders_and_all_counts_them():
    keys, dig = pool(2)
    entries = index_of(keys, dig, [[3, 7, 11], [7, 20]])
    args = (entries, keys[:2], dig[:2], np.zeros(2, np.uint32), np.array([100, 40], np.uint64), [7], 4, 64)
    e = P.peers(*args, P.EARLIER)
    assert e["peers"].tolist() == [[3, 0, 0, 0]] and e["peers_bytes"].tolist() == [[100, 0, 0, 0]]
    assert e["shared_bytes"].tolist() == [100] and e["unique_bytes"].tolist() == [40] and e["counts"]["pairs"] == 1
    a = P.peers(*args, P.ALL)
    assert a["peers"].tolist() == [[3, 11, 20, 0]] and a["peers_bytes"].tolist() == [[100, 100, 40, 0]]
    assert a["peer_count"].tolist() == [3] and a["shared_bytes"].tolist() == [140] and a["counts"]["pairs"] == 3
    # a file that is not in the index at all: EARLIER takes what is below its id, ALL everything
    args = args[:5] + ([10],) + args[6:]
    assert P.peers(*args, P.EARLIER)["peers"].tolist() == [[7, 3, 0, 0]]  # 7 holds 140 bytes, 3 holds 100
    assert P.peers(*args, P.ALL)["peers"].tolist() == [[7, 3, 11, 20]]


def test_cnt_equal_to_h_scores_and_h_plus_1_is_common():
    keys, dig = pool(2)
    entries = index_of(keys, dig, [range(10, 15), range(10, 16)])  # 5 and 6 holders
    args = (entries, keys[[0, 1, 1]], dig[[0, 1, 1]], np.zeros(3, np.uint32), np.array([8, 5, 5], np.uint64), [99], 8)
    got = P.peers(*args, 5)
    assert got["shared_bytes"].tolist() == [8] and got["common_bytes"].tolist() == [10]
    assert got["peer_count"].tolist() == [5] and got["peers_bytes"][0, :5].tolist() == [8] * 5
    assert got["counts"]["common_chunks"] == 2 and got["counts"]["pairs"] == 5
    got = P.peers(*args, 6)  # a chunk that occurs twice counts twice
    assert got["common_bytes"].tolist() == [0] and got["shared_bytes"].tolist() == [18]
    assert got["peers"][0].tolist() == [10, 11, 12, 13, 14, 15, 0, 0]
    assert got["peers_bytes"][0].tolist() == [18] * 5 + [10, 0, 0]
    # in EARLIER mode only the holders below the file's id count towards H
    got = P.peers(*args[:5], [13], 8, 3)
    assert got["common_bytes"].tolist() == [0] and got["peers"][0, :3].tolist() == [10, 11, 12]


def test_shared_unique_and_common_add_up_modulo_2_64():
    rng = np.random.default_rng(11)
    keys, dig = pool(60, 12)
    entries = index_of(keys, dig, [rng.permutation(30)[:rng.integers(0, 12)] for _ in range(60)])
    pick = rng.integers(0, 60, 400)
    chunk_file = rng.integers(0, 9, 400).astype(np.uint32)  # file 8 is out of range
    chunk_len = rng.integers(1, 1 << 63, 400, dtype=np.uint64) * np.uint64(3)
    valid = (rng.random(400) > 0.2).astype(np.uint8)
    ids = np.array([4, 9, 14, 19, 24, 29, 0, U64_MAX], np.uint64)
    for mode in (P.EARLIER, P.ALL):
        got = P.peers(entries, keys[pick], dig[pick], chunk_file, chunk_len, ids, 4, 6, mode, valid)
        take = (valid != 0) & (chunk_file < 8)
        total = np.zeros(8, np.uint64)
        np.add.at(total, chunk_file[take], chunk_len[take])
        with np.errstate(over="ignore"):
            assert ((got["shared_bytes"] + got["unique_bytes"] + got["common_bytes"]) == total).all()
        assert got["counts"]["chunks"] == int(take.sum()) and got["counts"]["common_chunks"] > 0
        assert got["peers_bytes"].max() > (1 << 63) or mode == P.EARLIER  # sums that wrapped are among them
        # the rows are ordered and the unused slots are zero
        for f in range(8):
            c = int(got["peer_count"][f])
            row = list(zip((-got["peers_bytes"][f, :c].astype(object)).tolist(), got["peers"][f, :c].tolist()))
            assert row == sorted(row) and not got["peers"][f, c:].any() and not got["peers_bytes"][f, c:].any()
        assert got["peer_count"][6] == 0 or mode == P.ALL  # id 0 has nothing below it
        # overflow: given one pair less than there are
        over = P.peers(entries, keys[pick], dig[pick], chunk_file, chunk_len, ids, 4, 6, mode, valid,
                       got["counts"]["pairs"] - 1)
        assert over["counts"]["overflow"] == 1 and not over["peers"].any() and not over["peer_count"].any()
        assert (over["shared_bytes"] == got["shared_bytes"]).all() and over["counts"]["pairs"] == got["counts"]["pairs"]
        exact = P.peers(entries, keys[pick], dig[pick], chunk_file, chunk_len, ids, 4, 6, mode, valid,
                        got["counts"]["pairs"])
        assert P.same(exact, got)
