"""The reference of the file families (tests/_families_ref.py) pinned with the
definition (include/sdcas.h): against a brute-force
breadth-first search on small random graphs, and on the edges of the slot
classes. No GPU."""
import numpy as np

from tests import _families_ref as F

M64 = (1 << 64) - 1


def bfs(ids, sizes, peer_count, peers, peer_bytes, num, den):
    """the components by breadth-first search over an adjacency list -> (family, family_size, links)"""
    n, k = len(ids), peers.shape[1]
    adj, links = [set() for _ in range(n)], 0
    for i in range(n):
        for s in range(min(int(peer_count[i]), k)):
            f, b = int(peers[i, s]), int(peer_bytes[i, s])
            rows = [j for j in range(n) if int(ids[j]) == f]
            if not rows or rows[0] == i:
                continue
            j = rows[0]
            if b > 0 and b * den >= num * max(int(sizes[i]), int(sizes[j])):
                adj[i].add(j), adj[j].add(i)
                links += 1
    family = [-1] * n
    for r in range(n):
        if family[r] >= 0:
            continue
        family[r], todo = r, [r]
        while todo:
            nxt = []
            for x in todo:
                for y in adj[x]:
                    if family[y] < 0:
                        family[y] = r
                        nxt.append(y)
            todo = nxt
    size = [family.count(f) for f in family]
    return np.array(family, np.int64), np.array(size, np.uint32), links


def random_graph(rng, n, k):
    ids = np.cumsum(rng.integers(1, 5, n)).astype(np.uint64)
    sizes = rng.integers(1, 2000, n).astype(np.uint64)
    peer_count = rng.integers(0, k + 3, n).astype(np.uint32)  # above k too: clamped
    pick = rng.integers(0, max(n, 1), (n, k))
    peers = np.where(rng.random((n, k)) < 0.8, ids[pick] if n else 0, rng.integers(0, 5 * n + 9, (n, k))).astype(np.uint64)
    peer_bytes = rng.integers(0, 2000, (n, k)).astype(np.uint64)
    return ids, sizes, peer_count, peers, peer_bytes


def test_reference_against_breadth_first_search():
    rng = np.random.default_rng(310)
    seen = set()
    for trial in range(120):
        n, k = int(rng.integers(0, 61)), int(rng.integers(1, 6))
        num, den = [(1, 2), (0, 1), (1, 1), (1, 8), (3, 4)][trial % 5]
        g = random_graph(rng, n, k)
        got = F.families(*g, num, den)
        family, size, links = bfs(*g, num, den)
        assert np.array_equal(got["family"], family) and np.array_equal(got["family_size"], size), trial
        c = got["counts"]
        assert c["links"] == links and c["files"] == n and c["unsorted"] == 0
        assert c["slots"] == int(np.minimum(g[2], k).sum()) == c["missing"] + c["self_slots"] + c["weak"] + c["links"]
        fams = {int(f) for f, s in zip(family, size) if s >= 2}
        assert c["families"] == len(fams) and c["members"] == int((size >= 2).sum())
        assert c["largest"] == (int(size.max()) if fams else 0)
        # the sets are the families of two or more, by lowest member, members ascending
        set_rep, set_offsets, members = F.sets_of(got["family"])
        assert set_rep.tolist() == sorted(fams) and int(set_offsets[-1]) == members.size == c["members"]
        for s, r in enumerate(set_rep):
            assert members[int(set_offsets[s]):int(set_offsets[s + 1])].tolist() == np.flatnonzero(family == r).tolist()
        seen.add((c["families"] > 1, c["missing"] > 0, c["self_slots"] > 0, c["weak"] > 0))
    assert (True, True, True, True) in seen


def one_slot(size_i, size_j, b, num, den):
    """rows 0 and 1, row 1 lists row 0 with b bytes -> the reference's dict"""
    return F.families([5, 9], [size_i, size_j], [0, 1], [[0], [5]], [[0], [b]], num, den)


def test_threshold_edges():
    # b * den == num * max passes, one byte less is weak
    for size_i, size_j, num, den, b in ((1000, 600, 1, 2, 500), (600, 1000, 1, 2, 500), (999, 7, 1, 3, 333),
                                        (1 << 40, 1 << 39, 3, 4, 3 << 38), (10, 10, 1, 1, 10)):
        assert b * den == num * max(size_i, size_j)
        hit, miss = one_slot(size_i, size_j, b, num, den), one_slot(size_i, size_j, b - 1, num, den)
        assert hit["family"].tolist() == [0, 0] and hit["counts"]["links"] == 1 and hit["counts"]["weak"] == 0
        assert miss["family"].tolist() == [0, 1] and miss["counts"]["links"] == 0 and miss["counts"]["weak"] == 1
        assert hit["family_size"].tolist() == [2, 2] and miss["family_size"].tolist() == [1, 1]
    # the size is the larger of the two, not the own and not the smaller
    assert one_slot(100, 2000, 100, 1, 2)["counts"]["weak"] == 1
    assert one_slot(2000, 100, 100, 1, 2)["counts"]["weak"] == 1
    # num = 0 links every slot with b > 0, and b = 0 never links
    assert one_slot(M64, M64, 1, 0, 1)["counts"]["links"] == 1
    assert one_slot(1, 1, 0, 0, 1)["counts"] == dict(files=2, slots=1, missing=0, self_slots=0, weak=1, links=0,
                                                     families=0, members=0, largest=0, unsorted=0)
    assert one_slot(0, 0, 0, 1, 2)["counts"]["weak"] == 1  # 0 >= 0, but b = 0
    # num = den: all of the larger file
    assert one_slot(700, 700, 700, 5, 5)["counts"]["links"] == 1
    assert one_slot(700, 701, 700, 5, 5)["counts"]["weak"] == 1


def wrapped(b, size_i, size_j, num, den):
    """the comparison as 64-bit arithmetic that wraps would make it"""
    return b > 0 and (b * den) & M64 >= (num * max(size_i, size_j)) & M64


def test_products_beyond_64_bits_are_compared_exactly():
    cases = (((1 << 63) + 20, 7, (1 << 63) + 5, 1, 2, True),    # 2 b = 2^64 + 10 wraps to 10
             ((1 << 63) + 1, 3, (1 << 63) - 1, 2, 2, False),    # 2 max = 2^64 + 2 wraps to 2
             (M64, M64, M64, 0xFFFFFFFF, 0xFFFFFFFF, True),      # both products near 2^96
             (M64, M64, M64 - 1, 0xFFFFFFFF, 0xFFFFFFFF, False),
             (M64, 1, (M64 // 3) + 1, 1, 3, True), (M64, 1, M64 // 3 - 1, 1, 3, False))
    flips = 0
    for size_i, size_j, b, num, den, link in cases:
        assert F.passes(b, size_i, size_j, num, den) == link
        got = one_slot(size_i, size_j, b, num, den)
        assert got["counts"]["links"] == int(link) and got["counts"]["weak"] == int(not link)
        flips += wrapped(b, size_i, size_j, num, den) != link
    (s0, t0, b0, n0, d0, _), (s1, t1, b1, n1, d1, _) = cases[:2]
    assert wrapped(b0, s0, t0, n0, d0) is False and wrapped(b1, s1, t1, n1, d1) is True and flips >= 2


def test_classes_of_a_slot_and_the_count_clamp():
    ids, sizes = [10, 20, 30, 40], [100, 100, 100, 100]
    peers = [[20, 10, 15], [5, 20, 99], [10, 40, 20], [30, 30, 30]]
    pbytes = [[90, 90, 90], [90, 90, 90], [10, 0, 50], [60, 60, 60]]
    got = F.families(ids, sizes, [3, 3, 3, 7], peers, pbytes)
    # row 0: link to 20, self, missing (between two ids); row 1: below the first id, self, above the last;
    # row 2: weak, b = 0, link; row 3: its count of 7 clamped to 3, three links to row 2
    assert got["counts"] == dict(files=4, slots=12, missing=3, self_slots=2, weak=2, links=5, families=1, members=4,
                                 largest=4, unsorted=0)
    assert got["family"].tolist() == [0, 0, 0, 0] and got["family_size"].tolist() == [4, 4, 4, 4]
    # a slot past the count that holds a real id is ignored
    got = F.families(ids, sizes, [0, 0, 0, 1], peers, pbytes)
    assert got["family"].tolist() == [0, 1, 2, 2] and got["counts"]["slots"] == 1


def test_unsorted_ids_give_the_trivial_rows():
    for ids in ([1, 1, 2], [1, 2, 2], [1, 3, 2], [2, 1]):
        got = F.families(ids, [9] * len(ids), [1] * len(ids), [[ids[0]]] * len(ids), [[9]] * len(ids))
        n = len(ids)
        assert got["family"].tolist() == list(range(n)) and got["family_size"].tolist() == [1] * n
        assert got["counts"] == dict(dict.fromkeys(F.COUNTS, 0), files=n, unsorted=1)
    assert F.families([], [], [], np.zeros((0, 4)), np.zeros((0, 4)))["counts"] == dict.fromkeys(F.COUNTS, 0)
