"""The file families on the GPU (sdcas_file_families and sdcas_dev_file_families,
csrc/families.hip) against the Python reference of tests/_families_ref.py:
through the host call and through the device call over guarded buffers (inputs
unchanged, guards intact, NULL outputs untouched, every output pre-poisoned).
Every comparison is exact equality. No test hands the device anything meant to
fault it: every input is well formed, or is rejected before launch."""
import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests import _families_ref as F
from tests._guarded import Guarded, guarded_from

pytestmark = pytest.mark.gpu

FILL = 0xFE
M64 = (1 << 64) - 1
SIZE, STRONG, FAINT = 1000, 600, 100  # under 1/2: 600 of 1000 links, 100 does not


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def ptr(g, used=True):
    return g.ptr if used and g.nbytes else 0


def arrays(ids, sizes, peer_count, peers, peer_bytes):
    ids, sizes = np.asarray(ids, np.uint64), np.asarray(sizes, np.uint64)
    n = ids.size
    peers, peer_bytes = np.asarray(peers, np.uint64), np.asarray(peer_bytes, np.uint64)
    k = peers.shape[1] if peers.ndim == 2 else peers.size // max(n, 1)
    return ids, sizes, np.asarray(peer_count, np.uint32), peers.reshape(n, k), peer_bytes.reshape(n, k)


def dev_families(eng, g, num=1, den=2, outputs=(True, True, True)):
    """sdcas_dev_file_families over guarded buffers -> (the reference's dict, the outputs' guards)"""
    ids, sizes, pc, peers, pb = g
    n, k = peers.shape
    ins = [guarded_from(ids, align=8), guarded_from(sizes, align=8), guarded_from(pc, align=4),
           guarded_from(peers, align=8), guarded_from(pb, align=8)]
    outs = [Guarded(8 * n, align=8, fill=FILL), Guarded(4 * n, align=4, fill=FILL), Guarded(80, align=8, fill=FILL)]
    torch.cuda.synchronize()
    eng.dev_file_families(*(ptr(x) for x in ins), n, k, num, den, *(ptr(o, outputs[j]) for j, o in enumerate(outs)))
    eng.dev_sync()
    torch.cuda.synchronize()
    for x in ins + outs:
        assert x.check() == []
    assert all(x.unchanged() for x in ins)
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {j} was written"
    got = {"family": outs[0].download(np.int64), "family_size": outs[1].download(np.uint32),
           "counts": dict(zip(F.COUNTS, (int(x) for x in outs[2].download(np.uint64))))}
    return got, outs


def both(eng, g, num=1, den=2, want=None):
    """the reference against the host form and the device form, the device form twice -> the reference's dict"""
    g = arrays(*g)
    want = F.families(*g, num, den) if want is None else want
    if want["counts"]["unsorted"]:
        with pytest.raises(N.SdcasError) as ei:
            eng.file_families(*g, num, den)
        assert ei.value.code == N.SDCAS_E_INVALID and "ascending" in str(ei.value)
    else:
        got = eng.file_families(*g, num, den)
        assert F.same(got, want), (got["counts"], want["counts"])
    a, ga = dev_families(eng, g, num, den)
    assert F.same(a, want), (a["counts"], want["counts"])
    _, gb = dev_families(eng, g, num, den)
    assert all((x.download() == y.download()).all() for x, y in zip(ga, gb))  # two calls give the same bytes
    return want


def dev_sets(eng, family):
    """sdcas_dev_duplicate_sets over a device label array, no host round trip of the labels"""
    n = family.numel()
    set_rep = torch.full((n // 2,), -1, dtype=torch.int64, device="cuda")
    set_off = torch.full((n // 2 + 1,), -1, dtype=torch.int64, device="cuda")
    members = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    cts = torch.zeros(6, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr() if t.numel() else 0  # noqa: E731
    eng.dev_duplicate_sets(p(family), 0, n, p(set_rep), p(set_off), 0, p(members), cts.data_ptr())
    eng.dev_sync()
    sets, mem = int(cts[1]), int(cts[2])
    return set_rep[:sets].cpu().numpy(), set_off[:sets + 1].cpu().numpy().view(np.uint64), members[:mem].cpu().numpy()


# ---- the small cases --------------------------------------------------------------------------

def test_no_row_one_row_and_two_rows(eng):
    want = both(eng, ([], [], [], np.zeros((0, 3)), np.zeros((0, 3))))
    assert want["counts"] == dict.fromkeys(F.COUNTS, 0)
    want = both(eng, ([7], [SIZE], [2], [[7, 9]], [[STRONG, STRONG]]))  # itself, and a missing id
    assert want["family"].tolist() == [0] and want["counts"]["self_slots"] == 1 and want["counts"]["missing"] == 1
    up = both(eng, ([7, 9], [SIZE, SIZE], [0, 1], [[0], [7]], [[0], [STRONG]]))    # row 1 lists row 0
    down = both(eng, ([7, 9], [SIZE, SIZE], [1, 0], [[9], [0]], [[STRONG], [0]]))  # row 0 lists row 1
    for want in (up, down):
        assert want["family"].tolist() == [0, 0] and want["family_size"].tolist() == [2, 2]
        assert want["counts"] == dict(files=2, slots=1, missing=0, self_slots=0, weak=0, links=1, families=1, members=2,
                                      largest=2, unsorted=0)
    each = both(eng, ([7, 9], [SIZE, SIZE], [1, 1], [[9], [7]], [[STRONG], [STRONG]]))
    assert each["counts"]["links"] == 2 and each["counts"]["families"] == 1  # a pair that lists each other counts twice


def test_threshold_edges_and_products_beyond_64_bits(eng):
    def one_slot(size_i, size_j, b, num, den):
        return both(eng, ([5, 9], [size_i, size_j], [0, 1], [[0], [5]], [[0], [b]]), num, den)

    for size_i, size_j, num, den, b in ((1000, 600, 1, 2, 500), (600, 1000, 1, 2, 500), (999, 7, 1, 3, 333),
                                        (1 << 40, 1 << 39, 3, 4, 3 << 38), (10, 10, 1, 1, 10)):
        assert one_slot(size_i, size_j, b, num, den)["counts"]["links"] == 1
        assert one_slot(size_i, size_j, b - 1, num, den)["counts"]["weak"] == 1
    assert one_slot(100, 2000, 100, 1, 2)["counts"]["weak"] == 1  # the larger size counts, either way round
    assert one_slot(2000, 100, 100, 1, 2)["counts"]["weak"] == 1
    assert one_slot(M64, M64, 1, 0, 1)["counts"]["links"] == 1  # num = 0
    assert one_slot(1, 1, 0, 0, 1)["counts"]["weak"] == 1       # b = 0
    assert one_slot(0, 0, 0, 1, 2)["counts"]["weak"] == 1
    assert one_slot(700, 700, 700, 5, 5)["counts"]["links"] == 1  # num = den
    assert one_slot(700, 701, 700, 5, 5)["counts"]["weak"] == 1
    # where arithmetic that wraps at 2^64 gives the opposite answer
    for size_i, size_j, b, num, den, link in (((1 << 63) + 20, 7, (1 << 63) + 5, 1, 2, True),
                                              ((1 << 63) + 1, 3, (1 << 63) - 1, 2, 2, False),
                                              (M64, M64, M64, 0xFFFFFFFF, 0xFFFFFFFF, True),
                                              (M64, M64, M64 - 1, 0xFFFFFFFF, 0xFFFFFFFF, False),
                                              (M64, 1, M64 // 3 + 1, 1, 3, True), (M64, 1, M64 // 3 - 1, 1, 3, False)):
        want = one_slot(size_i, size_j, b, num, den)
        assert want["counts"]["links"] == int(link) and want["counts"]["weak"] == int(not link)


def test_slot_classes_the_count_clamp_and_ids_at_the_ends(eng):
    ids, sizes = [10, 20, 30, 40], [100, 100, 100, 100]
    peers = [[20, 10, 15], [5, 20, 99], [10, 40, 20], [30, 30, 30]]
    pbytes = [[90, 90, 90], [90, 90, 90], [10, 0, 50], [60, 60, 60]]
    want = both(eng, (ids, sizes, [3, 3, 3, 7], peers, pbytes))  # 7 > k is clamped to 3
    assert want["counts"] == dict(files=4, slots=12, missing=3, self_slots=2, weak=2, links=5, families=1, members=4,
                                  largest=4, unsorted=0)
    # slots past the count hold real ids and strong bytes: they are not read
    want = both(eng, (ids, sizes, [0, 0, 0, 1], peers, pbytes))
    assert want["family"].tolist() == [0, 1, 2, 2] and want["counts"]["slots"] == 1
    want = both(eng, (ids, sizes, [0xFFFFFFFF] * 4, peers, pbytes))
    assert want["counts"]["slots"] == 12
    # ids with gaps, 0 and 2^64 - 1 among them; peers below the first, between two, above the last
    ids = [0, 3, 1 << 32, (1 << 63) - 1, 1 << 63, M64 - 1, M64]
    sizes = [SIZE] * 7
    peers = [[M64, 1], [0, 2], [(1 << 32) + 1, 3], [1 << 63, (1 << 63) + 1], [M64 - 2, M64 - 1], [M64, 1 << 32], [0, M64]]
    want = both(eng, (ids, sizes, [2] * 7, peers, np.full((7, 2), STRONG)))
    assert want["counts"]["missing"] == 5 and want["counts"]["self_slots"] == 1 and want["counts"]["links"] == 8
    assert want["family"].tolist() == [0] * 7
    want = both(eng, ([5, 6], [SIZE] * 2, [2, 2], [[4, 7], [0, M64]], np.full((2, 2), STRONG)))
    assert want["counts"]["missing"] == 4 and want["family"].tolist() == [0, 1]


def test_unsorted_ids_give_the_trivial_rows_and_the_host_form_refuses(eng):
    n = 600  # more than one workgroup: the flag is read by every one of them
    base = 10 * np.arange(n, dtype=np.uint64) + 7
    peers = np.roll(base, 1).reshape(n, 1)
    for at, value in ((n - 1, base[n - 2] - 1), (n - 1, base[n - 2]), (1, base[0]), (300, base[299])):
        ids = base.copy()
        ids[at] = value  # one descent at the last pair, equal neighbours at the end, the start and a workgroup's edge
        want = both(eng, (ids, np.full(n, SIZE), np.ones(n), peers, np.full((n, 1), STRONG)))
        assert want["counts"] == dict(dict.fromkeys(F.COUNTS, 0), files=n, unsorted=1)
        assert want["family"].tolist() == list(range(n)) and want["family_size"].tolist() == [1] * n
    want = both(eng, (base, np.full(n, SIZE), np.ones(n), peers, np.full((n, 1), STRONG)))
    assert want["counts"]["unsorted"] == 0 and want["counts"]["largest"] == n


# ---- the shapes: chains, stars, a random graph, one component of everything ----------------------

SHAPES = ("ascending_chain", "descending_chain", "star_on_row_0", "star_on_the_last_row", "two_interleaved_chains",
          "random", "one_component")
SIZES = (255, 256, 257, 70000)


def shape(kind, n, k=4):
    rng = np.random.default_rng(n + 1000 * SHAPES.index(kind))
    rows = np.arange(n)
    ids = (10 * rows + 7).astype(np.uint64)
    sizes = np.full(n, SIZE, np.uint64)
    pc = np.zeros(n, np.uint32)
    peers, pb = np.zeros((n, k), np.uint64), np.zeros((n, k), np.uint64)

    def first_slot(src, dst):
        pc[src], peers[src, 0], pb[src, 0] = 1, ids[dst], STRONG

    if kind == "ascending_chain":
        first_slot(rows[1:], rows[:-1])
    elif kind == "descending_chain":
        first_slot(rows[:-1], rows[1:])
    elif kind == "star_on_row_0":
        first_slot(rows[1:], 0)
    elif kind == "star_on_the_last_row":
        first_slot(rows[:-1], n - 1)
    elif kind == "two_interleaved_chains":
        first_slot(rows[2:], rows[:-2])
    elif kind == "random":
        # a few thousand groups at 70 000 rows; a row links one earlier row of its group, so a group is one
        # component; of the other slots about half are weak or missing
        groups = max(2, n // 20)
        group = rng.integers(0, groups, n)
        order = np.argsort(group, kind="stable")
        prev = np.full(n, -1)
        same = group[order][1:] == group[order][:-1]
        prev[order[1:][same]] = order[:-1][same]
        pc[:] = rng.integers(1, k + 2, n)
        peers[:, 0], pb[:, 0] = np.where(prev >= 0, ids[np.maximum(prev, 0)], ids), STRONG
        for s in range(1, k):
            kindof = rng.integers(0, 4, n)
            other = ids[rng.integers(0, n, n)]
            peers[:, s] = np.where(kindof == 0, other + np.uint64(1), other)          # 0: missing (no id ends in 8)
            pb[:, s] = np.where(kindof == 1, FAINT, np.where(kindof == 2, 0, STRONG))  # 1, 2: weak; 3: a link
            same_group = group[(peers[:, s] - np.uint64(7)) // np.uint64(10) % np.uint64(n)] == group
            pb[:, s] = np.where((kindof == 3) & ~same_group, FAINT, pb[:, s])           # links stay inside the group
    elif kind == "one_component":
        pc[:] = k
        peers[1:, 0], pb[1:, 0] = ids[(rng.random(n - 1) * rows[1:]).astype(np.int64)], STRONG  # a random earlier row
        peers[0, 0] = ids[0]
        peers[:, 1:], pb[:, 1:] = ids[rng.integers(0, n, (n, k - 1))], rng.choice([STRONG, FAINT], (n, k - 1))
    else:
        raise ValueError(kind)
    return ids, sizes, pc, peers, pb


_wanted = {}


def wanted(kind, n):
    """the shape and the reference's answer, computed once and shared"""
    if (kind, n) not in _wanted:
        g = shape(kind, n)
        _wanted[kind, n] = (g, F.families(*g))
    return _wanted[kind, n]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", SHAPES)
def test_shapes(eng, kind, n):
    g, want = wanted(kind, n)
    both(eng, g, want=want)
    c = want["counts"]
    if kind == "two_interleaved_chains":
        assert c["families"] == 2 and c["largest"] == (n + 1) // 2 and want["family"][:4].tolist() == [0, 1, 0, 1]
    elif kind == "random":
        assert c["families"] >= min(n // 40, 2000) and c["missing"] > n // 8 and c["weak"] > n // 8
        assert c["families"] < n // 4 and c["links"] > n // 2
    else:
        assert c["families"] == 1 and c["largest"] == c["members"] == n and not want["family"].any()
    # the families as sets, grouped on the device from the device's labels
    d = [torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
         for a, dt in zip(g, (np.int64, np.int64, np.int32, np.int64, np.int64))]
    family = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    eng.dev_file_families(*(t.data_ptr() for t in d), n, 4, 1, 2, family.data_ptr())
    set_rep, set_off, members = dev_sets(eng, family)
    w_rep, w_off, w_members = F.sets_of(want["family"])
    assert np.array_equal(set_rep, w_rep) and np.array_equal(set_off, w_off) and np.array_equal(members, w_members)
    assert set_rep.size == c["families"] and members.size == c["members"]


@pytest.mark.parametrize("k", [1, 64])
def test_k_1_and_k_64(eng, k):
    n = 300
    rng = np.random.default_rng(k)
    ids = np.cumsum(rng.integers(1, 9, n)).astype(np.uint64)
    sizes = rng.integers(500, 1500, n).astype(np.uint64)
    pc = rng.integers(0, k + 2, n).astype(np.uint32)
    peers = np.where(rng.random((n, k)) < 0.9, ids[rng.integers(0, n, (n, k))],
                     rng.integers(0, 9 * n, (n, k), dtype=np.uint64))
    pb = rng.integers(0, 1500, (n, k)).astype(np.uint64)
    for num, den in ((1, 2), (0, 1), (1, 1), (2, 3)):
        want = both(eng, (ids, sizes, pc, peers, pb), num, den)
    assert want["counts"]["slots"] == int(np.minimum(pc, k).sum())
    host = eng.file_families(ids, sizes, pc, peers.astype(np.uint64), pb, sets=True)
    w_rep, w_off, w_members = F.sets_of(host["family"])
    assert np.array_equal(host["set_rep"], w_rep) and np.array_equal(host["set_offsets"], w_off)
    assert np.array_equal(host["members"], w_members)


def test_null_outputs(eng):
    g, want = wanted("random", 257)
    for j in range(3):  # every single NULL output is accepted, and then all of them
        outputs = tuple(i != j for i in range(3))
        got, _ = dev_families(eng, g, outputs=outputs)
        for i, key in enumerate(("family", "family_size")):
            assert i == j or np.array_equal(got[key], want[key]), (j, key)
        assert j == 2 or got["counts"] == want["counts"]
    dev_families(eng, g, outputs=(False,) * 3)


def test_errors_leave_the_stream_empty_and_the_outputs_poisoned(eng):
    g = arrays(*shape("random", 64))
    ins = [guarded_from(a, align=8 if a.dtype.itemsize == 8 else 4) for a in g]
    outs = [Guarded(8 * 64, align=8, fill=FILL), Guarded(4 * 64, align=4, fill=FILL), Guarded(80, align=8, fill=FILL)]
    torch.cuda.synchronize()

    def call(n=64, k=4, num=1, den=2, **at):
        p = {name: x.ptr for name, x in zip(("ids", "sizes", "pc", "peers", "pb"), ins)}
        p.update({name: x.ptr for name, x in zip(("family", "fsize", "counts"), outs)})
        p.update(at)
        with pytest.raises(N.SdcasError) as ei:
            eng.dev_file_families(p["ids"], p["sizes"], p["pc"], p["peers"], p["pb"], n, k, num, den, p["family"],
                                  p["fsize"], p["counts"])
        return ei.value.code

    for bad in (dict(k=0), dict(k=65), dict(den=0), dict(num=3, den=2), dict(ids=0), dict(sizes=0), dict(pc=0),
                dict(peers=0), dict(pb=0), dict(ids=ins[0].ptr + 4), dict(sizes=ins[1].ptr + 4), dict(pc=ins[2].ptr + 2),
                dict(peers=ins[3].ptr + 4), dict(pb=ins[4].ptr + 4), dict(family=outs[0].ptr + 4),
                dict(fsize=outs[1].ptr + 2), dict(counts=outs[2].ptr + 4)):
        assert call(**bad) == N.SDCAS_E_INVALID, bad
    assert call(n=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    eng.dev_sync()
    torch.cuda.synchronize()
    assert all(o.untouched() and o.check() == [] for o in outs)
    assert all(x.unchanged() for x in ins)
    with pytest.raises(N.SdcasError) as ei:
        eng.file_families(*g, num=2, den=1)
    assert ei.value.code == N.SDCAS_E_INVALID and "threshold" in str(ei.value)
