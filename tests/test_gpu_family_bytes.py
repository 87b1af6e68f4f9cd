"""The family bytes on the GPU (sdcas_family_bytes and sdcas_dev_family_bytes,
csrc/family_bytes.hip) against the Python reference of
tests/_family_bytes_ref.py: through the host call and through the device call
over guarded buffers (inputs unchanged, guards intact, NULL outputs untouched,
every output pre-poisoned, set arrays of exactly n_files / 2 entries). Every
comparison is exact equality. No test hands the device anything meant to fault
it: every input is well formed, or is rejected before launch."""
import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests import _family_bytes_ref as R
from tests._guarded import Guarded, guarded_from

pytestmark = pytest.mark.gpu

FILL = 0xFE
M64 = (1 << 64) - 1
I64_MIN = -(1 << 63)
OUTS = R.ROWS + R.SETS + ("counts",)
DTYPES = dict(file_bytes=np.uint64, delta_bytes=np.uint64, self_bytes=np.uint64, inherited_bytes=np.uint64,
              set_rep=np.int64, set_files=np.uint32, set_total=np.uint64, set_stored=np.uint64)


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def ptr(g, used=True):
    return g.ptr if used and g.nbytes else 0


def arrays(chunk_file, chunk_len, rep, family):
    return (np.asarray(chunk_file, np.uint32).reshape(-1), np.asarray(chunk_len, np.uint64).reshape(-1),
            np.asarray(rep, np.int64).reshape(-1), np.asarray(family, np.int64).reshape(-1))


def out_guards(n):
    h = n // 2
    return [Guarded(8 * n, align=8, fill=FILL) for _ in range(4)] + \
           [Guarded(8 * h, align=8, fill=FILL), Guarded(4 * h, align=4, fill=FILL), Guarded(8 * h, align=8, fill=FILL),
            Guarded(8 * h, align=8, fill=FILL), Guarded(72, align=8, fill=FILL)]


def same(got, want):
    for name in R.ROWS + R.SETS:
        if not np.array_equal(got[name], want[name]):
            return False
    return got["counts"] == want["counts"]


def dev_bytes(eng, g, outputs=(True,) * 9):
    """sdcas_dev_family_bytes over guarded buffers -> (the outputs as a dict, their guards)"""
    cf, cl, rep, fam = g
    m, n = cf.size, fam.size
    ins = [guarded_from(cf, align=4), guarded_from(cl, align=8), guarded_from(rep, align=8), guarded_from(fam, align=8)]
    outs = out_guards(n)
    torch.cuda.synchronize()
    eng.dev_family_bytes(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), m, ptr(ins[3]), n,
                         *(ptr(o, outputs[j]) for j, o in enumerate(outs)))
    eng.dev_sync()
    torch.cuda.synchronize()
    for x in ins + outs:
        assert x.check() == []  # nothing outside any array was written
    assert all(x.unchanged() for x in ins)
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {OUTS[j]} was written"
    counts = dict(zip(R.COUNTS, (int(x) for x in outs[8].download(np.uint64))))
    got = {name: outs[j].download(DTYPES[name]) for j, name in enumerate(R.ROWS)}
    sets = counts["sets"] if outputs[8] else None
    for j, name in enumerate(R.SETS, start=4):
        got[name] = outs[j].download(DTYPES[name])
        if sets is not None and outputs[j]:
            assert sets <= n // 2
            size = np.dtype(DTYPES[name]).itemsize
            assert outs[j].untouched(lo=sets * size), f"{name} was written past the sets"
            got[name] = got[name][:sets]
    got["counts"] = counts
    return got, outs


def both(eng, g, want=None):
    """the reference against the host form and the device form, the device form twice -> the reference's dict"""
    g = arrays(*g)
    want = R.family_bytes(*g) if want is None else want
    host = eng.family_bytes(*g, sets=True)
    assert same(host, want), (host["counts"], want["counts"])
    assert np.array_equal(host["set_reclaimable"], want["set_reclaimable"])
    w_off, w_members = R.members_of(g[3], want["set_rep"])
    assert np.array_equal(host["set_offsets"], w_off) and np.array_equal(host["members"], w_members)
    a, ga = dev_bytes(eng, g)
    assert same(a, want), (a["counts"], want["counts"])
    _, gb = dev_bytes(eng, g)
    assert all((x.download() == y.download()).all() for x, y in zip(ga, gb))  # two calls give the same bytes
    return want


def confirm_style(rng, m, p_own=.5):
    """rep[rep[c]] == rep[c] <= c"""
    pos = np.arange(m, dtype=np.int64)
    own = rng.random(m) < p_own
    if m:
        own[0] = True
    last_own = np.maximum.accumulate(np.where(own, pos, 0))
    target = (rng.random(m) * (pos + 1)).astype(np.int64)
    return np.where(own, pos, last_own[np.minimum(target, pos)])


def random_case(m, n, seed=0):
    """adjacent chunks per file, labels that group nearby rows, and a few of everything out of range"""
    rng = np.random.default_rng(1000 * seed + m + n)
    pos = np.arange(m, dtype=np.int64)
    cf = np.sort(rng.integers(0, n, m)).astype(np.uint32)
    cf[rng.random(m) < .02] = n
    cf[rng.random(m) < .01] = 0xFFFFFFFF
    cl = rng.integers(0, 1 << 20, m).astype(np.uint64)
    cl[rng.random(m) < .05] = 0
    rep = np.where(rng.random(m) < .4, pos, np.maximum(pos - rng.integers(0, 200, m), 0))
    bad = rng.random(m) < .03
    rep[bad] = rng.choice(np.array([-1, I64_MIN, 1 << 40]), int(bad.sum()))
    above = rng.random(m) < .02
    rep[above] = pos[above] + 1
    rows = np.arange(n, dtype=np.int64)
    fam = np.clip(rows - rng.integers(0, 6, n), 0, None) // 4 * 4 + rng.integers(0, 2, n)
    fam = np.minimum(fam, n - 1)
    out = rng.random(n) < .05
    fam[out] = rng.choice(np.array([-1, n, I64_MIN, 1 << 33]), int(out.sum()))
    return arrays(cf, cl, rep, fam)


_wanted = {}


def wanted(m, n):
    """the case and the reference's answer, computed once and shared"""
    if (m, n) not in _wanted:
        g = random_case(m, n)
        _wanted[m, n] = (g, R.family_bytes(*g))
    return _wanted[m, n]


# ---- the small cases --------------------------------------------------------------------------

def test_nothing_one_and_two(eng):
    want = both(eng, ([], [], [], []))
    assert want["counts"] == dict.fromkeys(R.COUNTS, 0)
    want = both(eng, ([], [], [], [0, 0, 2]))  # m == 0: the rows still form a set, with zero bytes
    assert want["set_rep"].tolist() == [0] and want["set_files"].tolist() == [2] and want["set_total"].tolist() == [0]
    assert want["counts"]["files"] == 3 and want["counts"]["members"] == 2
    want = both(eng, ([0], [9], [0], [0]))
    assert want["delta_bytes"].tolist() == [9] and want["counts"]["sets"] == 0
    want = both(eng, ([0, 1], [9, 9], [0, 0], [0, 0]))
    assert want["inherited_bytes"].tolist() == [0, 9] and want["set_stored"].tolist() == [9]
    want = both(eng, ([0, 1], [9, 9], [0, 0], [0, 1]))  # two labels: the shared chunk is reclaimed by nobody
    assert want["delta_bytes"].tolist() == [9, 9] and want["counts"]["sets"] == 0
    want = both(eng, ([1, 0], [9, 9], [0, 1], []))  # no rows: no chunk takes part
    assert want["counts"] == dict.fromkeys(R.COUNTS, 0)


def test_the_worked_example(eng):
    want = both(eng, tuple(R.EXAMPLE[k] for k in ("chunk_file", "chunk_len", "rep", "family")))
    for name in R.ROWS:
        assert want[name].tolist() == R.EXAMPLE_ROWS[name]
    for name in R.SETS:
        assert want[name].tolist() == R.EXAMPLE_SETS[name]
    assert want["counts"] == R.EXAMPLE_COUNTS


# ---- the sizes: one block, its edges, past 2^16 -------------------------------------------------

@pytest.mark.parametrize("n", [1, 300, 70000])
@pytest.mark.parametrize("m", [255, 256, 257, 70000])
def test_sizes(eng, m, n):
    g, want = wanted(m, n)
    both(eng, g, want=want)
    c = want["counts"]
    assert 0 < c["chunks"] < m and c["classes"] <= c["chunks"]
    if n == 300:
        assert c["sets"] > 20 and 0 < c["files"] < n
    if n == 300 and m == 70000:
        assert want["inherited_bytes"].any() and want["self_bytes"].any() and c["set_reclaimable_bytes"] > 0


# ---- the contended inputs -----------------------------------------------------------------------

def test_one_class_in_one_family(eng):
    m = 70000
    ln = np.full(m, 4096, np.uint64)
    spread = both(eng, (np.arange(m) * 300 // m, ln, np.zeros(m), np.zeros(300)))
    assert spread["counts"]["classes"] == 1 and spread["counts"]["stored_bytes"] == 4096
    assert spread["set_files"].tolist() == [300] and spread["delta_bytes"][0] == 4096 and not spread["delta_bytes"][1:].any()
    one = both(eng, (np.zeros(m), ln, np.zeros(m), np.zeros(300)))  # all in one file
    assert one["counts"]["classes"] == 1 and one["self_bytes"][0] == 4096 * (m - 1) and one["file_bytes"][0] == 4096 * m
    # the first wave's first lane takes no part: the class's first occurrence is chunk 1, in row 5,
    # and row 0's chunks come later
    cf = np.concatenate([[300], np.full(99, 5), np.full(m - 100, 0)])
    late = both(eng, (cf, ln, np.full(m, 0), np.zeros(300)))
    assert late["delta_bytes"][5] == 4096 and late["self_bytes"][5] == 4096 * 98
    assert late["inherited_bytes"][0] == 4096 * (m - 100) and late["counts"]["chunks"] == m - 1


def test_every_chunk_its_own_class_and_one_file_of_everything(eng):
    m = 70000
    rng = np.random.default_rng(3)
    ln = rng.integers(1, 1 << 30, m).astype(np.uint64)
    want = both(eng, (np.arange(m) // 64, ln, np.arange(m), np.zeros(m // 64 + 1)))
    assert want["counts"]["classes"] == m and not want["inherited_bytes"].any() and not want["self_bytes"].any()
    want = both(eng, (np.zeros(m), ln, np.arange(m), [0, 0, 0]))  # one file holds every chunk
    assert want["delta_bytes"].tolist() == [int(ln.sum()), 0, 0] and want["set_files"].tolist() == [3]
    want = both(eng, (np.zeros(m), ln, confirm_style(rng, m), [0]))
    assert want["self_bytes"][0] > 0 and want["counts"]["sets"] == 0


def test_one_class_number_under_many_labels_does_not_merge(eng):
    m, n = 6000, 3000
    cf = np.arange(m) // 2
    want = both(eng, (cf, np.full(m, 10), np.zeros(m), np.arange(n) // 3 * 3))  # labels 0, 3, 6, ...: 1000 sets
    assert want["counts"]["classes"] == 1000 and want["counts"]["sets"] == 1000
    assert want["counts"]["stored_bytes"] == 10 * 1000 and set(want["set_stored"].tolist()) == {10}
    assert want["set_rep"].tolist() == list(range(0, n, 3))  # equal reclaimable bytes: by rep


def test_labels_that_are_not_the_lowest_row_and_labels_outside(eng):
    fam = [3, 3, -1, 3, 5, I64_MIN, 1, 1]
    cf = [0, 1, 2, 3, 4, 5, 6, 7, 8, 0xFFFFFFFF]
    want = both(eng, (cf, [8] * 10, [0] * 10, fam))
    assert want["set_rep"].tolist() == [0, 6] and want["set_files"].tolist() == [3, 2]
    assert want["file_bytes"].tolist() == [8, 8, 0, 8, 8, 0, 8, 8] and want["counts"]["files"] == 6
    assert want["counts"]["chunks"] == 6 and want["inherited_bytes"].tolist() == [0, 8, 0, 8, 0, 0, 0, 8]
    want = both(eng, ([0, 1, 2], [1, 2, 4], [0, 0, 0], [3, 3, 3]))  # the label n_files takes no part
    assert want["counts"] == dict.fromkeys(R.COUNTS, 0)


def test_reps_outside_and_lengths_zero_and_wrapping(eng):
    want = both(eng, ([0, 0, 0, 1, 1], [1, 2, 4, 8, 16], [0, 2, -1, 1, I64_MIN], [0, 0]))
    assert want["inherited_bytes"].tolist() == [0, 8] and want["counts"]["classes"] == 4
    want = both(eng, ([0, 0, 1, 1], [1 << 63, 1 << 63, 0, 1 << 63], [0, 1, 2, 0], [0, 0]))
    assert want["file_bytes"].tolist() == [0, 1 << 63] and want["counts"]["stored_bytes"] == 0
    want = both(eng, ([0, 1, 1], [M64, 2, M64], [0, 1, 0], [0, 0]))
    assert want["set_reclaimable"].tolist() == [M64] and want["counts"]["largest_reclaimable"] == M64
    m = 700  # a wave's sums wrap too
    want = both(eng, (np.arange(m) // 350, np.full(m, (1 << 63) + 1, np.uint64), np.arange(m) % 350, [0, 0]))
    assert want["delta_bytes"][0] == (350 * ((1 << 63) + 1)) & M64 and want["inherited_bytes"][1] == want["delta_bytes"][0]


def test_ties_and_sets_with_nothing_to_reclaim(eng):
    family = [5, 1, 1, 5, 4, 4, 7, 7]
    want = both(eng, ([1, 2, 4, 5, 0, 6], [6, 6, 6, 6, 3, 3], [0, 0, 2, 2, 4, 5], family))
    assert want["set_rep"].tolist() == [1, 4, 0, 6] and want["set_reclaimable"].tolist() == [6, 6, 0, 0]
    # many sets, three distinct reclaimable values: the order is (bytes descending, rep ascending)
    n = 3000
    rng = np.random.default_rng(9)
    fam = np.arange(n) // 2 * 2
    ln = rng.choice(np.array([0, 5, 9], np.uint64), n)
    want = both(eng, (np.arange(n), ln, np.arange(n) // 2 * 2, fam))
    back = want["set_reclaimable"].astype(np.int64)
    assert want["counts"]["sets"] == n // 2 and set(back.tolist()) == {0, 5, 9}
    key = list(zip((-back).tolist(), want["set_rep"].tolist()))
    assert key == sorted(key)


# ---- the laws -----------------------------------------------------------------------------------

def test_law_1_against_chunk_sharing_on_the_device(eng):
    m, n = 70000, 300
    rng = np.random.default_rng(21)
    cf = np.sort(rng.integers(0, n, m)).astype(np.uint32)
    g = arrays(cf, rng.integers(1, 1 << 20, m), confirm_style(rng, m), np.full(n, 7))
    d = [torch.from_numpy(a.view(dt)).cuda() for a, dt in zip(g, (np.int32, np.int64, np.int64, np.int64))]
    mine = [torch.full((n,), -1, dtype=torch.int64, device="cuda") for _ in range(4)]
    theirs = [torch.full((n,), -1, dtype=torch.int64, device="cuda") for _ in range(3)]
    cts, scts = torch.zeros(9, dtype=torch.int64, device="cuda"), torch.zeros(6, dtype=torch.int64, device="cuda")
    eng.dev_family_bytes(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, d[3].data_ptr(), n,
                         *(t.data_ptr() for t in mine), counts=cts.data_ptr())
    eng.dev_chunk_sharing(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, n, *(t.data_ptr() for t in theirs),
                          counts=scts.data_ptr())
    eng.dev_sync()
    torch.cuda.synchronize()
    for a, b in zip(mine[1:], theirs):  # delta / self / inherited are new / self / other
        assert torch.equal(a, b)
    assert torch.equal(mine[0], theirs[0] + theirs[1] + theirs[2])
    assert int(cts[4]) == int(scts[4]) and int(cts[3]) == int(scts[3])  # stored_bytes, total_bytes
    assert int(theirs[2].sum()) > 0 and int(theirs[1].sum()) > 0
    want = R.family_bytes(*g)
    assert [int(x) for x in cts.cpu()] == [want["counts"][k] for k in R.COUNTS]


def test_law_2_every_row_its_own_label(eng):
    g, _ = wanted(70000, 300)
    want = both(eng, (g[0], g[1], g[2], np.arange(300)))
    assert not want["inherited_bytes"].any() and want["set_rep"].size == 0 and want["counts"]["sets"] == 0


# ---- the workspace, the outputs, the errors -------------------------------------------------------

def test_a_dirty_workspace_changes_nothing(eng):
    big, want_big = wanted(70000, 70000)
    small, want_small = wanted(255, 300)
    a, ga = dev_bytes(eng, big)
    b, _ = dev_bytes(eng, small)
    c, gc = dev_bytes(eng, big)
    assert same(a, want_big) and same(b, want_small) and same(c, want_big)
    assert all((x.download() == y.download()).all() for x, y in zip(ga, gc))


def test_null_outputs(eng):
    g, want = wanted(257, 300)
    for j in range(9):  # every single NULL output is accepted, and then all of them
        outputs = tuple(i != j for i in range(9))
        got, _ = dev_bytes(eng, g, outputs=outputs)
        sets = want["counts"]["sets"]
        for i, key in enumerate(R.ROWS + R.SETS):
            assert i == j or np.array_equal(got[key][:sets] if i >= 4 else got[key], want[key]), (j, key)
        assert j == 8 or got["counts"] == want["counts"]
    dev_bytes(eng, g, outputs=(False,) * 9)
    dev_bytes(eng, g, outputs=(True,) * 4 + (False,) * 4 + (True,))  # no set array: no order is computed


def test_errors_leave_the_stream_empty_and_the_outputs_poisoned(eng):
    g, _ = wanted(256, 300)
    ins = [guarded_from(a, align=4 if a.dtype.itemsize == 4 else 8) for a in g]
    outs = out_guards(300)
    names = ("cf", "cl", "rep", "fam") + OUTS
    torch.cuda.synchronize()

    def call(m=256, n=300, **at):
        p = {name: x.ptr for name, x in zip(names, ins + outs)}
        p.update(at)
        with pytest.raises(N.SdcasError) as ei:
            eng.dev_family_bytes(p["cf"], p["cl"], p["rep"], m, p["fam"], n, *(p[name] for name in OUTS))
        return ei.value.code

    for bad in (dict(cf=0), dict(cl=0), dict(rep=0), dict(fam=0), dict(cf=ins[0].ptr + 2), dict(cl=ins[1].ptr + 4),
                dict(rep=ins[2].ptr + 4), dict(fam=ins[3].ptr + 4), dict(set_files=outs[5].ptr + 2)):
        assert call(**bad) == N.SDCAS_E_INVALID, bad
    for name in OUTS:
        if name != "set_files":
            assert call(**{name: outs[OUTS.index(name)].ptr + 4}) == N.SDCAS_E_INVALID, name
    assert call(m=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    assert call(n=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    eng.dev_sync()
    torch.cuda.synchronize()
    assert all(o.untouched() and o.check() == [] for o in outs)
    assert all(x.unchanged() for x in ins)
    cf, cl, rep, fam = g
    L = eng.L
    for args in ((None, cl, rep, fam), (cf, None, rep, fam), (cf, cl, None, fam), (cf, cl, rep, None)):
        p = [a.ctypes.data if a is not None else None for a in args]
        assert L.sdcas_family_bytes(eng.ctx, p[0], p[1], p[2], 256, p[3], 300, *([None] * 9)) == N.SDCAS_E_INVALID
    assert L.sdcas_family_bytes(eng.ctx, None, None, None, 0, None, 0, *([None] * 9)) == N.SDCAS_OK
