"""The family recipes on the GPU (sdcas_family_recipes and
sdcas_dev_family_recipes, csrc/family_recipes.hip) against the Python reference
of tests/_family_recipes_ref.py: through the host call and through the device
call over guarded buffers (inputs unchanged, guards intact, NULL outputs
untouched, every output pre-poisoned, op arrays untouched past `ops`, two device
calls with equal bytes). Every comparison is exact equality. No test hands the
device anything meant to fault it: every input is well formed, or is rejected
before launch."""
import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from spacedrive_amd import rebuild_files
from tests import _family_bytes_ref as B
from tests import _family_recipes_ref as R
from tests._guarded import Guarded, guarded_from

pytestmark = pytest.mark.gpu

FILL = 0xFE
M64 = (1 << 64) - 1
I64_MIN = -(1 << 63)
NAMES = R.OPS + ("chunk_op",) + R.ROWS
OUTS = NAMES + ("counts",)
DTYPES = {name: np.uint32 for name in R.OPS32 + ("chunk_op",) + R.ROWS}
DTYPES.update({name: np.uint64 for name in R.OPS64})


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def ptr(g, used=True):
    return g.ptr if used and g.nbytes else 0


def arrays(chunk_file, chunk_off, chunk_len, rep, family):
    cf, ln = np.asarray(chunk_file, np.uint32).reshape(-1), np.asarray(chunk_len, np.uint64).reshape(-1)
    off = R.running_offsets(cf, ln) if chunk_off is None else np.asarray(chunk_off, np.uint64).reshape(-1)
    return cf, off, ln, np.asarray(rep, np.int64).reshape(-1), np.asarray(family, np.int64).reshape(-1)


def out_guards(m, n):
    return [Guarded(4 * m, align=4, fill=FILL) for _ in range(4)] + \
           [Guarded(8 * m, align=8, fill=FILL) for _ in range(3)] + \
           [Guarded(4 * m, align=4, fill=FILL), Guarded(4 * n, align=4, fill=FILL), Guarded(4 * n, align=4, fill=FILL),
            Guarded(64, align=8, fill=FILL)]


def dev_recipes(eng, g, outputs=(True,) * 11):
    """sdcas_dev_family_recipes over guarded buffers -> (the outputs as a dict, their guards)"""
    cf, off, ln, rep, fam = g
    m, n = cf.size, fam.size
    ins = [guarded_from(cf, align=4)] + [guarded_from(a, align=8) for a in (off, ln, rep, fam)]
    outs = out_guards(m, n)
    torch.cuda.synchronize()
    eng.dev_family_recipes(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), m, ptr(ins[4]), n,
                           *(ptr(o, outputs[j]) for j, o in enumerate(outs)))
    eng.dev_sync()
    torch.cuda.synchronize()
    for x in ins + outs:
        assert x.check() == []  # nothing outside any array was written
    assert all(x.unchanged() for x in ins)
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {OUTS[j]} was written"
    counts = dict(zip(R.COUNTS, (int(x) for x in outs[10].download(np.uint64))))
    ops = counts["ops"] if outputs[10] else None
    got = {}
    for j, name in enumerate(NAMES):
        got[name] = outs[j].download(DTYPES[name])
        if j < 7 and ops is not None and outputs[j]:
            assert ops <= m
            assert outs[j].untouched(lo=ops * np.dtype(DTYPES[name]).itemsize), f"{name} was written past the ops"
            got[name] = got[name][:ops]
    got["counts"] = counts
    return got, outs


def both(eng, g, want=None):
    """the reference against the host form and the device form, the device form twice -> the reference's dict"""
    g = arrays(*g)
    want = R.family_recipes(*g) if want is None else want
    cf, off, ln, rep, fam = g
    host = eng.family_recipes(cf, ln, rep, fam, chunk_off=off)
    assert R.same(host, want), (host["counts"], want["counts"])
    assert np.array_equal(host["op_literal"], want["op_literal"]) and host["op_chunk"].size == want["counts"]["ops"]
    a, ga = dev_recipes(eng, g)
    assert R.same(a, want), (a["counts"], want["counts"])
    _, gb = dev_recipes(eng, g)
    assert all((x.download() == y.download()).all() for x, y in zip(ga, gb))  # two calls give the same bytes
    return want


def random_case(m, n, seed=0):
    """Adjacent chunks per file; stretches of new chunks and stretches that repeat the stretch before them
    chunk for chunk (the same lengths, so that copies form runs); labels that group nearby rows; a few
    files, labels and reps out of range, a few lengths zero. The offsets are the running sums."""
    rng = np.random.default_rng(1000 * seed + 7 * m + n)
    pos = np.arange(m, dtype=np.int64)
    cf = np.sort(rng.integers(0, n, m)).astype(np.uint32)
    ln = rng.integers(1, 1 << 20, m).astype(np.uint64)
    ln[rng.random(m) < .03] = 0
    rep = pos.copy()
    at, prev = 0, None  # prev: the last stretch of new chunks
    while at < m:
        k = min(int(rng.integers(1, 90)), m - at)
        if prev is not None and rng.random() < .5:
            k = min(k, prev[1])
            s = prev[0] + int(rng.integers(0, prev[1] - k + 1))
            rep[at:at + k] = pos[s:s + k]
            ln[at:at + k] = ln[s:s + k]
        else:
            prev = (at, k)
        at += k
    cf[rng.random(m) < .004] = n
    cf[rng.random(m) < .002] = 0xFFFFFFFF
    bad = rng.random(m) < .005
    rep[bad] = rng.choice(np.array([-1, I64_MIN, 1 << 40]), int(bad.sum()))
    above = rng.random(m) < .003
    rep[above] = pos[above] + 1
    rows = np.arange(n, dtype=np.int64)
    fam = np.minimum(rows // 4 * 4 + rng.integers(0, 2, n), n - 1)
    out = rng.random(n) < .03
    fam[out] = rng.choice(np.array([-1, n, I64_MIN, 1 << 33]), int(out.sum()))
    return arrays(cf, None, ln, rep, fam)


_wanted = {}


def wanted(m, n):
    """the case and the reference's answer, computed once and shared"""
    if (m, n) not in _wanted:
        g = random_case(m, n)
        _wanted[m, n] = (g, R.family_recipes(*g))
    return _wanted[m, n]


def one_run(m, rng=None):
    """one file, every chunk new: one literal op"""
    ln = np.full(m, 4096, np.uint64) if rng is None else rng.integers(1, 1 << 30, m).astype(np.uint64)
    return arrays(np.zeros(m), None, ln, np.arange(m), [0])


# ---- the small cases --------------------------------------------------------------------------

def test_nothing_one_and_two(eng):
    want = both(eng, ([], [], [], [], []))
    assert want["counts"] == dict.fromkeys(R.COUNTS, 0)
    want = both(eng, ([], [], [], [], [0, 0, 2]))  # m == 0: the rows take part and have no ops
    assert want["counts"] == dict(dict.fromkeys(R.COUNTS, 0), files=3)
    assert want["row_ops"].tolist() == [0, 0, 0] and want["row_first_op"].tolist() == [R.NONE] * 3
    want = both(eng, ([0], [5], [9], [0], [0]))
    assert want["op_len"].tolist() == [9] and want["op_dst_off"].tolist() == [5] and want["op_literal"].tolist() == [True]
    want = both(eng, ([0, 1], [0, 0], [9, 9], [0, 0], [0, 0]))
    assert want["op_literal"].tolist() == [True, False] and want["op_src_row"].tolist() == [0, 0]
    want = both(eng, ([0, 1], [0, 0], [9, 9], [0, 0], [0, 1]))  # two labels: each keeps its own
    assert want["op_literal"].tolist() == [True, True]
    want = both(eng, ([1, 0], [0, 0], [9, 9], [0, 1], []))  # no rows: no chunk takes part, every chunk_op says so
    assert want["counts"] == dict.fromkeys(R.COUNTS, 0) and want["chunk_op"].tolist() == [R.NONE, R.NONE]


def test_the_worked_example(eng):
    want = both(eng, tuple(R.EXAMPLE[k] for k in ("chunk_file", "chunk_off", "chunk_len", "rep", "family")))
    for name in R.OPS:
        assert want[name].tolist() == R.EXAMPLE_OPS[name]
    for name, v in R.EXAMPLE_REST.items():
        assert want[name].tolist() == v
    assert want["counts"] == R.EXAMPLE_COUNTS
    host = eng.family_recipes(R.EXAMPLE["chunk_file"], R.EXAMPLE["chunk_len"], R.EXAMPLE["rep"], R.EXAMPLE["family"])
    assert host["chunk_off"].tolist() == R.EXAMPLE["chunk_off"] and R.same(host, want)  # the offsets by default
    v1, v2 = bytes(range(60)), bytes(range(30)) + b"XXXXX" + bytes(range(30, 60))
    assert rebuild_files(host, lambda r, o, n: (v1, v2)[r][o:o + n]) == {0: v1, 1: v2}


# ---- the sizes: a wave, a workgroup, their edges, several workgroups ------------------------------

SIZES = [(0, 1), (1, 1), (2, 1), (2, 2), (63, 1), (63, 63), (64, 9), (65, 65), (255, 1), (255, 40), (256, 256),
         (257, 30), (1025, 1), (1025, 100), (1025, 1025), (5000, 1), (5000, 300), (5000, 5000)]


@pytest.mark.parametrize("m,n", SIZES)
def test_sizes(eng, m, n):
    g, want = wanted(m, n)
    both(eng, g, want=want)
    c = want["counts"]
    assert c["ops"] == c["literal_ops"] + c["copy_ops"] <= c["chunks"] <= m
    if m >= 1025 and n <= 300:
        assert 0 < c["copy_ops"] and c["ops"] < c["chunks"] < m and c["longest_op"] > 1 << 20


def test_laws_on_the_device_output(eng):
    """law 1 against the family bytes' reference, laws 2 and 3 through rebuild_files over bytes that
    agree with rep: the host form's dict is what a caller applies"""
    contents, cf, off, ln, rep, fam = R.versions(11, n_families=40, max_versions=6, blocks=30)
    assert cf.size > 1500
    got = eng.family_recipes(cf, ln, rep, fam)  # the offsets by default
    assert np.array_equal(got["chunk_off"], off)
    assert R.same(got, R.family_recipes(cf, off, ln, rep, fam))
    fb = B.family_bytes(cf, ln, rep, fam)
    n = fam.size
    lit, cp = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    np.add.at(lit, got["op_row"][got["op_literal"]], got["op_len"][got["op_literal"]])
    np.add.at(cp, got["op_row"][~got["op_literal"]], got["op_len"][~got["op_literal"]])
    assert np.array_equal(lit, fb["delta_bytes"]) and np.array_equal(cp, fb["self_bytes"] + fb["inherited_bytes"])
    assert got["counts"]["literal_bytes"] == fb["counts"]["stored_bytes"]
    reads = []

    def read(row, at, k):
        reads.append(k)
        return contents[row][at:at + k]
    built = rebuild_files(got, read)
    for i in range(n):
        assert built[i] == (contents[i] if 0 <= fam[i] < n else b"")
    assert sum(reads) == got["counts"]["literal_bytes"] < sum(len(x) for x in contents)
    own = eng.family_recipes(cf, ln, rep, np.arange(n))  # law 4
    assert np.array_equal(own["op_src_row"], own["op_row"]) and (~own["op_literal"]).any()
    assert rebuild_files(own, lambda r, a, k: contents[r][a:a + k]) == dict(enumerate(contents))


# ---- runs: one of everything, none, and boundaries at the wave's and the workgroup's edge ---------

@pytest.mark.parametrize("m", [64, 257, 1025, 5000])
def test_one_run_of_all_chunks(eng, m):
    g = one_run(m, np.random.default_rng(m))
    want = both(eng, g)
    assert want["counts"]["ops"] == 1 and want["op_len"].tolist() == [int(g[2].sum())]
    assert not want["chunk_op"].any() and want["row_ops"].tolist() == [1]
    # and as one copy run: a second file that repeats the first, chunk for chunk
    cf = np.concatenate([np.zeros(m), np.ones(m)])
    want = both(eng, (cf, None, np.tile(g[2], 2), np.tile(np.arange(m), 2), [0, 0]))
    assert want["op_literal"].tolist() == [True, False] and want["op_len"].tolist() == [int(g[2].sum())] * 2
    assert want["op_src_off"].tolist() == [0, 0] and want["row_first_op"].tolist() == [0, 1]


@pytest.mark.parametrize("m", [65, 256, 1025, 5000])
def test_no_runs_literal_and_copy_alternate(eng, m):
    pos = np.arange(m)
    want = both(eng, (np.zeros(m), None, np.full(m, 8), pos - (pos & 1), [0]))  # every odd chunk repeats the one before
    assert want["counts"]["ops"] == m and want["op_literal"].tolist() == [c % 2 == 0 for c in range(m)]
    assert want["row_ops"].tolist() == [m] and want["chunk_op"].tolist() == list(range(m))
    want = both(eng, (pos * 7 // m, None, np.full(m, 8), pos - (pos & 1), np.zeros(7)))  # and over seven files
    assert want["counts"]["ops"] == m and int(want["row_ops"].sum()) == m


BREAKS = [62, 63, 64, 65, 254, 255, 256, 257]


@pytest.mark.parametrize("at", BREAKS + [tuple(BREAKS)])
def test_run_boundaries_at_the_edges(eng, at):
    """one file of new chunks whose offsets jump before the chunks `at`: an op ends at at - 1, one starts at `at`"""
    m = 600
    at = (at,) if isinstance(at, int) else at
    rng = np.random.default_rng(at[0])
    cf, off, ln, rep, fam = one_run(m, rng)
    off = off.copy()
    for p in at:
        off[p:] += np.uint64(1)
    want = both(eng, (cf, off, ln, rep, fam))
    assert want["op_chunk"].tolist() == [0] + list(at)
    edges = [0] + list(at) + [m]
    assert want["op_len"].tolist() == [int(ln[a:b].sum()) for a, b in zip(edges, edges[1:])]
    # the same boundaries between a literal run and a copy run, and between two copy runs from two sources
    half = m // 2
    for p in at:
        if p >= half:
            continue
        rep2 = np.arange(m)
        rep2[half + p:] = np.arange(p, half)[:m - half - p]  # file 0's chunks from p on, again
        ln2 = ln.copy()
        ln2[half + p:] = ln[p:half][:m - half - p]
        want = both(eng, (np.zeros(m), None, ln2, rep2, [0]))
        assert want["op_chunk"].tolist() == [0, half + p] and want["op_literal"].tolist() == [True, False]


# ---- the contended inputs -----------------------------------------------------------------------

def test_one_class_in_one_family(eng):
    m = 5000
    ln = np.full(m, 4096, np.uint64)
    spread = both(eng, (np.arange(m) * 300 // m, None, ln, np.zeros(m), np.zeros(300)))
    assert spread["counts"]["literal_ops"] == 1 and spread["counts"]["copy_ops"] == m - 1  # the source never advances
    assert not spread["op_src_chunk"].any() and spread["counts"]["literal_bytes"] == 4096
    one = both(eng, (np.zeros(m), None, ln, np.zeros(m), np.zeros(300)))  # all in one file
    assert one["row_ops"][0] == m and one["counts"]["copy_bytes"] == 4096 * (m - 1)
    # the first wave's first lane takes no part: the class's first occurrence is chunk 1
    cf = np.concatenate([[300], np.full(99, 5), np.full(m - 100, 0)])
    late = both(eng, (cf, None, ln, np.zeros(m), np.zeros(300)))
    assert late["chunk_op"][0] == R.NONE and late["op_chunk"][0] == 1 and late["op_src_chunk"].tolist() == [1] * (m - 1)


def test_one_file_holds_every_chunk(eng):
    g, _ = wanted(5000, 300)
    cf, off, ln, rep, fam = g
    want = both(eng, (np.zeros(5000), None, ln, rep, [0, 0, 0]))
    assert want["row_ops"].tolist() == [want["counts"]["ops"], 0, 0] and want["counts"]["copy_ops"] > 0
    assert want["row_first_op"].tolist() == [0, R.NONE, R.NONE]


def test_every_row_its_own_label_and_all_rows_outside(eng):
    g, _ = wanted(5000, 300)
    cf, off, ln, rep, fam = g
    want = both(eng, (cf, off, ln, rep, np.arange(300)))  # law 4
    assert np.array_equal(want["op_src_row"], want["op_row"]) and want["counts"]["files"] == 300
    for fam2 in (np.full(300, -1), np.full(300, 300), np.full(300, I64_MIN)):
        want = both(eng, (cf, off, ln, rep, fam2))
        assert want["counts"] == dict.fromkeys(R.COUNTS, 0) and (want["chunk_op"] == R.NONE).all()
        assert not want["row_ops"].any() and (want["row_first_op"] == R.NONE).all()


def test_interleaved_rows_zero_lengths_and_wrapping(eng):
    m = 700
    pos = np.arange(m)
    want = both(eng, (pos & 1, None, np.full(m, 4), pos, [0, 0]))  # two rows, chunk about: no run survives
    assert want["counts"]["ops"] == m and want["row_ops"].tolist() == [350, 350]
    assert want["row_first_op"].tolist() == [0, 1]
    want = both(eng, (pos & 1, None, np.full(m, 4), pos - (pos & 1), [0, 0]))  # row 1 repeats row 0
    assert want["op_literal"].tolist() == [c % 2 == 0 for c in range(m)]
    want = both(eng, ([0, 0, 0], [0, 0, 4], [4, 4, 4], [0, 0, 2], [0]))  # two chunks of one row at one offset
    assert want["op_literal"].tolist() == [True, False, True]
    want = both(eng, ([0, 0], [0, 0], [0, 0], [0, 0], [0]))  # a zero-length literal and its copy at one offset
    assert want["counts"]["ops"] == 2
    want = both(eng, ([0, 0, 0, 1, 1], [0, 3, 3, 0, 0], [3, 0, 2, 0, 0], [0, 1, 2, 1, 1], [0, 0]))
    assert want["op_len"].tolist() == [5, 0]
    big = (1 << 63) + 1  # offsets and lengths wrap: all arithmetic is modulo 2^64
    want = both(eng, (np.zeros(m), None, np.full(m, big, np.uint64), pos, [0]))
    assert want["counts"]["ops"] == 1 and want["op_len"].tolist() == [(m * big) & M64]
    want = both(eng, ([0, 0, 1], [M64, 1, 5], [2, 3, 2], [0, 1, 0], [0, 0]))
    assert want["op_len"].tolist() == [5, 2] and want["counts"]["longest_op"] == 5


def test_more_workgroup_counts_than_one_pass_of_the_scan(eng):
    m, n = 262145, 4096  # 1025 counts: the one-workgroup scan carries into a second pass
    g, want = wanted(m, n)
    both(eng, g, want=want)
    c = want["counts"]
    assert 0 < c["copy_ops"] and c["ops"] < c["chunks"] < m
    assert want["chunk_op"][-1] in (c["ops"] - 1, R.NONE) and int(want["row_ops"].sum()) == c["ops"]
    got, _ = dev_recipes(eng, one_run(m))  # one op over every workgroup
    assert got["counts"]["ops"] == 1 and got["op_len"].tolist() == [4096 * m] and not got["chunk_op"].any()


# ---- the workspace, the outputs, the errors -------------------------------------------------------

def test_a_dirty_workspace_changes_nothing(eng):
    big, want_big = wanted(5000, 5000)
    small, want_small = wanted(255, 40)
    a, ga = dev_recipes(eng, big)
    b, _ = dev_recipes(eng, small)
    c, gc = dev_recipes(eng, big)
    assert R.same(a, want_big) and R.same(b, want_small) and R.same(c, want_big)
    assert all((x.download() == y.download()).all() for x, y in zip(ga, gc))


def test_null_outputs(eng):
    g, want = wanted(257, 30)
    ops = want["counts"]["ops"]
    for j in range(11):  # every single NULL output is accepted, and then all of them
        outputs = tuple(i != j for i in range(11))
        got, _ = dev_recipes(eng, g, outputs=outputs)
        for i, key in enumerate(NAMES):
            assert i == j or np.array_equal(got[key][:ops] if i < 7 else got[key], want[key]), (j, key)
        assert j == 10 or got["counts"] == want["counts"]
    dev_recipes(eng, g, outputs=(False,) * 11)
    got, _ = dev_recipes(eng, g, outputs=(False,) * 10 + (True,))  # only the counts are asked for
    assert got["counts"] == want["counts"]


def test_errors_leave_the_stream_empty_and_the_outputs_poisoned(eng):
    g, _ = wanted(256, 256)
    m, n = 256, 256
    ins = [guarded_from(a, align=4 if a.dtype.itemsize == 4 else 8) for a in g]
    outs = out_guards(m, n)
    names = ("cf", "off", "ln", "rep", "fam") + OUTS
    torch.cuda.synchronize()

    def call(m=m, n=n, **at):
        p = {name: x.ptr for name, x in zip(names, ins + outs)}
        p.update(at)
        with pytest.raises(N.SdcasError) as ei:
            eng.dev_family_recipes(p["cf"], p["off"], p["ln"], p["rep"], m, p["fam"], n, *(p[name] for name in OUTS))
        return ei.value.code

    for bad in (dict(cf=0), dict(off=0), dict(ln=0), dict(rep=0), dict(fam=0), dict(cf=ins[0].ptr + 2),
                dict(off=ins[1].ptr + 4), dict(ln=ins[2].ptr + 4), dict(rep=ins[3].ptr + 4), dict(fam=ins[4].ptr + 4)):
        assert call(**bad) == N.SDCAS_E_INVALID, bad
    for j, name in enumerate(OUTS):
        assert call(**{name: outs[j].ptr + (2 if DTYPES.get(name) == np.uint32 else 4)}) == N.SDCAS_E_INVALID, name
    assert call(m=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    assert call(n=(1 << 30) + 1) == N.SDCAS_E_CAPACITY
    eng.dev_sync()
    torch.cuda.synchronize()
    assert all(o.untouched() and o.check() == [] for o in outs)
    assert all(x.unchanged() for x in ins)
    cf, off, ln, rep, fam = g
    L = eng.L
    for args in ((None, off, ln, rep, fam), (cf, None, ln, rep, fam), (cf, off, None, rep, fam),
                 (cf, off, ln, None, fam), (cf, off, ln, rep, None)):
        p = [a.ctypes.data if a is not None else None for a in args]
        assert L.sdcas_family_recipes(eng.ctx, p[0], p[1], p[2], p[3], m, p[4], n, *([None] * 11)) == N.SDCAS_E_INVALID
    assert L.sdcas_family_recipes(eng.ctx, None, None, None, None, 0, None, 0, *([None] * 11)) == N.SDCAS_OK
    with pytest.raises(N.SdcasError) as ei:
        eng.family_recipes_plan((1 << 30) + 1, 1)
    assert ei.value.code == N.SDCAS_E_CAPACITY
