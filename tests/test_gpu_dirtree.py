"""Directory digests and top-most duplicates on the GPU (sdcas_tree_digests /
sdcas_dev_tree_digests / sdcas_tree_top / sdcas_dev_tree_top, csrc/dirtree.hip):
every output array and all counts against tests/_tree_ref.py, through the host
call and through the device call with torch tensors, twice each on a workspace
earlier cases left dirty. The shapes are the smallest at which each mechanism
can go wrong: BLAKE3's block / chunk / 1 MiB boundaries in M(d) = 16 + 72 k
bytes, the sort's tile of 4096, runs of equal 8-byte name prefixes, depth."""
import os
import shutil
import stat

import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests import _tree_ref as R
from tests._guarded import Guarded, guarded_from
from tests._oracle import load_oracle

pytestmark = pytest.mark.gpu

TILE = 4096  # csrc/dupsets.h kDupsetsTile: items per workgroup of the sort
OUTS = ("keys", "digests", "valid", "tree_bytes", "tree_files", "flags", "counts")
P8, P64 = 0xA5, 0xA5A5A5A5A5A5A5A5  # what the directory slots hold before a call


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle():
    return load_oracle()


# ---- cases -------------------------------------------------------------------------

class Case:
    """a tree with everything the calls read: names, the file entries'
    digests / keys / valid (the directory slots poisoned), sizes"""

    def __init__(self, parent, is_dir, seed=1, names=None, valid=True, sizes=True):
        self.parent = np.ascontiguousarray(parent, np.int64)
        self.is_dir = np.ascontiguousarray(is_dir, np.uint8)
        n = self.n = self.parent.size
        rng = np.random.default_rng(seed)
        d = self.is_dir != 0
        self.names = rng.integers(0, 256, (n, 32), dtype=np.uint8) if names is None else \
            np.ascontiguousarray(names, np.uint8).reshape(n, 32)
        self.digests = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.digests[d] = P8
        self.keys = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        self.keys[d] = P64
        self.valid = None
        if valid is not None:
            self.valid = np.ones(n, np.uint8) if valid is True else np.ascontiguousarray(valid, np.uint8).copy()
            self.valid[d] = P8
        self.sizes = None
        if sizes is not None:
            self.sizes = rng.integers(0, 1 << 20, n, dtype=np.uint64) if sizes is True else \
                np.ascontiguousarray(sizes, np.uint64)
        self._want = None

    def want(self, oracle):
        if self._want is None:  # computed once, shared by the four calls
            self._want = R.tree_digests(oracle, self.parent, self.is_dir, self.names, self.digests, self.valid,
                                        self.sizes, self.keys)
        return self._want


def flat(k, **kw):
    """one directory of k files"""
    return Case(np.r_[-1, np.zeros(k, np.int64)], np.r_[1, np.zeros(k, np.uint8)].astype(np.uint8), **kw)


def chain(depth, **kw):
    """`depth` directories inside one another, one file at the bottom"""
    return Case(np.arange(-1, depth, dtype=np.int64), np.r_[np.ones(depth, np.uint8), 0].astype(np.uint8), **kw)


# ---- the calls ---------------------------------------------------------------------

def _t(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda() if a.size else \
        torch.zeros(16, dtype=torch.uint8, device="cuda")


def device_call(eng, c, outputs=OUTS, stream=0):
    """sdcas_dev_tree_digests over torch tensors -> dict of host arrays;
    outputs: which of OUTS are passed (digests always is: it is an input)"""
    n = c.n
    t = {"names": _t(c.names), "digests": _t(c.digests), "keys": _t(c.keys),
         "valid": _t(c.valid if c.valid is not None else np.full(n, P8, np.uint8)),
         "sizes": _t(c.sizes) if c.sizes is not None else None,
         "tree_bytes": _t(np.full(n, P64, np.uint64)), "tree_files": _t(np.full(n, P64, np.uint64)),
         "flags": _t(np.full(n, P8, np.uint8)), "counts": _t(np.full(6, P64, np.uint64))}
    torch.cuda.synchronize()
    p = lambda k: t[k].data_ptr() if k in outputs and (n or k == "counts") else 0
    eng.dev_tree_digests(c.parent, c.is_dir, t["names"].data_ptr() if n else 0,
                         t["sizes"].data_ptr() if t["sizes"] is not None and n else 0, n, p("keys"),
                         t["digests"].data_ptr() if n else 0, p("valid") if c.valid is not None else 0,
                         p("tree_bytes"), p("tree_files"), p("flags"), p("counts"), stream)
    eng.dev_sync(stream)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in t.items() if v is not None}
    got = {"keys": host["keys"].view(np.uint64)[:n], "digests": host["digests"][:32 * n].reshape(n, 32),
           "valid": host["valid"][:n], "tree_bytes": host["tree_bytes"].view(np.uint64)[:n],
           "tree_files": host["tree_files"].view(np.uint64)[:n], "flags": host["flags"][:n],
           "counts": dict(zip(R.TREE_COUNTS, (int(x) for x in host["counts"].view(np.uint64))))}
    assert (host["names"][:32 * n] == c.names.reshape(-1)).all(), "the names were written"
    return got


def compare(how, got, want, c, outputs=OUTS):
    """every passed output equals the checker's; a null one holds what it held"""
    n = c.n
    before = {"keys": c.keys, "valid": c.valid if c.valid is not None else np.full(n, P8, np.uint8),
              "tree_bytes": np.full(n, P64, np.uint64), "tree_files": np.full(n, P64, np.uint64),
              "flags": np.full(n, P8, np.uint8)}
    for k in OUTS:
        if k == "counts":
            if k in outputs:
                assert got[k] == want[k], f"{how} counts: {got[k]} != {want[k]}"
            else:
                assert set(got[k].values()) == {P64}, f"{how}: null counts were written"
            continue
        w = want[k] if k in outputs and (k != "valid" or c.valid is not None) else before[k]
        g = got[k]
        assert g.shape == w.shape, f"{how} {k}: {g.shape} != {w.shape}"
        bad = np.flatnonzero((g != w).reshape(n, -1).any(axis=1)) if n else np.zeros(0, np.int64)
        assert bad.size == 0, f"{how} {k}: {bad.size} entries differ, first {bad[:5]}: {g[bad[:3]]} != {w[bad[:3]]}"


def host_call(eng, c):
    ks, dig, va, tb, tf, fl, counts = eng.tree_digests(c.parent, c.is_dir, c.names, c.digests, c.valid, c.sizes,
                                                       c.keys)
    return {"keys": ks, "digests": dig, "valid": va if va is not None else np.full(c.n, P8, np.uint8),
            "tree_bytes": tb, "tree_files": tf, "flags": fl, "counts": counts}


def check(eng, oracle, c):
    want = c.want(oracle)
    for again in range(2):
        compare(f"host call {again}", host_call(eng, c), want, c)
        compare(f"device call {again}", device_call(eng, c), want, c)
    return want


# ---- smallest trees ------------------------------------------------------------------

def test_no_entries(eng):
    c = Case([], [])
    got = device_call(eng, c)
    assert got["counts"] == dict.fromkeys(R.TREE_COUNTS, 0)
    assert host_call(eng, c)["counts"] == dict.fromkeys(R.TREE_COUNTS, 0)
    assert device_call(eng, c, outputs=())["counts"] == dict.fromkeys(R.TREE_COUNTS, P64)


@pytest.mark.parametrize("parent,is_dir", [([-1], [0]), ([-1], [1]), ([-1, 0], [1, 0]), ([1, -1], [0, 1])],
                         ids=["file", "empty-dir", "dir-file", "file-dir"])
def test_smallest_trees(eng, oracle, parent, is_dir):
    want = check(eng, oracle, Case(parent, is_dir))
    if is_dir == [1]:
        assert want["flags"][0] == R.DIR | R.EMPTY and want["valid"][0] == 0 and want["digests"][0].any()


# ---- BLAKE3's boundaries in M(d) -------------------------------------------------------

@pytest.mark.parametrize("k", [6, 13, 14, 15, 28, 29, 14563, 14564, 70001])
def test_message_length_boundaries(eng, oracle, k):
    """448 B is 7 blocks, 1024 B (k = 14) one chunk, k = 14563 / 14564 either
    side of 1 MiB (the batch hash's tile), 70 001 children a 5 MB message"""
    want = check(eng, oracle, flat(k, seed=k))
    assert want["counts"]["largest_dir"] == k and want["tree_files"][0] == k


# ---- the sort and its tile -------------------------------------------------------------

@pytest.mark.parametrize("k", [TILE - 1, TILE, TILE + 1])
def test_one_directory_around_the_tile(eng, oracle, k):
    check(eng, oracle, flat(k - 1, seed=k))  # k entries with the directory itself
    check(eng, oracle, flat(k, seed=k + 7))


def test_interleaved_and_striped_directories(eng, oracle):
    # two directories whose children alternate lane by lane in entry order
    n = 2 + 600
    parent = np.r_[-1, -1, np.arange(600) % 2]
    check(eng, oracle, Case(parent, np.r_[1, 1, np.zeros(600, np.uint8)].astype(np.uint8), seed=3))
    # 8 tiles + 1 entries under 3 striped directories
    n = 8 * TILE + 1
    parent = np.r_[-1, -1, -1, np.arange(n - 3) % 3]
    check(eng, oracle, Case(parent, np.r_[1, 1, 1, np.zeros(n - 3, np.uint8)].astype(np.uint8), seed=4))


def test_descending_names_and_parents_after_children(eng, oracle):
    k = 700
    names = np.zeros((k + 1, 32), np.uint8)
    v = (k - np.arange(k)).astype(">u8")  # descending in entry order
    names[:k, :8] = v.view(np.uint8).reshape(k, 8)
    # the files first, their directory last
    check(eng, oracle, Case(np.r_[np.full(k, k), -1], np.r_[np.zeros(k, np.uint8), 1].astype(np.uint8),
                            names=names))
    parent, is_dir = R.random_tree(3000, 11)
    check(eng, oracle, Case(parent, is_dir, seed=12))


# ---- the tie fix-up ----------------------------------------------------------------------

def _prefixed(n, rng):
    names = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    names[:, :8] = np.frombuffer(b"\x40prefix\x01", np.uint8)
    return names


def test_ties_on_the_first_eight_bytes(eng, oracle):
    rng = np.random.default_rng(21)
    # three siblings: differ at byte 8, at byte 31, in several bytes — listed in descending order
    names = np.zeros((7, 32), np.uint8)
    names[:, :8] = 7
    names[1, 8], names[2, 8] = 9, 3
    names[3, 31], names[4, 31] = 200, 100
    names[5, 8:] = 0xF0
    names[6, 8:] = 0x0F
    c = Case([-1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0], names=names)
    check(eng, oracle, c)
    assert R.child_order(c.parent, names)[0][0] == [4, 3, 2, 1, 6, 5]
    # a run of 65 among other children
    names = rng.integers(0, 256, (1 + 200, 32), dtype=np.uint8)
    names[50:115] = _prefixed(65, rng)
    check(eng, oracle, Case(np.r_[-1, np.zeros(200, np.int64)], np.r_[1, np.zeros(200, np.uint8)].astype(np.uint8),
                            names=names))


def test_long_tie_runs_take_the_full_sort(eng, oracle):
    """runs above the fix-up's cap of 64: 65 (above), 64 (below, beside it
    under another directory), and 5000 siblings over two tiles with identical
    names among them; then a call without ties on the same workspace"""
    rng = np.random.default_rng(23)
    k = 9000
    names = rng.integers(0, 256, (3 + k, 32), dtype=np.uint8)
    parent = np.r_[-1, -1, -1, np.zeros(k, np.int64)]
    names[1000:6000] = _prefixed(5000, rng)
    names[2000:2010] = names[1999]  # identical: index order
    names[3000:3020, 8:] = 0
    names[3000:3020, 31] = np.arange(20)[::-1]  # differ in the last byte alone, descending
    parent[6100:6165], parent[6200:6264] = 1, 2
    names[6100:6165], names[6200:6264] = _prefixed(65, rng), _prefixed(64, rng)
    is_dir = np.r_[1, 1, 1, np.zeros(k, np.uint8)].astype(np.uint8)
    check(eng, oracle, Case(parent, is_dir, names=names))
    check(eng, oracle, flat(300, seed=24))


def test_a_tie_run_across_a_tile_boundary(eng, oracle):
    """one directory of 2 * TILE children: 4076 names below the run's prefix
    80 00 .., the run of 40, the rest above it"""
    rng = np.random.default_rng(22)
    k = 2 * TILE
    names = rng.integers(0, 256, (1 + k, 32), dtype=np.uint8)
    run = np.arange(1 + k - 40, 1 + k)
    others = rng.permutation(np.arange(1, 1 + k - 40))
    names[others[:4076], 0] &= 0x7F
    names[others[4076:], 0] |= 0x80
    names[others[4076:], 1] |= 1
    names[run, :8] = np.frombuffer(b"\x80\x00\x00\x00\x00\x00\x00\x00", np.uint8)
    c = Case(np.r_[-1, np.zeros(k, np.int64)], np.r_[1, np.zeros(k, np.uint8)].astype(np.uint8), names=names)
    order = R.child_order(c.parent, names)[0][0]
    at = sorted(order.index(int(r)) for r in run)
    # the directory itself is sorted first: child position p is sorted position p + 1
    assert at == list(range(4076, 4116)) and at[0] + 1 < TILE < at[-1] + 1
    check(eng, oracle, c)


def test_identical_names_and_one_prefix_under_two_parents(eng, oracle):
    names = np.zeros((8, 32), np.uint8)
    names[:, :8] = 5
    names[2], names[3] = 77, 77  # identical: index order
    names[4, 20], names[5, 20], names[6, 20], names[7, 20] = 4, 3, 2, 1
    c = Case([-1, -1, 0, 0, 0, 1, 0, 1], [1, 1, 0, 0, 0, 0, 0, 0], names=names)
    check(eng, oracle, c)
    kids = R.child_order(c.parent, names)[0]
    assert kids[0] == [6, 4, 2, 3] and kids[1] == [7, 5]


# ---- depth ---------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [300, 4096])
def test_chains(eng, oracle, depth):
    c = chain(depth - 1) if depth == 4096 else chain(depth)  # 4096 levels with the file
    want = check(eng, oracle, c)
    assert want["counts"]["levels"] == (4096 if depth == 4096 else 301)


def test_a_chain_of_4096_directories(eng, oracle):
    parent, is_dir = np.arange(-1, 4095, dtype=np.int64), np.ones(4096, np.uint8)
    c = Case(parent, is_dir)
    want = check(eng, oracle, c)
    assert want["counts"] == {"entries": 4096, "dirs": 4096, "complete_dirs": 4096, "empty_dirs": 4096,
                              "levels": 4096, "largest_dir": 1}
    with pytest.raises(N.SdcasError) as e:
        eng.dev_tree_digests(np.arange(-1, 4096, dtype=np.int64), np.ones(4097, np.uint8), 16, 0, 4097, 0, 16)
    assert e.value.code == N.SDCAS_E_CAPACITY


def test_twelve_levels_fifty_thousand_entries(eng, oracle):
    parent, is_dir = R.random_tree(50000, 5, max_depth=12)
    rng = np.random.default_rng(6)
    c = Case(parent, is_dir, seed=6, valid=(rng.random(50000) > 0.002).astype(np.uint8))
    want = check(eng, oracle, c)
    assert want["counts"]["levels"] == 12
    assert 0 < want["counts"]["complete_dirs"] < want["counts"]["dirs"]


# ---- completeness and rollups ----------------------------------------------------------------

def test_one_invalid_file_at_depth_five(eng, oracle):
    # a chain 0..4 with the file 5 at depth 5; every directory of the chain has a sibling subtree
    parent = [-1, 0, 1, 2, 3, 4]
    is_dir = [1, 1, 1, 1, 1, 0]
    for d in range(5):  # sibling directory with two files under chain directory d
        s = len(parent)
        parent += [d, s, s]
        is_dir += [1, 0, 0]
    valid = np.ones(len(parent), np.uint8)
    valid[5] = 0
    c = Case(parent, is_dir, valid=valid)
    want = check(eng, oracle, c)
    inc = np.flatnonzero(want["flags"] & R.INCOMPLETE)
    assert inc.tolist() == [0, 1, 2, 3, 4]
    assert not want["digests"][inc].any() and not want["keys"][inc].any() and not want["valid"][inc].any()
    sib = [i for i in range(6, len(parent)) if is_dir[i]]
    assert (want["flags"][sib] == R.DIR).all() and want["valid"][sib].all()
    # the same tree with a NULL valid: every file takes part
    c2 = Case(parent, is_dir, valid=None)
    want2 = check(eng, oracle, c2)
    assert not (want2["flags"] & R.INCOMPLETE).any()


def test_empty_directories_in_empty_directories(eng, oracle):
    #   0/ { 1/ { 2/ {} , 3/ {} }, 4 (file) }
    want = check(eng, oracle, Case([-1, 0, 1, 1, 0], [1, 1, 1, 1, 0]))
    assert want["flags"].tolist() == [R.DIR, R.DIR | R.EMPTY, R.DIR | R.EMPTY, R.DIR | R.EMPTY, 0]
    assert want["valid"].tolist() == [1, 0, 0, 0, 1] and want["digests"][1].any()
    assert (want["digests"][2] == want["digests"][3]).all()
    assert want["counts"]["empty_dirs"] == 3 and want["counts"]["complete_dirs"] == 4


def test_sizes_null_large_and_wrapping(eng, oracle):
    parent, is_dir = [-1, 0, 0, 0, 1, 1], [1, 1, 0, 0, 0, 0]
    want = check(eng, oracle, Case(parent, is_dir, sizes=None))
    assert not want["tree_bytes"].any() and want["tree_files"].tolist() == [4, 2, 1, 1, 1, 1]
    big = np.array([0, 0, (1 << 40) + 5, 1 << 63, (1 << 63) + 9, (1 << 33) + 1], np.uint64)
    want = check(eng, oracle, Case(parent, is_dir, sizes=big))
    assert int(want["tree_bytes"][1]) == ((1 << 63) + 9 + (1 << 33) + 1)
    assert int(want["tree_bytes"][0]) == ((1 << 40) + 5 + 9 + (1 << 33) + 1)  # wrapped past 2^64
    # 200 files of 2^63 under one directory: the wave's pre-combined sum wraps too
    halves = np.full(201, (1 << 63) + 1, np.uint64)
    want = check(eng, oracle, flat(200, sizes=halves))
    assert int(want["tree_bytes"][0]) == 200


# ---- equal trees, equal digests ----------------------------------------------------------------

def _two_copies(m, seed):
    """A/ and B/ hold the same m-entry subtree, B's entries in another index
    order -> (Case, index of A, index of B, map from A's entries to B's)"""
    sp, sd = R.random_tree(m, seed)
    rng = np.random.default_rng(seed + 1)
    perm = rng.permutation(m)  # where B's copy of subtree entry i stands
    n = 2 + 2 * m
    parent = np.zeros(n, np.int64)
    is_dir = np.zeros(n, np.uint8)
    parent[0], parent[1], is_dir[0], is_dir[1] = -1, -1, 1, 1
    a = 2 + np.arange(m)
    b = 2 + m + perm
    parent[a] = np.where(sp >= 0, 2 + np.maximum(sp, 0), 0)
    parent[b] = np.where(sp >= 0, 2 + m + perm[np.maximum(sp, 0)], 1)
    is_dir[a], is_dir[b] = sd, sd
    c = Case(parent, is_dir, seed=seed + 2)
    for arr in (c.names, c.digests, c.sizes):
        arr[b] = arr[a]
    return c, a, b


def test_two_copies_in_different_index_order(eng, oracle):
    c, a, b = _two_copies(2000, 31)
    want = check(eng, oracle, c)
    d = c.is_dir[a] != 0
    assert (want["digests"][a[d]] == want["digests"][b[d]]).all() and (want["keys"][0] == want["keys"][1])
    assert (want["tree_bytes"][a] == want["tree_bytes"][b]).all()


@pytest.mark.parametrize("change", ["name", "digest", "kind"])
def test_a_changed_copy_gets_another_digest(eng, oracle, change):
    #   0 A/ { 2 x, 3 e/ }     1 B/ { 4 x, 5 e (a directory, or a file holding T(e)) }
    t_e = np.frombuffer(bytes.fromhex(oracle.hash(b"SDTREE01" + bytes(8))), np.uint8)
    is_dir = [1, 1, 0, 1, 0, 0 if change == "kind" else 1]
    c = Case([-1, -1, 0, 0, 1, 1], is_dir)
    c.names[4], c.names[5], c.digests[4] = c.names[2], c.names[3], c.digests[2]
    if change == "name":
        c.names[4, 31] ^= 1
    elif change == "digest":
        c.digests[4, 0] ^= 0x80
    else:
        c.digests[5], c.valid[5] = t_e, 1  # the same name and content bytes, the other kind
    want = check(eng, oracle, c)
    assert (want["digests"][3] == t_e).all()
    assert (want["digests"][0] != want["digests"][1]).any() and want["keys"][0] != want["keys"][1]


# ---- the contract --------------------------------------------------------------------------------

def test_each_output_null_in_turn(eng, oracle):
    parent, is_dir = R.random_tree(5000, 41)
    c = Case(parent, is_dir, seed=42)
    want = c.want(oracle)
    for skip in ("keys", "valid", "tree_bytes", "tree_files", "flags", "counts"):
        outputs = tuple(k for k in OUTS if k != skip)
        compare(f"without {skip}", device_call(eng, c, outputs), want, c, outputs)
    compare("only digests", device_call(eng, c, ("digests",)), want, c, ("digests",))


def test_each_output_null_in_turn_through_the_host_call(eng, oracle):
    import ctypes
    parent, is_dir = R.random_tree(1500, 48)
    c = Case(parent, is_dir, seed=49)
    want = c.want(oracle)
    n = c.n
    for skip in ("keys", "valid", "tree_bytes", "tree_files", "flags", "counts", None):
        outputs = tuple(k for k in OUTS if k != skip)
        a = {"keys": c.keys.copy(), "digests": c.digests.copy(), "valid": c.valid.copy(),
             "tree_bytes": np.full(n, P64, np.uint64), "tree_files": np.full(n, P64, np.uint64),
             "flags": np.full(n, P8, np.uint8)}
        counts = N.TreeCounts(*([P64] * 6))
        p = lambda k: a[k].ctypes.data if k in outputs else None
        rc = eng.L.sdcas_tree_digests(eng.ctx, c.parent.ctypes.data, c.is_dir.ctypes.data, c.names.ctypes.data,
                                      c.sizes.ctypes.data, n, p("keys"), a["digests"].ctypes.data, p("valid"),
                                      p("tree_bytes"), p("tree_files"), p("flags"),
                                      ctypes.byref(counts) if "counts" in outputs else None)
        assert rc == N.SDCAS_OK
        a["counts"] = counts.as_dict()
        # (a NULL valid also means that every file takes part: the same here, where all are valid)
        compare(f"host without {skip}", a, want, c, outputs)


def test_guarded_buffers_of_exactly_the_stated_sizes(eng, oracle):
    parent, is_dir = R.random_tree(4099, 43)
    c = Case(parent, is_dir, seed=44)
    n = c.n
    want = c.want(oracle)
    g = {"names": guarded_from(c.names, align=16), "digests": guarded_from(c.digests, align=16, snapshot=False),
         "keys": guarded_from(c.keys, align=8, snapshot=False), "valid": guarded_from(c.valid, align=1, snapshot=False),
         "sizes": guarded_from(c.sizes, align=8), "tree_bytes": Guarded(8 * n, align=8),
         "tree_files": Guarded(8 * n, align=8), "flags": Guarded(n, align=1), "counts": Guarded(48, align=8)}
    for again in range(2):
        eng.dev_tree_digests(c.parent, c.is_dir, g["names"].ptr, g["sizes"].ptr, n, g["keys"].ptr, g["digests"].ptr,
                             g["valid"].ptr, g["tree_bytes"].ptr, g["tree_files"].ptr, g["flags"].ptr,
                             g["counts"].ptr)
        eng.dev_sync()
        for k, b in g.items():
            assert b.check() == [], f"call {again}: bytes around {k} were written"
        assert g["names"].unchanged() and g["sizes"].unchanged()
        got = {"keys": g["keys"].download(np.uint64), "digests": g["digests"].download().reshape(n, 32),
               "valid": g["valid"].download(), "tree_bytes": g["tree_bytes"].download(np.uint64),
               "tree_files": g["tree_files"].download(np.uint64), "flags": g["flags"].download(),
               "counts": dict(zip(R.TREE_COUNTS, (int(x) for x in g["counts"].download(np.uint64))))}
        compare(f"guarded call {again}", got, want, c)


def test_misaligned_arrays_are_refused_before_anything_runs(eng):
    c = flat(20)
    names, dig = _t(np.r_[c.names.reshape(-1), np.zeros(16, np.uint8)]), _t(np.r_[c.digests.reshape(-1), np.zeros(16, np.uint8)])
    out = _t(np.full(c.n, P64, np.uint64))
    torch.cuda.synchronize()
    for np_, dp in ((names.data_ptr() + 8, dig.data_ptr()), (names.data_ptr(), dig.data_ptr() + 8),
                    (names.data_ptr() + 1, dig.data_ptr())):
        with pytest.raises(N.SdcasError) as e:
            eng.dev_tree_digests(c.parent, c.is_dir, np_, 0, c.n, 0, dp, 0, out.data_ptr())
        assert e.value.code == N.SDCAS_E_INVALID
    with pytest.raises(N.SdcasError) as e:
        eng.dev_tree_digests(c.parent, c.is_dir, names.data_ptr(), 0, c.n, 0, dig.data_ptr(), 0, out.data_ptr() + 4)
    assert e.value.code == N.SDCAS_E_INVALID
    with pytest.raises(N.SdcasError) as e:  # a shape error, with every pointer in order
        eng.dev_tree_digests(np.full(c.n, 3, np.int64), c.is_dir, names.data_ptr(), 0, c.n, 0, dig.data_ptr(), 0,
                             out.data_ptr())
    assert e.value.code == N.SDCAS_E_INVALID
    eng.dev_sync()
    assert (out.cpu().numpy().view(np.uint64) == P64).all()
    assert (dig.cpu().numpy()[:32 * c.n] == c.digests.reshape(-1)).all()


def test_a_small_call_after_a_large_one(eng, oracle):
    parent, is_dir = R.random_tree(30000, 45)
    check(eng, oracle, Case(parent, is_dir, seed=46))
    check(eng, oracle, Case([-1, 0, 0, 1], [1, 1, 0, 0], seed=47))


# ---- tree_top ----------------------------------------------------------------------------------------

def top_device(eng, parent, rep, outputs=(True, True, True), stream=0):
    parent, rep = np.ascontiguousarray(parent, np.int64), np.ascontiguousarray(rep, np.int64)
    n = rep.size
    dp, dr = _t(parent), _t(rep)
    top, fl, cts = _t(np.full(n, P64, np.uint64)), _t(np.full(n, P8, np.uint8)), _t(np.full(6, P64, np.uint64))
    torch.cuda.synchronize()
    eng.dev_tree_top(dp.data_ptr() if n else 0, dr.data_ptr() if n else 0, n,
                     top.data_ptr() if outputs[0] and n else 0, fl.data_ptr() if outputs[1] and n else 0,
                     cts.data_ptr() if outputs[2] else 0, stream)
    eng.dev_sync(stream)
    torch.cuda.synchronize()
    return (top.cpu().numpy().view(np.int64)[:n], fl.cpu().numpy()[:n],
            dict(zip(R.TOP_COUNTS, (int(x) for x in cts.cpu().numpy().view(np.uint64)))))


def check_top(eng, parent, rep, host=True):
    want = R.tree_top(parent, rep, stray_parent_is_root=True)
    calls = [("device", lambda: top_device(eng, parent, rep))]
    if host:
        calls.append(("host", lambda: eng.tree_top(parent, rep)))
    for how, call in calls:
        for again in range(2):
            got = call()
            assert (got[0] == want[0]).all(), f"{how} {again} top_rep: first at {np.flatnonzero(got[0] != want[0])[:5]}"
            assert (got[1] == want[1]).all(), f"{how} {again} flags: first at {np.flatnonzero(got[1] != want[1])[:5]}"
            assert got[2] == want[2], f"{how} {again} counts: {got[2]} != {want[2]}"
    return want


def test_top_smallest_and_hand_made(eng):
    assert top_device(eng, [], [])[2] == dict.fromkeys(R.TOP_COUNTS, 0)
    assert eng.tree_top([], [])[2] == dict.fromkeys(R.TOP_COUNTS, 0)
    want = check_top(eng, [-1, 0, 0, -1, 3, 0], [0, 1, 1, 0, -1, 5])
    assert want[0].tolist() == [0, -1, -1, 0, -1, -1]
    check_top(eng, [-1], [0])
    check_top(eng, [-1, -1], [0, 0])


def test_top_a_stray_member_keeps_its_class_whole(eng):
    #   0 A/ { 2 c/ { 4 p, 5 q } }   1 B/ { 3 c/ { 6 p, 7 q } }   8 X/ { 9 p, 10 q }  with X equal to A/c
    parent = [-1, -1, 0, 1, 2, 2, 3, 3, -1, 8, 8]
    rep = [0, 0, 2, 2, 4, 5, 4, 5, 2, 4, 5]
    want = check_top(eng, parent, rep)
    assert want[0].tolist() == [0, 0, 2, 2, -1, -1, -1, -1, 2, -1, -1]
    assert want[2]["kept_classes"] == 2 and want[2]["dropped_classes"] == 2


def test_top_a_clone_nested_in_a_clone(eng):
    #   0 A/ { 1 s/ { 2 f }, 3 t/ { 4 f } }  5 B/ { 6 s/ { 7 f }, 8 t/ { 9 f } }: s equals t, A equals B
    parent = [-1, 0, 1, 0, 3, -1, 5, 6, 5, 8]
    rep = [0, 1, 2, 1, 2, 0, 1, 2, 1, 2]
    want = check_top(eng, parent, rep)
    assert want[0].tolist() == [0, -1, -1, -1, -1, 0, -1, -1, -1, -1]
    assert want[2] == {"entries": 10, "dup_entries": 10, "nested_entries": 8, "top_entries": 2, "kept_classes": 1,
                       "dropped_classes": 2}


def test_top_stray_labels_and_parents(eng):
    n = 3000
    rng = np.random.default_rng(51)
    parent, _ = R.random_tree(n, 52, dir_share=0.5)
    rep = rng.integers(0, 400, n).astype(np.int64)
    rep[::3] = -1
    rep[[1, 10, 100, 1000, 2000]] = [-7, n, 1 << 40, np.iinfo(np.int64).max, np.iinfo(np.int64).min]
    check_top(eng, parent, rep)
    stray = parent.copy()
    stray[[5, 50, 500, 2500]] = [n, -9, 1 << 40, np.iinfo(np.int64).min]
    check_top(eng, stray, rep, host=False)
    with pytest.raises(N.SdcasError) as e:
        eng.tree_top(stray, rep)
    assert e.value.code == N.SDCAS_E_INVALID


@pytest.mark.parametrize("n", [63, 64, 65, TILE - 1, TILE, TILE + 1, 100000])
def test_top_one_class(eng, n):
    want = check_top(eng, np.full(n, -1, np.int64), np.full(n, n - 1, np.int64))
    assert want[2] == {"entries": n, "dup_entries": n, "nested_entries": 0, "top_entries": n, "kept_classes": 1,
                       "dropped_classes": 0}
    # the same class inside one duplicate directory pair: all nested, dropped
    parent = np.r_[-1, -1, np.arange(n) % 2]
    rep = np.r_[0, 0, np.full(n, 5)]
    want = check_top(eng, parent, rep)
    assert want[2]["dropped_classes"] == 1 and want[2]["top_entries"] == 2


def test_top_no_duplicates_and_null_outputs(eng):
    n = 5000
    parent, _ = R.random_tree(n, 53)
    want = check_top(eng, parent, np.arange(n))
    assert want[2]["dup_entries"] == 0 and (want[0] == -1).all()
    rep = np.random.default_rng(54).integers(0, 900, n)
    full = R.tree_top(parent, rep)
    for j in range(3):
        outputs = [k != j for k in range(3)]
        got = top_device(eng, parent, rep, outputs)
        assert (got[0] == full[0]).all() if outputs[0] else (got[0].view(np.uint64) == P64).all()
        assert (got[1] == full[1]).all() if outputs[1] else (got[1] == P8).all()
        assert got[2] == full[2] if outputs[2] else set(got[2].values()) == {P64}


# ---- the four calls on one stream ------------------------------------------------------------------------

def test_the_chain_on_another_stream_without_synchronisation(eng, oracle):
    c, a, b = _two_copies(1500, 61)
    n = c.n
    # the file entries keyed by their digests' first 8 bytes, as identify_duplicate_trees does
    f = c.is_dir == 0
    c.keys[f] = c.digests[f, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
    want = c.want(oracle)
    rep_h = eng.confirm_duplicates(want["keys"], want["digests"], want["valid"])[0]
    top_h = R.tree_top(c.parent, rep_h)
    sets_h = eng.duplicate_sets(top_h[0], want["tree_bytes"], N.SDCAS_SETS_BY_RECLAIMABLE)
    s = torch.cuda.Stream()
    t = {k: _t(v) for k, v in (("names", c.names), ("digests", c.digests), ("keys", c.keys), ("valid", c.valid),
                               ("sizes", c.sizes), ("parent", c.parent))}
    i64 = lambda m: torch.full((max(m, 1),), -3, dtype=torch.int64, device="cuda")
    tb, rep, top, set_rep, set_off, set_bytes, members, cts = i64(n), i64(n), i64(n), i64(n // 2), \
        i64(n // 2 + 1), i64(n // 2), i64(n), i64(18)
    torch.cuda.synchronize()
    st = s.cuda_stream
    eng.dev_tree_digests(c.parent, c.is_dir, t["names"].data_ptr(), t["sizes"].data_ptr(), n, t["keys"].data_ptr(),
                         t["digests"].data_ptr(), t["valid"].data_ptr(), tb.data_ptr(), 0, 0, cts.data_ptr(), st)
    eng.dev_confirm_duplicates(t["keys"].data_ptr(), t["digests"].data_ptr(), t["valid"].data_ptr(), n,
                               rep.data_ptr(), 0, 0, 0, st)
    eng.dev_tree_top(t["parent"].data_ptr(), rep.data_ptr(), n, top.data_ptr(), 0, cts.data_ptr() + 48, st)
    eng.dev_duplicate_sets(top.data_ptr(), tb.data_ptr(), n, set_rep.data_ptr(), set_off.data_ptr(),
                           set_bytes.data_ptr(), members.data_ptr(), cts.data_ptr() + 96,
                           N.SDCAS_SETS_BY_RECLAIMABLE, st)
    s.synchronize()
    assert (rep.cpu().numpy() == rep_h).all() and (top.cpu().numpy() == top_h[0]).all()
    counts = cts.cpu().numpy().view(np.uint64)
    assert dict(zip(R.TREE_COUNTS, map(int, counts[:6]))) == want["counts"]
    assert dict(zip(R.TOP_COUNTS, map(int, counts[6:12]))) == top_h[2]
    ns, nm = int(sets_h[4]["sets"]), int(sets_h[4]["members"])
    assert int(counts[13]) == ns and int(counts[14]) == nm
    assert (set_rep.cpu().numpy()[:ns] == sets_h[0]).all() and (members.cpu().numpy()[:nm] == sets_h[3]).all()
    # A and B are the first set: the most reclaimable
    assert sets_h[3][:2].tolist() == [0, 1] and int(sets_h[2][0]) == int(want["tree_bytes"][0])


# ---- the C++ mirror ------------------------------------------------------------------------------------------

def test_tree_report_on_both_libraries(oracle, tmp_path):
    """tests/cpp/test_dirtree.cpp --gpu: the identifier job with checksums over
    real files, then tree_report on a MemoryLibrary and a SqliteLibrary (the
    program checks that the two agree and that nothing is written); the sets it
    prints are the checker's for that directory"""
    import subprocess
    from tests.test_gpu_dupsets import group_sets
    root = tmp_path / "loc"
    (root / "photos" / "2019" / "trip").mkdir(parents=True)
    rng = np.random.default_rng(81)
    for rel, size in (("photos/2019/a.jpg", 5000), ("photos/2019/b.jpg", 150000), ("photos/2019/trip/c.jpg", 70),
                      ("photos/2019/trip/README", 9), ("photos/note.txt", 33), ("single.bin", 2000)):
        (root / rel).write_bytes(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
    shutil.copytree(root / "photos" / "2019", root / "backup")
    shutil.copytree(root / "photos" / "2019", root / "almost")
    data = bytearray((root / "almost" / "b.jpg").read_bytes())
    data[77777] ^= 1
    (root / "almost" / "b.jpg").write_bytes(bytes(data))
    shutil.copy(root / "single.bin", root / "photos" / "single-copy.bin")
    (root / "hollow" / "inner").mkdir(parents=True)
    os.symlink(root / "photos", root / "link")

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "cpp", "build",
                        "test_dirtree")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.dirname(os.path.dirname(path)), "-f", "dirtree.mk"], check=True)
    r = subprocess.run([path, "--gpu", str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr

    # the checker over the same directory
    rel, is_dir, parent = [], [], []
    stack = [("", -1)]
    while stack:
        prefix, at = stack.pop()
        for name in sorted(os.listdir(root / prefix)):
            p = os.path.join(prefix, name)
            if os.path.islink(root / p):
                continue
            rel.append(p), is_dir.append(int(os.path.isdir(root / p))), parent.append(at)
            if is_dir[-1]:
                stack.append((p, len(rel) - 1))
    n = len(rel)
    names = np.stack([np.frombuffer(bytes.fromhex(oracle.hash(os.fsencode(os.path.basename(p)))), np.uint8)
                      for p in rel])
    dig = np.zeros((n, 32), np.uint8)
    sizes = np.zeros(n, np.uint64)
    for i, p in enumerate(rel):
        if not is_dir[i]:
            dig[i] = np.frombuffer(bytes.fromhex(oracle.file_checksum(str(root / p))), np.uint8)
            sizes[i] = os.path.getsize(root / p)
    f = np.array(is_dir) == 0
    keys = np.zeros(n, np.uint64)
    keys[f] = dig[f, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
    want = R.tree_digests(oracle, parent, is_dir, names, dig, f.astype(np.uint8), sizes, keys)
    first, rep = {}, np.full(n, -1, np.int64)
    for i in range(n):
        if want["valid"][i]:
            rep[i] = first.setdefault((int(want["keys"][i]), want["digests"][i].tobytes()), i)
    top, _, top_counts = R.tree_top(parent, rep)
    set_rep, offs, set_bytes, members, counts = group_sets(top, want["tree_bytes"], N.SDCAS_SETS_BY_RECLAIMABLE)
    expect = []
    for s in range(len(set_rep)):
        m = members[int(offs[s]):int(offs[s + 1])]
        one = int(set_bytes[s])
        expect.append((-(len(m) - 1) * one, sorted(rel[i] for i in m), "d" if is_dir[set_rep[s]] else "f", one,
                       int(want["tree_files"][set_rep[s]])))
    got = []
    for line in r.stdout.splitlines():
        if line.startswith("set "):
            _, kind, tb, tf, recl, paths = line.split(" ", 5)
            got.append((-int(recl), sorted(paths.split("|")), kind, int(tb), int(tf)))
        elif line.startswith("counts "):
            assert [int(x) for x in line.split()[1:]] == [want["counts"]["dirs"], top_counts["dropped_classes"],
                                                          counts["sets"]]
    assert [g[0] for g in got] == sorted(g[0] for g in got), "most reclaimable first"
    assert sorted(got) == sorted(expect)
    assert got[0][1] == ["backup", os.path.join("photos", "2019")] and got[0][2] == "d" and got[0][4] == 4
    assert sorted(["single.bin", os.path.join("photos", "single-copy.bin")]) in [g[1] for g in got]


# ---- real files ----------------------------------------------------------------------------------------------

def test_real_files(eng, oracle, tmp_path):
    root = tmp_path / "lib"
    (root / "photos" / "2019" / "trip").mkdir(parents=True)
    rng = np.random.default_rng(71)
    for rel, size in (("photos/2019/a.jpg", 5000), ("photos/2019/b.jpg", 150000), ("photos/2019/trip/c.jpg", 70),
                      ("photos/2019/trip/empty.txt", 0), ("photos/note.txt", 33)):
        (root / rel).write_bytes(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
    shutil.copytree(root / "photos" / "2019", root / "backup")  # a complete copy
    shutil.copytree(root / "photos" / "2019", root / "almost")  # one byte changed
    data = bytearray((root / "almost" / "b.jpg").read_bytes())
    data[77777] ^= 1
    (root / "almost" / "b.jpg").write_bytes(bytes(data))
    (root / "hollow" / "inner").mkdir(parents=True)  # empty directories
    os.symlink(root / "photos", root / "link")  # skipped, not followed
    locked = root / "photos" / "locked.bin"
    locked.write_bytes(b"secret")
    os.chmod(locked, 0)
    unreadable = not os.access(locked, os.R_OK)
    try:
        r = eng.identify_duplicate_trees(str(root))
    finally:
        os.chmod(locked, stat.S_IRUSR | stat.S_IWUSR)
    rel = [p for p, _ in r["entries"]]
    n = len(rel)
    assert "link" not in rel and not any(p.startswith("link" + os.sep) for p in rel)
    # photos, backup, almost, hollow; photos/2019, note, locked; 3 x (a, b, trip, c, empty); hollow/inner
    assert n == 4 + 3 + 3 * 5 + 1
    at = {p: i for i, p in enumerate(rel)}
    for i, p in enumerate(rel):
        assert r["parent"][i] == (at[os.path.dirname(p)] if os.path.dirname(p) else -1)
        assert bool(r["is_dir"][i]) == os.path.isdir(root / p)
    # the checker, fed with the oracle's checksums
    names = np.stack([np.frombuffer(bytes.fromhex(oracle.hash(os.fsencode(os.path.basename(p)))), np.uint8)
                      for p in rel])
    dig = np.zeros((n, 32), np.uint8)
    valid = np.zeros(n, np.uint8)
    sizes = np.zeros(n, np.uint64)
    for i, p in enumerate(rel):
        if r["is_dir"][i]:
            continue
        sizes[i] = os.path.getsize(root / p)
        if p == os.path.join("photos", "locked.bin") and unreadable:
            sizes[i] = r["sizes"][i]
            continue
        dig[i] = np.frombuffer(bytes.fromhex(oracle.file_checksum(str(root / p))), np.uint8)
        valid[i] = 1
    f = r["is_dir"] == 0
    assert (r["name32"] == names).all() and (r["valid"][f] == valid[f]).all()
    assert (r["digests"][f & (valid == 1)] == dig[f & (valid == 1)]).all()
    keys = np.zeros(n, np.uint64)
    keys[f] = r["digests"][f, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
    dig[f] = r["digests"][f]
    want = R.tree_digests(oracle, r["parent"], r["is_dir"], names, dig, valid, sizes, keys)
    for k, g in (("keys", "keys"), ("digests", "digests"), ("valid", "valid"), ("tree_bytes", "tree_bytes"),
                 ("tree_files", "tree_files"), ("flags", "tree_flags")):
        assert (r[g] == want[k]).all(), k
    assert r["tree_counts"] == want["counts"]
    top = R.tree_top(r["parent"], r["rep"])
    assert (r["top_rep"] == top[0]).all() and (r["top_flags"] == top[1]).all() and r["top_counts"] == top[2]
    # photos/2019 and backup are one set, reported once: nothing below them is
    pair = sorted((at[os.path.join("photos", "2019")], at["backup"]))
    sets = [r["members"][int(r["set_offsets"][s]):int(r["set_offsets"][s + 1])].tolist()
            for s in range(len(r["set_rep"]))]
    assert sets[0] == pair and int(r["set_bytes"][0]) == 5000 + 150000 + 70
    # below the pair: b.jpg (changed in almost/) and what lies in trip/ (a duplicate in almost/ too) are
    # implied and dropped; a.jpg and trip/ have a carrier outside any duplicate directory (almost/'s), so
    # their classes are kept whole
    for name, kept in (("b.jpg", False), (os.path.join("trip", "c.jpg"), False),
                       (os.path.join("trip", "empty.txt"), False), ("a.jpg", True), ("trip", True)):
        for top in ("backup", os.path.join("photos", "2019")):
            i = at[os.path.join(top, name)]
            assert (r["top_rep"][i] != -1) == kept and r["top_flags"][i] == R.DUP | R.NESTED, (top, name)
    # the near-copy is no duplicate directory, but its unchanged files and its trip/ are duplicates still
    assert r["top_rep"][at["almost"]] == -1
    assert r["top_rep"][at[os.path.join("almost", "trip")]] == r["rep"][at[os.path.join("photos", "2019", "trip")]]
    assert r["tree_flags"][at["hollow"]] == R.DIR | R.EMPTY and r["top_rep"][at["hollow"]] == -1
    if unreadable:
        assert r["tree_flags"][at["photos"]] == R.DIR | R.INCOMPLETE and r["valid"][at["photos"]] == 0
