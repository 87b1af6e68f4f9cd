"""GPU tests of the duplicates confirmed by checksum (csrc/confirm.hip;
sdcas_confirm_duplicates, sdcas_dev_confirm_duplicates,
Engine.identify_confirmed): the group-by over (cas key, 32-byte digest).

The checker is the dict-based group-by below — first index per (key, digest),
digest set per key — never the code under test. Every output array and all
six counts are compared for equality, through the host call and through the
device call with torch tensors."""
import os

import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests._oracle import cas_windows, content_key, mix64

pytestmark = pytest.mark.gpu

DUP, COL, SKIP = N.SDCAS_CONFIRM_DUPLICATE, N.SDCAS_CONFIRM_COLLISION, N.SDCAS_CONFIRM_SKIPPED
COUNTS = ("files", "classes", "keys", "collided_keys", "collided_files", "duplicate_files")


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


# ---- the checker ---------------------------------------------------------------

def group_by(keys, digests, valid=None):
    keys = np.asarray(keys, np.uint64)
    n = keys.size
    digests = np.asarray(digests, np.uint8).reshape(n, 32)
    first, key_first, sums = {}, {}, {}
    cls = [None] * n
    for i in range(n):
        if valid is not None and not valid[i]:
            continue
        k = int(keys[i])
        d = digests[i].tobytes()
        cls[i] = (k, d)
        first.setdefault((k, d), i)
        key_first.setdefault(k, i)
        sums.setdefault(k, set()).add(d)
    rep = np.full(n, -1, np.int64)
    key_rep = np.full(n, -1, np.int64)
    flags = np.full(n, SKIP, np.uint8)
    for i in range(n):
        if cls[i] is None:
            continue
        rep[i] = first[cls[i]]
        key_rep[i] = key_first[cls[i][0]]
        flags[i] = (DUP if rep[i] != i else 0) | (COL if len(sums[cls[i][0]]) >= 2 else 0)
    files = sum(c is not None for c in cls)
    collided = [k for k, s in sums.items() if len(s) >= 2]
    counts = {"files": files, "classes": len(first), "keys": len(key_first), "collided_keys": len(collided),
              "collided_files": sum(1 for c in cls if c is not None and len(sums[c[0]]) >= 2),
              "duplicate_files": files - len(first)}
    return rep, key_rep, flags, counts


def digests_of(ids):
    """32 bytes per id: four mixed words"""
    ids = np.asarray(ids, np.uint64)
    with np.errstate(over="ignore"):
        w = mix64(ids[:, None] * np.uint64(4) + np.arange(4, dtype=np.uint64)[None, :])
    return np.ascontiguousarray(w).view(np.uint8).reshape(len(ids), 32)


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).cuda()


def device_call(eng, keys, digests, valid=None, outputs=(True, True, True, True)):
    """sdcas_dev_confirm_duplicates over torch tensors; outputs: which of
    rep / key_rep / flags / counts are passed (the others are null and come
    back as None)"""
    keys = np.asarray(keys, np.uint64)
    n = keys.size
    k = _i64(keys) if n else torch.zeros(1, dtype=torch.int64, device="cuda")
    d = torch.from_numpy(np.ascontiguousarray(digests, np.uint8).reshape(-1).copy()).cuda() if n else \
        torch.zeros(32, dtype=torch.uint8, device="cuda")
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8).copy()).cuda()
    rep = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    krep = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    fl = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((6,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.dev_confirm_duplicates(k.data_ptr(), d.data_ptr(), v.data_ptr() if v is not None and n else 0, n,
                               rep.data_ptr() if outputs[0] else 0, krep.data_ptr() if outputs[1] else 0,
                               fl.data_ptr() if outputs[2] else 0, cnt.data_ptr() if outputs[3] else 0)
    eng.dev_sync()
    got = (rep.cpu().numpy()[:n], krep.cpu().numpy()[:n], fl.cpu().numpy()[:n],
           dict(zip(COUNTS, (int(x) for x in cnt.cpu().numpy()))))
    # an output that was not passed stays as it was filled
    untouched = (np.full(n, -7, np.int64), np.full(n, -7, np.int64), np.full(n, 0xEE, np.uint8),
                 dict.fromkeys(COUNTS, -7))
    for j in range(4):
        if not outputs[j]:
            assert _same(got[j], untouched[j]), f"null output {j} was written"
    return tuple(g if outputs[j] else None for j, g in enumerate(got))


def _same(a, b):
    return a == b if isinstance(a, dict) else (a.shape == b.shape and bool((a == b).all()))


def check(eng, keys, digests, valid=None):
    """host call and device call against the checker; returns the checker's answer"""
    want = group_by(keys, digests, valid)
    names = ("rep", "key_rep", "flags", "counts")
    for how, got in (("host", eng.confirm_duplicates(keys, digests, valid)),
                     ("device", device_call(eng, keys, digests, valid))):
        for nm, g, w in zip(names, got, want):
            if isinstance(w, dict):
                assert g == w, f"{how} {nm}: {g} != {w}"
            else:
                assert g.dtype == w.dtype and g.shape == w.shape, f"{how} {nm}: {g.dtype}{g.shape}"
                bad = np.flatnonzero(g != w)
                assert bad.size == 0, f"{how} {nm}: {bad.size} differ, first at {bad[:5]}: {g[bad[:5]]} != {w[bad[:5]]}"
    return want


def shuffled_classes(n, n_keys, seed, max_sums=3):
    """n files over n_keys keys, 1..max_sums digests per key, in seeded random order"""
    rng = np.random.default_rng(seed)
    key_id = rng.integers(0, n_keys, n)
    sum_id = rng.integers(0, 1 + key_id % max_sums)  # key k has 1 + k % max_sums digests
    keys = mix64(key_id.astype(np.uint64) + np.uint64(seed << 20))
    return keys, digests_of(key_id * 8 + sum_id + (seed << 24))


# ---- synthetic cases --------------------------------------------------------------

def test_no_files_and_one_file(eng):
    rep, key_rep, flags, counts = check(eng, np.zeros(0, np.uint64), np.zeros((0, 32), np.uint8))
    assert counts == dict.fromkeys(COUNTS, 0)
    rep, key_rep, flags, counts = check(eng, [5], digests_of([1]))
    assert rep.tolist() == [0] and key_rep.tolist() == [0] and flags.tolist() == [0]
    rep, key_rep, flags, counts = check(eng, [5], digests_of([1]), [0])
    assert rep.tolist() == [-1] and flags.tolist() == [SKIP] and counts["files"] == 0


def test_two_files(eng):
    # an equal pair
    rep, key_rep, flags, counts = check(eng, [9, 9], digests_of([1, 1]))
    assert rep.tolist() == [0, 0] and flags.tolist() == [0, DUP] and counts["duplicate_files"] == 1
    # a colliding pair: one key, two digests
    rep, key_rep, flags, counts = check(eng, [9, 9], digests_of([1, 2]))
    assert rep.tolist() == [0, 1] and key_rep.tolist() == [0, 0] and flags.tolist() == [COL, COL]
    assert counts == {"files": 2, "classes": 2, "keys": 1, "collided_keys": 1, "collided_files": 2,
                      "duplicate_files": 0}
    # different keys with the same digest: two classes, no collision
    rep, key_rep, flags, counts = check(eng, [9, 10], digests_of([1, 1]))
    assert rep.tolist() == [0, 1] and key_rep.tolist() == [0, 1] and flags.tolist() == [0, 0]
    assert counts["classes"] == 2 and counts["collided_keys"] == 0


@pytest.mark.parametrize("n", [63, 64, 65, 257, 1025])
def test_wave_and_workgroup_edges(eng, n):
    keys, digests = shuffled_classes(n, max(2, n // 4), seed=n)
    rep, key_rep, flags, counts = check(eng, keys, digests)
    assert counts["duplicate_files"] > 0 and counts["collided_keys"] > 0


def test_one_class_of_4096(eng):
    """every insert contends on one slot of either table"""
    n = 4096
    rep, key_rep, flags, counts = check(eng, np.full(n, 0xC0FFEE, np.uint64), np.tile(digests_of([7]), (n, 1)))
    assert (rep == 0).all() and (key_rep == 0).all() and flags[0] == 0 and (flags[1:] == DUP).all()
    assert counts == {"files": n, "classes": 1, "keys": 1, "collided_keys": 0, "collided_files": 0,
                      "duplicate_files": n - 1}


@pytest.mark.parametrize("byte", [31, 0])
def test_one_key_digests_differ_in_one_byte(eng, byte):
    """2048 files of ONE key whose digests differ only in one byte (a byte has
    256 values: 256 classes of 8 files): a compare or a hash that covers part
    of the digest merges them or chains every probe"""
    n = 2048
    digests = np.tile(digests_of([3]), (n, 1))
    digests[:, byte] = np.arange(n) % 256
    rep, key_rep, flags, counts = check(eng, np.full(n, 0xABCD, np.uint64), digests)
    assert counts["classes"] == 256 and counts["keys"] == 1 and counts["collided_files"] == n
    assert (rep == np.arange(n) % 256).all() and (key_rep == 0).all()


@pytest.mark.parametrize("first", [30, 0])
def test_one_key_2048_different_digests(eng, first):
    """2048 different digests of ONE key that differ only in two neighbouring
    bytes, the last two or the first two"""
    n = 2048
    digests = np.tile(digests_of([4]), (n, 1))
    digests[:, first] = np.arange(n) >> 8
    digests[:, first + 1] = np.arange(n) & 255
    rep, key_rep, flags, counts = check(eng, np.full(n, 0x1234, np.uint64), digests)
    assert counts["classes"] == n and counts["collided_keys"] == 1 and counts["duplicate_files"] == 0
    assert (rep == np.arange(n)).all() and (flags == COL).all()


def test_lowest_index_rule_with_shuffled_members(eng):
    """20 workgroups; the classes' members land anywhere (seeded), and three
    classes are placed by hand: their copies in the first workgroup and one
    member in the last, in either order"""
    n = 5000
    keys, digests = shuffled_classes(n, 900, seed=11)
    keys, digests = keys.copy(), digests.copy()
    hand = {0x111: [n - 1, 0, 1, 2], 0x222: [3, n - 2, 4], 0x333: [n - 3, n - 4, 5]}
    for k, members in hand.items():
        keys[members] = k
        digests[members] = digests_of([k])[0]
    rep, key_rep, flags, counts = check(eng, keys, digests)
    for k, members in hand.items():
        assert (rep[members] == min(members)).all() and (key_rep[members] == min(members)).all()


def test_valid_mask_skips_lowest_members(eng):
    """every third file skipped, among them files that would have been their
    class's or their key's lowest: a skipped file is nobody's rep or key_rep"""
    n = 3001
    keys, digests = shuffled_classes(n, 400, seed=5)
    valid = (np.arange(n) % 3 != 0).astype(np.uint8)
    all_rep, all_key_rep, _, _ = group_by(keys, digests)
    assert (valid[all_rep] == 0).any() and (valid[all_key_rep] == 0).any()  # the case is in the data
    rep, key_rep, flags, counts = check(eng, keys, digests, valid)
    on = valid != 0
    assert (valid[rep[on]] == 1).all() and (valid[key_rep[on]] == 1).all()
    assert (flags[~on] == SKIP).all() and (rep[~on] == -1).all() and (key_rep[~on] == -1).all()
    assert counts["files"] == int(on.sum())
    # nothing valid at all
    check(eng, keys[:100], digests[:100], np.zeros(100, np.uint8))


@pytest.fixture(scope="module")
def big_case():
    """100 003 files over 30 000 keys, 1-3 digests per key, 1-5 copies per class"""
    rng = np.random.default_rng(2024)
    n, n_keys = 100003, 30000
    class_key = np.repeat(np.arange(n_keys), 1 + np.arange(n_keys) % 3)  # key k has 1 + k % 3 digests
    class_sum = np.concatenate([np.arange(1 + k % 3) for k in range(n_keys)])
    copies = rng.choice([1, 2, 3, 4, 5], class_key.size, p=[0.6, 0.22, 0.1, 0.05, 0.03])
    # trim or pad the copies, class by class, to exactly n files
    c = 0
    while copies.sum() != n:
        if copies.sum() > n and copies[c] > 1:
            copies[c] -= 1
        elif copies.sum() < n and copies[c] < 5:
            copies[c] += 1
        c = (c + 1) % copies.size
    assert copies.min() == 1 and copies.max() == 5
    key_ids = np.repeat(class_key, copies).astype(np.uint64)
    sum_ids = np.repeat(class_sum, copies).astype(np.uint64)
    order = rng.permutation(n)
    key_ids, sum_ids = key_ids[order], sum_ids[order]
    return mix64(key_ids + np.uint64(77 << 32)), digests_of(key_ids * np.uint64(4) + sum_ids + np.uint64(1 << 40))


def test_many_workgroups(eng, big_case):
    keys, digests = big_case
    rep, key_rep, flags, counts = check(eng, keys, digests)
    assert counts["files"] == 100003 and counts["keys"] == 30000 and counts["classes"] == 60000
    assert counts["collided_keys"] == 20000 and counts["duplicate_files"] == 40003


def test_smaller_call_after_a_larger_one(eng, big_case):
    """the tables and counters are cleared per call: no claim of the larger
    call survives into the smaller, which reuses its keys and digests"""
    keys, digests = big_case
    check(eng, keys[:50000], digests[:50000])
    check(eng, keys[40000:40700], digests[40000:40700])
    check(eng, keys[:3], digests[:3])


def test_null_outputs_one_at_a_time(eng):
    keys, digests = shuffled_classes(1000, 150, seed=3)
    valid = (np.arange(1000) % 7 != 0).astype(np.uint8)
    want = group_by(keys, digests, valid)
    for skip in range(4):
        outputs = tuple(j != skip for j in range(4))
        got = device_call(eng, keys, digests, valid, outputs)
        for j in range(4):
            assert got[j] is None if j == skip else _same(got[j], want[j]), (skip, j)
        # the host call with the same output null
        rep, krep, fl = np.zeros(1000, np.int64), np.zeros(1000, np.int64), np.zeros(1000, np.uint8)
        cnt = N.ConfirmCounts()
        import ctypes
        ptrs = [rep.ctypes.data, krep.ctypes.data, fl.ctypes.data, ctypes.byref(cnt)]
        ptrs[skip] = None
        k, d = np.ascontiguousarray(keys), np.ascontiguousarray(digests)
        rc = eng.L.sdcas_confirm_duplicates(eng.ctx, k.ctypes.data, d.ctypes.data, valid.ctypes.data, 1000, *ptrs)
        assert rc == N.SDCAS_OK
        for j, g in enumerate((rep, krep, fl, cnt.as_dict())):
            if j != skip:
                assert _same(g, want[j]), (skip, j)
    assert device_call(eng, keys, digests, valid, (False, False, False, False)) == (None, None, None, None)


def test_argument_errors(eng):
    k = torch.zeros(8, dtype=torch.int64, device="cuda")
    d = torch.zeros(8 * 32 + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L, ctx = eng.L, eng.ctx
    assert L.sdcas_dev_confirm_duplicates(ctx, k.data_ptr(), d.data_ptr() + 8, None, 8, None, None, None, None,
                                          None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_confirm_duplicates(ctx, None, d.data_ptr(), None, 8, None, None, None, None,
                                          None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_confirm_duplicates(ctx, k.data_ptr(), None, None, 8, None, None, None, None,
                                          None) == N.SDCAS_E_INVALID
    assert L.sdcas_dev_confirm_duplicates(ctx, k.data_ptr(), d.data_ptr(), None, (1 << 30) + 1, None, None, None,
                                          None, None) == N.SDCAS_E_CAPACITY
    hk = np.zeros(8, np.uint64)
    assert L.sdcas_confirm_duplicates(ctx, hk.ctypes.data, None, None, 8, None, None, None,
                                      None) == N.SDCAS_E_INVALID
    assert L.sdcas_confirm_duplicates(ctx, hk.ctypes.data, hk.ctypes.data, None, (1 << 30) + 1, None, None, None,
                                      None) == N.SDCAS_E_CAPACITY
    # 16-byte aligned but not 32: accepted
    torch.cuda.synchronize()
    eng.dev_confirm_duplicates(k.data_ptr(), d.data_ptr() + 16, 0, 8)
    eng.dev_sync()


# ---- real files ----------------------------------------------------------------------

def test_identify_confirmed_on_real_files(eng, oracle, tmp_path):
    rng = np.random.default_rng(99)

    def blob(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    small, mid, big = blob(3 * 1024), blob(150 * 1024), bytearray(blob(204800))
    # offset 20 000 of a 204 800-byte file is read by no cas window
    assert cas_windows(204800) == [(0, 8192), (8192, 10240), (55296, 10240), (102400, 10240), (149504, 10240),
                                   (196608, 8192)]
    assert not any(off <= 20000 < off + n for off, n in cas_windows(204800))
    other = bytearray(big)
    other[20000] ^= 0x40
    files = [("u0.bin", blob(700)), ("s1.bin", small), ("m1.bin", mid), ("c1.bin", bytes(big)), ("u1.bin", blob(9000)),
             ("s2.bin", small), ("empty.bin", b""), ("u2.bin", blob(102400)), ("c2.bin", bytes(other)),
             ("u3.bin", blob(102401)), ("m2.bin", mid), ("s3.bin", small), ("u4.bin", blob(1)),
             ("u5.bin", blob(40000)), ("u6.bin", blob(204800)), ("u7.bin", blob(65536)), ("u8.bin", blob(5000))]
    paths = []
    for name, data in files:
        p = tmp_path / name
        p.write_bytes(data)
        paths.append(str(p))
    (tmp_path / "a_directory").mkdir()
    paths += [str(tmp_path / "a_directory"), str(tmp_path / "missing.bin")]
    idx = {os.path.basename(p): i for i, p in enumerate(paths)}
    n = len(paths)
    assert n == 19

    # the oracle: the pair shares its cas_id, the checksums differ
    size = {i: os.path.getsize(paths[i]) for i in range(len(files))}
    cas = {i: oracle.generate_cas_id(paths[i], size[i]) for i in range(len(files)) if size[i]}
    chk = {i: oracle.file_checksum(paths[i]) for i in range(len(files))}
    c1, c2 = idx["c1.bin"], idx["c2.bin"]
    assert cas[c1] == cas[c2] and chk[c1] != chk[c2]

    (sizes, keys, digests, status, mflags), (rep, key_rep, flags, counts) = eng.identify_confirmed(paths)
    for i in range(len(files)):
        assert status[i] == 0 and sizes[i] == size[i]
        assert bytes(digests[i]).hex() == chk[i], paths[i]
        if size[i]:
            assert f"{int(keys[i]):016x}" == cas[i], paths[i]
    # the identical sets
    s = [idx["s1.bin"], idx["s2.bin"], idx["s3.bin"]]
    m = [idx["m1.bin"], idx["m2.bin"]]
    assert rep[s].tolist() == [s[0]] * 3 and flags[s].tolist() == [0, DUP, DUP]
    assert rep[m].tolist() == [m[0]] * 2 and flags[m].tolist() == [0, DUP]
    assert key_rep[s].tolist() == [s[0]] * 3 and key_rep[m].tolist() == [m[0]] * 2
    # the colliding pair: each its own class, the key's lowest file the first
    assert rep[[c1, c2]].tolist() == [c1, c2] and key_rep[[c1, c2]].tolist() == [c1, c1]
    assert flags[[c1, c2]].tolist() == [COL, COL]
    # the empty file, the directory and the missing path take no part
    for name in ("empty.bin", "a_directory", "missing.bin"):
        i = idx[name]
        assert flags[i] == SKIP and rep[i] == -1 and key_rep[i] == -1, name
    assert status[idx["missing.bin"]] != 0 and mflags[idx["a_directory"]] & N.SDCAS_META_DIR
    # every other file is alone
    rest = [i for i in range(n) if i not in s + m + [c1, c2, idx["empty.bin"], idx["a_directory"], idx["missing.bin"]]]
    assert len(rest) == 9 and all(rep[i] == i and key_rep[i] == i and flags[i] == 0 for i in rest)
    assert counts == {"files": 16, "classes": 13, "keys": 12, "collided_keys": 1, "collided_files": 2,
                      "duplicate_files": 3}
    # and the whole answer is the checker's over the oracle's strings
    valid = np.array([1 if i in cas else 0 for i in range(n)], np.uint8)
    okeys = np.array([int(cas.get(i, "0"), 16) for i in range(n)], np.uint64)
    odig = np.zeros((n, 32), np.uint8)
    for i, h in chk.items():
        odig[i] = np.frombuffer(bytes.fromhex(h), np.uint8)
    want = group_by(okeys, odig, valid)
    assert _same(rep, want[0]) and _same(key_rep, want[1]) and _same(flags, want[2]) and counts == want[3]


# ---- chained on the device -------------------------------------------------------------

def test_dev_identify_then_confirm_on_one_stream(eng, oracle):
    """sdcas_dev_identify's three outputs go into sdcas_dev_confirm_duplicates
    as they are, on the context's stream, with no host copy in between"""
    rng = np.random.default_rng(8)
    contents = [(content_key(0xC0F1, c), int(s)) for c, s in
                enumerate([0, 1, 1000, 5000, 70000, 1016, 1017, 33, 2048, 102400, 64, 0])]
    pick = rng.integers(0, len(contents), 48)
    ckeys = [contents[p][0] for p in pick]
    sizes = [contents[p][1] for p in pick]
    n = len(pick)
    offs, off = [], 16
    for s in sizes:
        offs.append(off)
        off = (off + s + 64 + 15) // 16 * 16 + 16
    blob = torch.zeros(off + 64, dtype=torch.uint8, device="cuda")
    args = [_i64(ckeys), _i64([0] * n), _i64(sizes), _i64(offs)]
    k = torch.zeros(n, dtype=torch.int64, device="cuda")
    d = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    h = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    rep = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    krep = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    fl = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((6,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.dev_synth_content(*(a.data_ptr() for a in args), n, blob.data_ptr())
    a = sum(max(1, -(-(s + 8) // 1024)) if 1 <= s <= 102400 else 1 for s in sizes)
    eng.dev_reserve(n, 2 * (a + 2048) + 4096)
    eng.dev_identify(blob.data_ptr(), args[3].data_ptr(), args[2].data_ptr(), n, k.data_ptr(), d.data_ptr(),
                     h.data_ptr())
    eng.dev_confirm_duplicates(k.data_ptr(), d.data_ptr(), h.data_ptr(), n, rep.data_ptr(), krep.data_ptr(),
                               fl.data_ptr(), cnt.data_ptr())
    eng.dev_sync()
    okeys = np.array([oracle.synth_cas_key(ck, s) if s else 0 for ck, s in zip(ckeys, sizes)], np.uint64)
    odig = np.stack([np.frombuffer(bytes.fromhex(oracle.synth_checksum(ck, s)), np.uint8)
                     for ck, s in zip(ckeys, sizes)])
    valid = np.array([1 if s else 0 for s in sizes], np.uint8)
    assert (k.cpu().numpy().view(np.uint64)[valid != 0] == okeys[valid != 0]).all()
    assert (d.cpu().numpy() == odig).all() and (h.cpu().numpy() == valid).all()
    want = group_by(okeys, odig, valid)
    assert _same(rep.cpu().numpy(), want[0]) and _same(krep.cpu().numpy(), want[1])
    assert _same(fl.cpu().numpy(), want[2])
    assert dict(zip(COUNTS, (int(x) for x in cnt.cpu().numpy()))) == want[3]
    assert want[3]["duplicate_files"] > 20 and want[3]["files"] < n and want[3]["collided_keys"] == 0
