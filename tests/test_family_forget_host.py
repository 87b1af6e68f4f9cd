"""A family store that forgets rows, without a GPU: the entry points, the numpy
forms in spacedrive_amd/recipes.py against the plain-Python reference
(tests/_family_forget_ref.py), the law that removal gives the store of the
surviving files alone, keep's laws, moves' definition on hand-made inputs, and
FamilyStore's chunk arrays through save, load and check."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from spacedrive_amd import FamilyStore, _native as N
from spacedrive_amd.engine import Engine
from spacedrive_amd.recipes import STORE_NONE, apply_moves, keep_chunks, pack_store, store_layout, store_moves
from tests import _family_forget_ref as F
from tests import _family_recipes_ref as R
from tests import _family_store_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_family_forget_plan": 3, "sdcas_family_chunks_keep": 18, "sdcas_dev_family_chunks_keep": 19,
           "sdcas_family_store_moves": 21, "sdcas_dev_family_store_moves": 25}
KERNELS = ("k_fg_rows", "k_fg_chunks", "k_fg_scan", "k_fg_row_scatter", "k_fg_row_family", "k_fg_chunk_scatter",
           "k_fg_chunk_rep", "k_fg_keep_counts", "k_fg_flag", "k_fg_emit", "k_fg_close", "k_fg_moves_counts")
SEEDS = range(12)


def same_keep(got, want):
    for name in F.KEEP_ARRAYS:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert got["counts"] == want["counts"]


def same_moves(got, want):
    for name in F.MOVE_ARRAYS:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.dtype == b.dtype == np.uint64 and np.array_equal(a, b), name
    assert got["counts"] == want["counts"]


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sdcas_\w+)", out))
    for name, nargs in SYMBOLS.items():
        assert name in N.ABI_SYMBOLS and name in exported, name
        assert len(getattr(N.load(), name).argtypes) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
    assert "#define SDCAS_ABI_VERSION 7" in hdr and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("family store: forget rows"):]
    assert "added after abi 7; probe for the symbol (sdcas_abi_version stays 7)" in section[:300].lower()
    for struct, names, cls in (("sdcas_family_keep_counts", F.KEEP_COUNTS, N.FamilyKeepCounts),
                               ("sdcas_family_moves_counts", F.MOVES_COUNTS, N.FamilyMovesCounts)):
        fields = re.findall(r"uint64_t (\w+);", section[section.index("typedef struct " + struct):
                                                        section.index("} %s;" % struct)])
        assert fields == list(names) == [name for name, _ in cls._fields_]
        assert ctypes.sizeof(cls) == 8 * len(names)
    assert "(0, 0, 30), (30, 60, 5), (35, 30, 30)" in section
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in KERNELS:
        assert k in out, k


def test_plan_ranges_and_bytes():
    def plan(m, n):
        ws = ctypes.c_uint64(0)
        return N.load().sdcas_family_forget_plan(m, n, ctypes.byref(ws)), ws.value
    assert plan(1 << 30, 1 << 30)[0] == N.SDCAS_OK and plan(0, 0)[0] == N.SDCAS_OK
    assert plan((1 << 30) + 1, 4)[0] == N.SDCAS_E_CAPACITY and plan(4, (1 << 30) + 1)[0] == N.SDCAS_E_CAPACITY
    assert N.load().sdcas_family_forget_plan(5, 5, None) == N.SDCAS_OK
    (rc, small), (rc2, big) = plan(1, 1), plan(1 << 20, 1)
    assert rc == rc2 == N.SDCAS_OK and 0 < small < big
    assert 17 << 20 <= big <= (17 << 20) + (64 << 10)  # moves' 17 bytes per chunk, the sums and the counters
    assert plan(1, 1 << 20)[1] >= 8 << 20              # keep's 8 bytes per row
    assert Engine.family_forget_plan(1 << 20, 1) == big
    with pytest.raises(N.SdcasError) as e:
        Engine.family_forget_plan((1 << 30) + 1, 1)
    assert e.value.code == N.SDCAS_E_CAPACITY


def old_store(seed):
    contents, fl, off, ln, rep, fam = R.versions(seed)
    rec = R.family_recipes(fl, off, ln, rep, fam)
    rec["chunk_off"] = off
    lay = S.layout(rec)
    return contents, (fl, off, ln, rep, fam), rec, lay, S.pack_all(rec, lay, contents)


@pytest.mark.parametrize("seed", SEEDS)
def test_removal_gives_the_store_of_the_surviving_files(seed):
    contents, arrays, rec, lay, store = old_store(seed)
    fl, off, ln, rep, fam = arrays
    assert lay["counts"]["uncovered_ops"] == 0
    for name, mask in F.masks(seed, fam):
        kept = keep_chunks(fl, off, ln, rep, fam, mask)
        same_keep(kept, F.keep(fl, off, ln, rep, fam, mask))
        rec2 = R.family_recipes(kept["chunk_file"], kept["chunk_off"], kept["chunk_len"], kept["rep"], kept["family"])
        rec2["chunk_off"] = kept["chunk_off"]
        lay2 = S.layout(rec2)
        mv = store_moves(rec, lay, rec2, lay2, kept["chunk_from"], kept["chunk_len"])
        same_moves(mv, F.moves(F.old_side(rec, lay, off), F.new_side(kept, rec2, lay2)))
        new = apply_moves(mv, np.frombuffer(bytes(store), np.uint8))
        # the law: the store built from the surviving files alone
        contents2, want_rec, want_lay, want_store = F.from_scratch(contents, fl, off, ln, fam, mask)
        assert R.same(rec2, want_rec), name
        assert np.array_equal(lay2["op_store_off"], want_lay["op_store_off"]) and lay2["counts"] == want_lay["counts"]
        assert new.dtype == np.uint8 and new.tobytes() == bytes(want_store), name
        assert new.tobytes() == bytes(F.apply(mv, store, lay2["counts"]["store_bytes"]))
        assert mv["counts"]["lost_chunks"] == 0 and mv["counts"]["lost_bytes"] == 0
        assert len(new) == lay2["counts"]["store_bytes"] <= lay["counts"]["store_bytes"]
        assert mv["counts"]["moved_bytes"] == len(new)
        # the moves' destinations are disjoint and cover the new store
        at = 0
        for d, n in sorted(zip(mv["move_dst"].tolist(), mv["move_len"].tolist())):
            assert d == at
            at += n
        assert at == len(new)
        # every surviving file comes back
        sizes = [len(c) if want_rec["row_ops"][r] else 0 for r, c in enumerate(contents2)]
        back = S.restore_all(rec2, lay2, bytearray(new.tobytes()), sizes)
        assert all(back[r] == (contents2[r] if sizes[r] else b"") for r in range(len(contents2)))


def test_the_header_example():
    ex = R.EXAMPLE
    rec = R.family_recipes(**ex)
    rec["chunk_off"] = np.array(ex["chunk_off"], np.uint64)
    lay = S.layout(rec)
    assert lay["op_store_off"].tolist() == S.EXAMPLE_STORE_OFF
    for keep_fn in (keep_chunks, F.keep):
        kept = keep_fn(ex["chunk_file"], ex["chunk_off"], ex["chunk_len"], ex["rep"], ex["family"], F.EXAMPLE_KEEP)
        assert kept["row_new"].tolist() == [0xFFFFFFFF, 0] and kept["row_from"].tolist() == [1]
        assert kept["family"].tolist() == [0] and kept["chunk_from"].tolist() == [3, 4, 5, 6]
        assert kept["chunk_file"].tolist() == [0, 0, 0, 0] and kept["chunk_off"].tolist() == [0, 10, 30, 35]
        assert kept["chunk_len"].tolist() == [10, 20, 5, 30] and kept["rep"].tolist() == [0, 1, 2, 3]
        assert kept["counts"] == dict(rows_kept=1, rows_removed=1, chunks_kept=4, chunks_removed=3, bytes_kept=65,
                                      bytes_removed=60)
    rec2 = R.family_recipes(kept["chunk_file"], kept["chunk_off"], kept["chunk_len"], kept["rep"], kept["family"])
    rec2["chunk_off"] = kept["chunk_off"]
    assert rec2["counts"]["ops"] == rec2["counts"]["literal_ops"] == 1 and rec2["op_len"].tolist() == [65]
    lay2 = S.layout(rec2)
    ref = F.moves(F.old_side(rec, lay, ex["chunk_off"]), F.new_side(kept, rec2, lay2))
    assert ref["old_at"] == F.EXAMPLE_OLD_AT
    mv = store_moves(rec, lay, rec2, lay2, kept["chunk_from"], kept["chunk_len"])
    for got in (mv, ref):
        assert {k: got[k].tolist() for k in F.MOVE_ARRAYS} == F.EXAMPLE_MOVES
        assert got["counts"] == F.EXAMPLE_MOVES_COUNTS
    a, b, c, x = b"a" * 10, b"b" * 20, b"c" * 30, b"x" * 5
    assert apply_moves(mv, np.frombuffer(a + b + c + x, np.uint8)).tobytes() == a + b + x + c


def odd_inputs(seed, m=300, n=40):
    """rep outside [0, c], chunk_file >= n, labels -1, n, 2^40 and -2^63"""
    rng = np.random.default_rng(seed)
    fl = np.sort(rng.integers(0, n + 3, m)).astype(np.uint32)
    ln = rng.integers(0, 50, m).astype(np.uint64)
    off = rng.integers(0, 1 << 64, m, dtype=np.uint64) >> rng.integers(0, 64, m).astype(np.uint64)
    rep = np.minimum(rng.integers(0, 40, m), np.arange(m)).astype(np.int64)
    wild = rng.random(m) < 0.2
    rep[wild] = rng.choice([-1, m, m + 7, 1 << 40, -(1 << 63)], int(wild.sum())) + np.where(
        rng.random(int(wild.sum())) < 0.5, 0, np.arange(m)[wild])
    fam = rng.integers(0, 6, n).astype(np.int64)
    fam[rng.integers(0, n, 8)] = [-1, n, 1 << 40, -(1 << 63), n + 1, -2, (1 << 63) - 1, n]
    return fl, off, ln, rep, fam


@pytest.mark.parametrize("seed", range(6))
def test_keeps_laws(seed):
    fl, off, ln, rep, fam = odd_inputs(seed)
    m, n = fl.size, fam.size
    rng = np.random.default_rng(50 + seed)
    a, b = rng.random(n) < 0.7, rng.random(n) < 0.7
    one = keep_chunks(fl, off, ln, rep, fam, a)
    same_keep(one, F.keep(fl, off, ln, rep, fam, a))
    r2 = one["rep"]
    pos = np.arange(r2.size)
    assert ((r2 >= 0) & (r2 <= pos)).all() and np.array_equal(r2[r2], r2)  # idempotent, at or below
    r = np.where((rep >= 0) & (rep <= np.arange(m)), rep, np.arange(m))[one["chunk_from"]]
    for i in range(r2.size):  # equal out_rep if and only if equal class number
        assert np.array_equal(r2 == r2[i], r == r[i])
    lab, rows = one["family"], one["row_from"]
    part = (fam[rows] >= 0) & (fam[rows] < n)
    assert ((lab == -1) == ~part).all()
    for i in np.flatnonzero(part):  # equal labels if and only if they were equal
        assert np.array_equal((lab == lab[i]) & part, (fam[rows] == fam[rows][i]) & part)
    assert ((lab[part] >= 0) & (lab[part] <= np.flatnonzero(part))).all()
    # keep(A) then keep(B) over its outputs equals one keep of the rows both keep
    two = keep_chunks(one["chunk_file"], one["chunk_off"], one["chunk_len"], one["rep"], one["family"], b[rows])
    both = keep_chunks(fl, off, ln, rep, fam, a & b)
    for name in ("family", "chunk_file", "chunk_off", "chunk_len", "rep"):
        assert np.array_equal(two[name], both[name]), name
    assert np.array_equal(rows[two["row_from"]], both["row_from"])
    assert np.array_equal(one["chunk_from"][two["chunk_from"]], both["chunk_from"])
    for key in ("rows_kept", "chunks_kept", "bytes_kept"):
        assert two["counts"][key] == both["counts"][key]
    # keep-all changes nothing but the normal form of rep and the labels
    whole = keep_chunks(fl, off, ln, rep, fam, np.ones(n, bool))
    assert whole["counts"]["rows_removed"] == 0 and whole["counts"]["chunks_kept"] == int((fl < n).sum())
    with pytest.raises(ValueError):
        keep_chunks(fl, off, ln, rep, fam, a[:-1])
    with pytest.raises(ValueError):
        keep_chunks(fl, off[:-1], ln, rep, fam, a)


def test_confirms_rep_over_the_survivors():
    contents, fl, off, ln, rep, fam = R.versions(3, n_families=5, max_versions=5)
    rng = np.random.default_rng(9)
    mask = rng.random(fam.size) < 0.5
    kept = keep_chunks(fl, off, ln, rep, fam, mask)
    seen, want = {}, []
    for c in kept["chunk_from"]:
        want.append(seen.setdefault(contents[fl[c]][int(off[c]):int(off[c] + ln[c])], len(want)))
    assert kept["rep"].tolist() == want


def hand_made():
    """two old ops (a literal at 0, a copy with a place), six new chunks of one new literal op"""
    old = dict(chunk_off=np.array([0, 10, 20, 30, 5, 0], np.uint64),
               chunk_op=np.array([0, 0, 0xFFFFFFFF, 1, 2, 3], np.uint32),
               op_dst_off=np.array([0, 30, 9, 0], np.uint64),
               op_store_off=np.array([100, 110, 50, STORE_NONE], np.uint64))
    new = dict(chunk_from=np.array([0, 1, 2, 3, 4, 5, 9], np.uint32),
               chunk_off=np.array([0, 10, 20, 30, 40, 50, 60], np.uint64),
               chunk_len=np.array([10, 10, 10, 10, 10, 10, 3], np.uint64),
               chunk_op=np.array([0, 0, 0, 0, 0, 0, 0], np.uint32), op_chunk=np.array([0], np.uint32),
               op_src_chunk=np.array([0], np.uint32), op_dst_off=np.array([0], np.uint64),
               op_store_off=np.array([0], np.uint64))
    return old, new


def moves_np(old, new):
    return store_moves({"chunk_off": old["chunk_off"], "chunk_op": old["chunk_op"], "op_dst_off": old["op_dst_off"]},
                       {"op_store_off": old["op_store_off"]},
                       {"chunk_off": new["chunk_off"], "chunk_op": new["chunk_op"], "op_chunk": new["op_chunk"],
                        "op_src_chunk": new["op_src_chunk"], "op_dst_off": new["op_dst_off"]},
                       {"op_store_off": new["op_store_off"]}, new["chunk_from"], new["chunk_len"])


def test_moves_by_hand():
    old, new = hand_made()
    ref = F.moves(old, new)
    # chunk 2: old op 0xFFFFFFFF; chunk 4: chunk_off 5 below the op's dst_off 9; chunk 5: a store offset of NONE;
    # chunk 6: an old position past m. Each is lost and counted, never followed. Chunk 3 follows a lost chunk: a head,
    # though 110 is where a chunk after chunk 1 would lie.
    assert ref["old_at"] == [100, 110, F.NONE, 110, F.NONE, F.NONE, F.NONE]
    assert ref["move_dst"].tolist() == [0, 30] and ref["move_src"].tolist() == [100, 110]
    assert ref["move_len"].tolist() == [20, 10]
    assert ref["counts"] == dict(moves=2, literal_chunks=7, moved_bytes=30, lost_chunks=4, lost_bytes=33,
                                 longest_move=20)
    same_moves(moves_np(old, new), ref)
    # a chunk that is no literal, an op past the new ops, a run cut by another new op
    new["op_chunk"], new["op_src_chunk"] = np.array([0, 3, 1], np.uint32), np.array([0, 3, 0], np.uint32)
    new["op_dst_off"], new["op_store_off"] = np.array([0, 30, 10], np.uint64), np.array([0, 20, 7], np.uint64)
    new["chunk_op"] = np.array([0, 2, 9, 1, 1, 0xFFFFFFFF, 1], np.uint32)
    old["chunk_op"][:4] = [0, 0, 0, 0]
    old["chunk_off"][:4] = [0, 10, 20, 30]
    ref = F.moves(old, new)
    assert ref["move_dst"].tolist() == [0, 20] and ref["move_src"].tolist() == [100, 130]
    assert ref["counts"]["literal_chunks"] == 4 and ref["counts"]["lost_chunks"] == 2
    same_moves(moves_np(old, new), ref)
    # nothing at all
    empty = {k: v[:0] for k, v in new.items()}
    same_moves(moves_np(old, empty), F.moves(old, empty))
    assert F.moves(old, empty)["counts"]["moves"] == 0
    with pytest.raises(ValueError):
        apply_moves({"move_dst": [0], "move_src": [90], "move_len": [20]}, np.zeros(100, np.uint8))


@pytest.mark.parametrize("seed", range(4))
def test_moves_on_arbitrary_arrays(seed):
    rng = np.random.default_rng(70 + seed)
    m, k, m2, k2 = 90, 30, 120, 25
    wide = lambda n: rng.integers(0, 1 << 64, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64)  # noqa
    old = dict(chunk_off=wide(m), chunk_op=rng.integers(0, k + 5, m).astype(np.uint32), op_dst_off=wide(k),
               op_store_off=np.where(rng.random(k) < 0.2, np.uint64(STORE_NONE), wide(k)))
    old["chunk_op"][rng.integers(0, m, 6)] = 0xFFFFFFFF
    new = dict(chunk_from=np.sort(rng.integers(0, m + 8, m2)).astype(np.uint32), chunk_off=wide(m2),
               chunk_len=rng.integers(0, 30, m2).astype(np.uint64),
               chunk_op=np.sort(rng.integers(0, k2 + 3, m2)).astype(np.uint32),
               op_chunk=rng.integers(0, m2, k2).astype(np.uint32), op_dst_off=wide(k2), op_store_off=wide(k2))
    new["op_src_chunk"] = np.where(rng.random(k2) < 0.7, new["op_chunk"], 0).astype(np.uint32)
    # runs that do continue: consecutive old chunks of one old op, contiguous there
    run = np.arange(10, 30)
    old["chunk_op"][run], old["op_store_off"][3], old["op_dst_off"][3] = 3, 1000, 50
    old["chunk_off"][run] = 50 + 7 * (run - 10)
    new["chunk_from"][40:60], new["chunk_len"][40:60], new["chunk_op"][40:60] = run, 7, 4
    new["op_chunk"][4] = new["op_src_chunk"][4] = 40
    ref = F.moves(old, new)
    assert ref["counts"]["longest_move"] >= 140 and ref["counts"]["lost_chunks"] > 0
    same_moves(moves_np(old, new), ref)


# ---- FamilyStore without a GPU -------------------------------------------------------------

def make_store(seed=5, chunks=True):
    contents, fl, off, ln, rep, fam = R.versions(seed, n_families=6, max_versions=4, strays=3)
    rec = R.family_recipes(fl, off, ln, rep, fam)
    rec["chunk_off"] = off
    lay = store_layout(rec)
    store = pack_store(rec, lay, lambda row, at, n: contents[row][at:at + n])
    sizes = np.array([len(c) for c in contents], np.uint64)
    digests = np.arange(32 * len(contents), dtype=np.uint64).astype(np.uint8).reshape(-1, 32)
    ch = {"chunk_file": fl, "chunk_len": ln, "rep": rep, "family": fam} if chunks else None
    return FamilyStore(rec, lay, store, sizes, digests, chunks=ch)


def test_chunk_arrays_round_trip_and_old_files_load(tmp_path):
    fs = make_store()
    fs.save(tmp_path / "with.npz")
    back = FamilyStore.load(tmp_path / "with.npz")
    for name in ("chunk_file", "chunk_len", "rep", "family"):
        assert back.chunks[name].dtype == fs.chunks[name].dtype and np.array_equal(back.chunks[name], fs.chunks[name])
    assert np.array_equal(back.recipes["chunk_off"], fs.recipes["chunk_off"])
    assert back.recipes["chunk_off"].dtype == np.uint64
    assert R.same(back.recipes, fs.recipes) and np.array_equal(back.store, fs.store)
    # a file saved without them, as every file saved before they were kept
    plain = make_store(chunks=False)
    assert plain.chunks is None
    plain.save(tmp_path / "without.npz")
    with np.load(tmp_path / "without.npz") as z:
        assert not [k for k in z.files if k.startswith("chunks_")]
    old = FamilyStore.load(tmp_path / "without.npz")
    assert old.chunks is None and np.array_equal(old.store, fs.store) and R.same(old.recipes, fs.recipes)
    with pytest.raises(ValueError, match="chunk arrays"):
        old.remove([0])
    with pytest.raises(ValueError, match="chunk arrays"):
        plain.remove([])
    with pytest.raises(ValueError, match="outside"):
        fs.remove([len(fs.sizes)])
    with pytest.raises(ValueError, match="outside"):
        fs.remove([-1])


def test_check_rejects_chunk_arrays_that_disagree(tmp_path):
    fs = make_store()

    def broken(**changes):
        ch = {k: v.copy() for k, v in fs.chunks.items()}
        for k, fn in changes.items():
            ch[k] = fn(ch[k])
        return ch

    def bump(i, by):
        def fn(a):
            a[i] += by
            return a
        return fn

    FamilyStore(fs.recipes, fs.layout, fs.store, fs.sizes, fs.digests, chunks=broken())
    for changes in (dict(chunk_file=lambda a: a[:-1]), dict(chunk_len=lambda a: a[:-1]), dict(rep=lambda a: a[:-1]),
                    dict(family=lambda a: a[:-1]),                  # lengths against chunk_op and sizes
                    dict(chunk_file=bump(0, len(fs.sizes))),        # chunk_file < n
                    dict(chunk_len=bump(0, 1)),                     # a row's chunks add up to its size
                    dict(chunk_file=bump(0, 1))):
        with pytest.raises(ValueError):
            FamilyStore(fs.recipes, fs.layout, fs.store, fs.sizes, fs.digests, chunks=broken(**changes))
    # a stray row takes no part: its chunks are not held against its size
    stray = int(np.flatnonzero(fs.chunks["family"] < 0)[0])
    sizes = fs.sizes.copy()
    sizes[stray] += 5
    FamilyStore(fs.recipes, fs.layout, fs.store, sizes, fs.digests, chunks=broken())
    # and through load
    fs.save(tmp_path / "good.npz")
    with np.load(tmp_path / "good.npz") as z:
        parts = {k: z[k] for k in z.files}
    parts["chunks_chunk_len"] = parts["chunks_chunk_len"].copy()
    parts["chunks_chunk_len"][0] += 1
    with open(tmp_path / "bad.npz", "wb") as f:
        np.savez(f, **parts)
    with pytest.raises(ValueError):
        FamilyStore.load(tmp_path / "bad.npz")


def test_the_tool_counts_without_a_device():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ab_family_forget",
                                                  os.path.join(ROOT, "tools", "ab_family_forget.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    small = tool.model("firsts", m=1 << 13)
    fam = tool.corpus(1 << 13)[4]
    assert small["rows"] == 128 and small["rows_removed"] == int((fam == np.arange(128)).sum()) > 0
    assert small["lost_chunks"] == 0 and small["chunks"] == 1 << 13
    assert small["new_store_bytes"] <= small["old_store_bytes"] and small["moved_bytes"] == small["new_store_bytes"]
    assert small["launches"] == {"keep": 9, "recipes": 7, "layout": 5, "moves": 5, "carry": 5}
    assert small["workspace_bytes"] == Engine.family_forget_plan(small["chunks"], small["rows"])
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_family_forget.py"), "--count-only",
                          "--chunks", "4096"], capture_output=True, text=True,
                         env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0 and '"removal": "every_second"' in out.stdout
