"""The family store, the host layers: the entry points in the header, the
binding and the library, the GPU-free plan and tile size, spacedrive_amd.recipes'
store functions against the plain reference, and FamilyStore's save, load and
the checks a loaded file passes. The kernels' tests are
tests/test_gpu_family_store.py and tests/test_gpu_store_files.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from spacedrive_amd import FamilyStore, _native as N
from spacedrive_amd.engine import Engine
from spacedrive_amd.recipes import STORE_NONE, pack_store, restore_from_store, store_layout
from tests import _family_recipes_ref as R
from tests import _family_store_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sdcas_family_store_plan": 3, "sdcas_dev_family_store_layout": 15, "sdcas_dev_family_pack": 19,
           "sdcas_dev_family_restore": 17, "sdcas_family_store_layout": 13, "sdcas_family_pack": 17,
           "sdcas_family_restore": 15}
KERNELS = ("k_fs_sum", "k_fs_scan", "k_fs_literal", "k_fs_copy", "k_fs_counts", "k_fs_clip", "k_fs_starts",
           "k_fs_move", "k_fs_moved")


def plan(max_ops, n):
    ws = ctypes.c_uint64(0)
    rc = N.load().sdcas_family_store_plan(max_ops, n, ctypes.byref(ws))
    return rc, ws.value


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdcas.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (sdcas_\w+)", out))
    for name, nargs in SYMBOLS.items():
        assert name in N.ABI_SYMBOLS and name in exported, name
        assert len(getattr(N.load(), name).argtypes) == nargs, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
    assert "sdcas_family_store_tile_bytes" in exported and "sdcas_family_store_tile_bytes" in N.ABI_SYMBOLS
    assert "#define SDCAS_ABI_VERSION 7" in hdr and N.load().sdcas_abi_version() == 7
    section = hdr[hdr.index("family store: pack the literal bytes and restore files from them"):]
    assert "added after abi 7; probe for the symbol (sdcas_abi_version stays 7)" in section[:300].lower()
    for struct, names, cls in (("sdcas_family_store_counts", S.LAYOUT_COUNTS, N.FamilyStoreCounts),
                               ("sdcas_family_move_counts", S.MOVE_COUNTS, N.FamilyMoveCounts)):
        fields = re.findall(r"uint64_t (\w+);", section[section.index("typedef struct " + struct):
                                                        section.index("} %s;" % struct)])
        assert fields == list(names) == [name for name, _ in cls._fields_]
        assert ctypes.sizeof(cls) == 8 * len(names)
    assert "store_off [0, 0, 60, 30]" in section and "store_bytes 65" in section


def test_library_holds_the_kernels():
    out = subprocess.run(["nm", "-C", N.LIB_PATH], capture_output=True, text=True).stdout
    for k in KERNELS:
        assert k in out, k


def test_plan_ranges_and_bytes():
    assert plan(1 << 30, 1 << 30)[0] == N.SDCAS_OK
    assert plan((1 << 30) + 1, 4)[0] == N.SDCAS_E_CAPACITY
    assert plan(4, (1 << 30) + 1)[0] == N.SDCAS_E_CAPACITY
    assert plan(0, 0)[0] == N.SDCAS_OK
    assert N.load().sdcas_family_store_plan(5, 5, None) == N.SDCAS_OK
    rc, small = plan(1, 1)
    rc2, big = plan(1 << 20, 1)
    assert rc == rc2 == N.SDCAS_OK and 0 < small < big
    assert 32 << 20 <= big <= (32 << 20) + (64 << 10)  # 32 bytes per op, the sums and the counters
    assert Engine.family_store_plan(1 << 20, 1) == big
    with pytest.raises(N.SdcasError) as e:
        Engine.family_store_plan((1 << 30) + 1, 1)
    assert e.value.code == N.SDCAS_E_CAPACITY


def test_tile_bytes():
    t = N.load().sdcas_family_store_tile_bytes()
    assert t > 0 and t % 16 == 0 and Engine.family_store_tile_bytes() == t


@pytest.fixture(scope="module")
def corpus():
    contents, fl, off, ln, rep, fam = R.versions(5, n_families=12, max_versions=5, blocks=20)
    rec = R.family_recipes(fl, off, ln, rep, fam)
    return contents, rec


def test_recipes_functions_against_the_reference(corpus):
    contents, rec = corpus
    read = lambda row, at, n: contents[row][at:at + n]
    lay, want = store_layout(rec), S.layout(rec)
    assert np.array_equal(lay["op_store_off"], want["op_store_off"]) and lay["counts"] == want["counts"]
    assert lay["op_store_off"].dtype == np.uint64
    store = pack_store(rec, lay, read)
    assert store.dtype == np.uint8 and store.tobytes() == bytes(S.pack_all(rec, want, contents))
    sizes = [len(c) if rec["row_ops"][r] else 0 for r, c in enumerate(contents)]
    assert restore_from_store(rec, lay, store) == S.restore_all(rec, want, bytearray(store.tobytes()), sizes)
    assert restore_from_store(rec, lay, store, rows=[2]) == {2: contents[2]}
    # arbitrary arrays: wrapping offsets and lengths, sources out of range
    rng = np.random.default_rng(3)
    k, m = 200, 260
    odd = {"op_chunk": rng.integers(0, m, k).astype(np.uint32), "op_row": rng.integers(0, 9, k).astype(np.uint32),
           "op_src_row": rng.integers(0, 9, k).astype(np.uint32),
           "op_dst_off": rng.integers(0, 1 << 64, k, dtype=np.uint64) >> rng.integers(0, 64, k).astype(np.uint64),
           "op_src_off": rng.integers(0, 1 << 64, k, dtype=np.uint64) >> rng.integers(0, 64, k).astype(np.uint64),
           "op_len": rng.integers(0, 1 << 64, k, dtype=np.uint64) >> rng.integers(0, 64, k).astype(np.uint64),
           "chunk_op": rng.integers(0, k + 40, m).astype(np.uint32)}
    odd["op_src_chunk"] = np.where(rng.random(k) < 0.5, odd["op_chunk"], rng.integers(0, m + 30, k)).astype(np.uint32)
    lay, want = store_layout(odd), S.layout(odd)
    assert np.array_equal(lay["op_store_off"], want["op_store_off"]) and lay["counts"] == want["counts"]
    with pytest.raises(ValueError):
        pack_store(rec, {"op_store_off": lay["op_store_off"], "counts": lay["counts"]}, read)
    with pytest.raises(ValueError):
        pack_store(rec, store_layout(rec), lambda row, at, n: b"")
    bad = store_layout(rec)
    bad["op_store_off"][int(np.flatnonzero(~rec["op_literal"])[0])] = STORE_NONE
    with pytest.raises(ValueError):
        restore_from_store(rec, bad, store)


def make_store(corpus):
    contents, rec = corpus
    lay = store_layout(rec)
    store = pack_store(rec, lay, lambda row, at, n: contents[row][at:at + n])
    sizes = np.array([len(c) for c in contents], np.uint64)
    digests = np.arange(32 * len(contents), dtype=np.uint64).astype(np.uint8).reshape(-1, 32)
    return FamilyStore(rec, lay, store, sizes, digests)


def test_save_and_load_round_trip(corpus, tmp_path):
    fs = make_store(corpus)
    path = tmp_path / "families.npz"
    fs.save(path)
    back = FamilyStore.load(path)
    assert R.same(back.recipes, fs.recipes)
    assert np.array_equal(back.layout["op_store_off"], fs.layout["op_store_off"])
    assert back.layout["counts"] == fs.layout["counts"]
    assert np.array_equal(back.store, fs.store) and np.array_equal(back.sizes, fs.sizes)
    assert np.array_equal(back.digests, fs.digests) and back.store.dtype == np.uint8
    assert restore_from_store(back.recipes, back.layout, back.store) == \
        restore_from_store(fs.recipes, fs.layout, fs.store)
    with pytest.raises(ValueError):
        FamilyStore.load(tmp_path / "missing.npz")
    (tmp_path / "junk.npz").write_bytes(b"not an archive")
    with pytest.raises(ValueError):
        FamilyStore.load(tmp_path / "junk.npz")


def damage(path, out, **changes):
    with np.load(path) as z:
        parts = {k: z[k] for k in z.files}
    for k, fn in changes.items():
        parts[k] = fn(parts[k].copy())
    with open(out, "wb") as f:
        np.savez(f, **parts)
    return out


def bump(i, by=1):
    def fn(a):
        a[i] += by
        return a
    return fn


@pytest.mark.parametrize("name,change", [
    ("op_len", lambda a: a[:-1]),                      # array lengths
    ("op_store_off", lambda a: a[:-1]),
    ("digests", lambda a: a[:-1]),
    ("sizes", lambda a: a[:-1]),
    ("row_ops", lambda a: a[:-1]),
    ("store", lambda a: a[:-1]),                       # the store's size
    ("store", lambda a: np.concatenate([a, a[:1]])),
    ("recipes_counts", bump(2)),                       # ops consistent
    ("layout_counts", bump(0)),
    ("layout_counts", bump(4)),                        # store_bytes
    ("layout_counts", lambda a: a[:-1]),
    ("op_store_off", bump(-1, 1)),                     # offsets within the store, and the recipes' own
    ("op_store_off", bump(0, 1 << 40)),
    ("op_row", bump(0, 1 << 20)),                      # rows in range
    ("chunk_op", bump(0, 1 << 20)),                    # chunk_op in range
    ("op_len", bump(0, 1 << 50)),                      # ops inside their rows
    ("op_dst_off", bump(0, 1 << 63)),
])
def test_load_checks_fire(corpus, tmp_path, name, change):
    fs = make_store(corpus)
    good = tmp_path / "good.npz"
    fs.save(good)
    FamilyStore.load(good)
    with pytest.raises(ValueError):
        FamilyStore.load(damage(good, tmp_path / "bad.npz", **{name: change}))


def test_load_rejects_a_missing_part(corpus, tmp_path):
    fs = make_store(corpus)
    good = tmp_path / "good.npz"
    fs.save(good)
    with np.load(good) as z:
        parts = {k: z[k] for k in z.files if k != "op_store_off"}
    with open(tmp_path / "bad.npz", "wb") as f:
        np.savez(f, **parts)
    with pytest.raises(ValueError):
        FamilyStore.load(tmp_path / "bad.npz")


def test_the_tool_counts_without_a_device():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ab_family_store", os.path.join(ROOT, "tools", "ab_family_store.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    t = N.load().sdcas_family_store_tile_bytes()
    one = tool.model("one_op")
    assert one["ops"] == 1 and one["pack"]["bytes_moved"] == one["restore"]["bytes_moved"] == 4 << 30
    assert one["pack"]["tiles"] == (4 << 30) // t and one["launches"] == {"layout": 5, "pack": 5, "restore": 5}
    hot = tool.model("one_class")
    assert hot["counts"]["store_bytes"] == 64 << 10 and hot["counts"]["uncovered_ops"] == 0
    assert hot["pack"]["bytes_moved"] == 64 << 10 and hot["restore"]["bytes_moved"] == 65537 * (64 << 10)
    assert hot["workspace_bytes"] == plan(65537, 65537)[1]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_family_store.py"), "--count-only", "--shapes",
                          "one_op"], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert out.returncode == 0 and '"tile_bytes": %d' % t in out.stdout
