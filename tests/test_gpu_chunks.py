"""Content-defined chunks on the GPU (sdcas_chunk_messages / sdcas_dev_chunk,
csrc/cdc.hip): every array and all six counts against tests/_cdc_ref.py, every
chunk digest against the oracle's BLAKE3 of the chunk's bytes and every key
against the digest's first 8 bytes, through the host call and through the
device call with torch tensors."""
import os

import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests import _cdc_ref as R
from tests._guarded import Guarded, guarded_from
from tests._oracle import content, content_key

pytestmark = pytest.mark.gpu

P = R.TEST_PARAMS
COUNTS = ("files", "chunks", "total_bytes", "hash_cuts", "max_cuts", "end_chunks")
ARRAYS = ("file_chunks", "chunk_off", "chunk_len", "chunk_file")
TILE, STRIP = N.SDCAS_CHUNK_GEAR_TILE, N.SDCAS_CHUNK_GEAR_STRIP
POISON = 0xA7


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def synth(n, cid):
    return content("synth", 0, int(n), content_key(0xCDC0, int(cid)))


def lay_out(files, starts=None):
    """the files in one blob image at 16-byte aligned offsets, 64 bytes at
    least between them and behind the last, every other byte poisoned ->
    (image, offsets, lens)"""
    lens = np.array([len(f) for f in files], np.uint64)
    if starts is None:
        starts, cur = [], 16  # nothing at 0 unless asked for
        for f in files:
            starts.append(cur)
            cur += (len(f) + 64 + 15) // 16 * 16
    size = max([int(s) + len(f) for s, f in zip(starts, files)], default=0) + 64
    img = np.full(size + 16, POISON, np.uint8)
    for s, f in zip(starts, files):
        img[int(s):int(s) + len(f)] = f
    return img, np.array(starts, np.uint64), lens


def reference(files, offs, params, max_share=None):
    want = R.chunk_files(files, offs, params)
    if max_share is not None:  # the input itself must exercise the hash cuts
        c = want["counts"]
        assert c["chunks"] and c["max_cuts"] <= max_share * c["chunks"], c
    return want


def check_hashes(oracle, img, got, m):
    for c in range(m):
        o, n = int(got["chunk_off"][c]), int(got["chunk_len"][c])
        d = bytes(got["digests"][c])
        assert d.hex() == oracle.hash(img[o:o + n].tobytes()), (c, o, n)
        assert int(got["keys"][c]) == int.from_bytes(d[:8], "big"), c


def check(got, want, oracle=None, img=None):
    assert got["counts"] == want["counts"]
    m = want["counts"]["chunks"]
    assert (got["file_chunks"] == want["file_chunks"]).all()
    for name in ARRAYS[1:]:
        assert got[name].size >= m and (got[name][:m] == want[name]).all(), name
    if oracle is not None:
        check_hashes(oracle, img, got, m)


def host_call(eng, img, offs, lens, params=P):
    fc, off, ln, fl, keys, dig, counts = eng.chunk_messages(img, offs, lens, params)
    return {"file_chunks": fc, "chunk_off": off, "chunk_len": ln, "chunk_file": fl, "keys": keys, "digests": dig,
            "counts": counts}


FILL = 0xFE


def device_call(eng, img, offs, lens, params=P, outputs=(True,) * 7, plan=None, stream=0):
    """sdcas_dev_chunk over guarded buffers of exactly the planned capacities;
    outputs: which of file_chunks, chunk_off, chunk_len, chunk_file, keys,
    digests, counts are passed. Asserts the guards and that nothing past
    `chunks` (and no null output) was written."""
    n = len(lens)
    mc, ms = plan or eng.chunk_plan(lens, params)
    blob = guarded_from(img)
    d_offs, d_lens = guarded_from(np.asarray(offs, np.uint64), align=8), guarded_from(np.asarray(lens, np.uint64), align=8)
    sizes = (8 * (n + 1), 8 * mc, 8 * mc, 4 * mc, 8 * mc, 32 * mc, 48)
    aligns = (8, 8, 8, 4, 8, 16, 8)
    outs = [Guarded(s, align=a, fill=FILL) for s, a in zip(sizes, aligns)]
    torch.cuda.synchronize()
    ptr = [o.ptr if outputs[j] else 0 for j, o in enumerate(outs)]
    eng.dev_chunk(blob.ptr, d_offs.ptr if n else 0, d_lens.ptr if n else 0, n, mc, ms, params, *ptr, stream=stream)
    eng.dev_sync(stream)
    torch.cuda.synchronize()
    for g in [blob, d_offs, d_lens] + outs:
        assert g.check() == []
    assert blob.unchanged() and d_offs.unchanged() and d_lens.unchanged()
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {j} was written"
    got = {"file_chunks": outs[0].download(np.uint64), "chunk_off": outs[1].download(np.uint64),
           "chunk_len": outs[2].download(np.uint64), "chunk_file": outs[3].download(np.uint32),
           "keys": outs[4].download(np.uint64), "digests": outs[5].download(np.uint8).reshape(-1, 32),
           "counts": dict(zip(COUNTS, (int(x) for x in outs[6].download(np.uint64))))}
    if outputs[6]:
        m = got["counts"]["chunks"]
        per = (None, 8, 8, 4, 8, 32)
        for j in range(1, 6):
            if outputs[j]:
                assert outs[j].untouched(per[j] * m), f"output {j} was written past its {m} chunks"
    return got


def both(eng, oracle, files, params=P, max_share=None, starts=None):
    img, offs, lens = lay_out(files, starts)
    want = reference(files, offs, params, max_share)
    check(host_call(eng, img, offs, lens, params), want, oracle, img)
    check(device_call(eng, img, offs, lens, params), want, oracle, img)
    return want


# ---- boundary cases --------------------------------------------------------------------

def test_no_files(eng):
    fc, off, ln, fl, keys, dig, counts = eng.chunk_messages(np.zeros(0, np.uint8), [], [], P)
    assert fc.tolist() == [0] and off.size == 0 and counts == dict.fromkeys(COUNTS, 0)
    got = device_call(eng, np.zeros(64, np.uint8), [], [], P)
    assert got["counts"] == dict.fromkeys(COUNTS, 0) and got["file_chunks"][0] == 0


def test_small_lengths_and_empty_files(eng, oracle):
    rng = np.random.default_rng(1)
    lens = [0, 1, 31, 0, 32, 33, 63, 64, 65, 0, 1024, 0]
    files = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    want = both(eng, oracle, files, P, 0.02)
    assert want["counts"]["files"] == len(lens) and want["counts"]["end_chunks"] == len(lens) - 4
    both(eng, oracle, [np.zeros(0, np.uint8)] * 3)  # empty files alone: no chunk at all


def test_the_other_branch_max_cuts_and_dense_candidates(eng, oracle):
    files = [np.zeros(1025, np.uint8), np.full(5000, 138, np.uint8), np.zeros(100000, np.uint8),
             content("pattern251", 0, 4096)]
    want = both(eng, oracle, files)
    fc = want["file_chunks"]
    assert np.diff(fc).tolist() == [2, 20, 98, 14]
    assert want["chunk_len"][:2].tolist() == [1024, 1] and want["counts"]["max_cuts"] == 1 + 97
    ends = np.cumsum(want["chunk_len"][int(fc[3]):])
    assert ends.tolist() == [263, 560, 835, 1205, 1487, 1769, 2066, 2341, 2711, 2993, 3275, 3572, 3847, 4096]


def test_pinned_synthetic_vectors(eng, oracle):
    x = content("synth", 0, 20000, content_key(0x5D, 1))
    want = both(eng, oracle, [x], P, 0.02)
    assert want["counts"]["chunks"] == 67
    assert np.cumsum(want["chunk_len"])[:6].tolist() == [542, 799, 1059, 1209, 1594, 1958]
    want = both(eng, oracle, [x], (1024, 12, 16384))
    assert np.cumsum(want["chunk_len"]).tolist() == [1209, 5448, 7028, 10324, 12777, 14628, 20000]


# ---- nothing depends on where a tile or a strip begins ------------------------------------

def test_one_content_at_41_offsets_gives_41_identical_cut_lists(eng):
    x = synth(50000, 41)
    starts = [2 * TILE * j + 16 * j for j in range(41)]  # 16 j past a multiple of the tile (and of the strip)
    files = [x] * 41
    img, offs, lens = lay_out(files, starts)
    want = reference(files, offs, P, 0.02)
    for got in (host_call(eng, img, offs, lens), device_call(eng, img, offs, lens)):
        check(got, want)
        fc = got["file_chunks"]
        first = got["chunk_len"][:int(fc[1])]
        for j in range(41):
            assert (got["chunk_len"][int(fc[j]):int(fc[j + 1])] == first).all(), j
            assert (got["digests"][int(fc[j]):int(fc[j + 1])] == got["digests"][:int(fc[1])]).all(), j


def test_lengths_around_the_gear_tile_and_strip(eng, oracle):
    lens = [T + d for T in (STRIP, TILE) for d in (-1, 0, 1)] + [2 * STRIP + 17, 2 * TILE + 17]
    files = [synth(n, 1000 + i) for i, n in enumerate(lens)]
    both(eng, oracle, files, P, 0.02)
    # a content whose candidates are dense, so that a seam would show at every position
    both(eng, oracle, [np.full(n, 138, np.uint8) for n in (TILE - 1, TILE + 1, 2 * TILE + 17)])


# ---- many files ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    """1 000 files of 0..20 000 bytes, a third of them copies or one-byte
    inserted variants of earlier ones; the reference is computed once"""
    rng = np.random.default_rng(1000)
    files = []
    for i in range(1000):
        kind = rng.integers(0, 6) if i else 0
        if kind == 4:
            files.append(files[int(rng.integers(0, i))].copy())
        elif kind == 5:
            src = files[int(rng.integers(0, i))]
            at = int(rng.integers(0, src.size + 1))
            files.append(np.concatenate([src[:at], rng.integers(0, 256, 1, dtype=np.uint8), src[at:]]))
        else:
            files.append(synth(int(rng.integers(0, 20001)), i))
    img, offs, lens = lay_out(files)
    return files, img, offs, lens, reference(files, offs, P, 0.02)


def test_a_thousand_files(eng, oracle, corpus):
    files, img, offs, lens, want = corpus
    assert want["counts"]["chunks"] > 20000
    check(host_call(eng, img, offs, lens), want, oracle, img)
    check(device_call(eng, img, offs, lens), want)


def test_many_small_hash_batches_give_the_same(eng, corpus, monkeypatch):
    files, img, offs, lens, want = corpus
    plain = device_call(eng, img, offs, lens)
    monkeypatch.setenv("SDCAS_CHUNK_PACK_BYTES", "4096")
    small = device_call(eng, img, offs, lens)
    check(small, want)
    m = want["counts"]["chunks"]
    assert (small["digests"][:m] == plain["digests"][:m]).all() and (small["keys"][:m] == plain["keys"][:m]).all()


def test_a_smaller_call_after_a_larger_one_and_null_outputs(eng, oracle, corpus):
    files, img, offs, lens, want = corpus
    device_call(eng, img, offs, lens)  # leaves the workspace dirty
    few = files[10:30]
    img2, offs2, lens2 = lay_out(few)
    want2 = reference(few, offs2, P, 0.02)
    check(device_call(eng, img2, offs2, lens2), want2, oracle, img2)
    full = device_call(eng, img2, offs2, lens2)
    m = want2["counts"]["chunks"]
    for j in range(7):
        got = device_call(eng, img2, offs2, lens2, outputs=tuple(k != j for k in range(7)))
        for k, name in enumerate(ARRAYS + ("keys", "digests")):
            if k != j:
                size = len(lens2) + 1 if k == 0 else m
                assert (got[name][:size] == full[name][:size]).all(), (j, name)
        if j != 6:
            assert got["counts"] == want2["counts"]
    # no keys and no digests: the call never plans a hash batch
    got = device_call(eng, img2, offs2, lens2, outputs=(True, True, True, True, False, False, True))
    check({**got, "digests": None, "keys": None}, want2)


def test_one_8_mib_file_at_the_default_parameters(eng, oracle):
    x = synth(8 << 20, 8)
    img, offs, lens = lay_out([x])
    want = reference([x], offs, R.DEFAULT_PARAMS, 0.02)
    assert 500 < want["counts"]["chunks"] < 2500
    check(device_call(eng, img, offs, lens, R.DEFAULT_PARAMS), want, oracle, img)


# ---- the memory contract ---------------------------------------------------------------------

def test_poisoned_gaps_and_a_file_at_offset_zero(eng, oracle):
    files = [synth(n, 70 + i) for i, n in enumerate((5000, 1, 33000, 777, 0, 4096))]
    starts, cur = [], 0  # the first file at blob offset 0
    for f in files:
        starts.append(cur)
        cur += (len(f) + 64 + 15) // 16 * 16
    img, offs, lens = lay_out(files, starts)
    assert offs[0] == 0
    want = reference(files, offs, P, 0.02)
    got = device_call(eng, img, offs, lens)
    check(got, want, oracle, img)
    # another poison in every gap: the same cuts and digests
    img2 = img.copy()
    gap = np.ones(img.size, bool)
    for s, f in zip(starts, files):
        gap[s:s + len(f)] = False
    img2[gap] = 0x00
    got2 = device_call(eng, img2, offs, lens)
    check(got2, want, oracle, img2)
    m = want["counts"]["chunks"]
    assert (got2["digests"][:m] == got["digests"][:m]).all()


def test_misaligned_arguments_are_refused_before_anything_runs(eng):
    x = synth(5000, 3)
    img, offs, lens = lay_out([x])
    blob = guarded_from(img)
    d_offs, d_lens = guarded_from(offs, align=8), guarded_from(lens, align=8)
    mc, ms = eng.chunk_plan(lens, P)
    out = Guarded(64 * mc + 64, align=16, fill=FILL)
    for kw in ({"blob": blob.ptr + 8}, {"digests": out.ptr + 8}, {"keys": out.ptr + 4}, {"chunk_file": out.ptr + 2},
               {"counts": out.ptr + 4}):
        args = {"blob": blob.ptr, **kw}
        with pytest.raises(N.SdcasError) as e:
            eng.dev_chunk(args.pop("blob"), d_offs.ptr, d_lens.ptr, 1, mc, ms, P, **args)
        assert e.value.code == N.SDCAS_E_INVALID
    with pytest.raises(N.SdcasError) as e:
        eng.dev_chunk(blob.ptr, d_offs.ptr, d_lens.ptr, 1, mc, ms, (31, 8, 1024), counts=out.ptr)
    assert e.value.code == N.SDCAS_E_INVALID
    torch.cuda.synchronize()
    assert out.untouched() and out.check() == []
