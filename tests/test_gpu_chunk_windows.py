"""Chunk windows on the GPU (sdcas_dev_chunk_windows / sdcas_chunk_windows,
csrc/cdc.hip): every array, `consumed` and all six counts against
tests/_cdc_win_ref.py and, for final windows, against sdcas_dev_chunk itself;
every chunk digest against the oracle's BLAKE3 of the chunk's bytes and every
key against the digest. The device call runs over guarded buffers of exactly
the planned capacities. The segment length is set to 2112 bytes, so that
windows of a few KiB take the segmented cut pass."""
import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests import _cdc_ref as R
from tests import _cdc_win_ref as W
from tests import test_gpu_chunks as C
from tests._guarded import Guarded, guarded_from

pytestmark = pytest.mark.gpu

P = R.TEST_PARAMS
SEG = 2112
COUNTS, ARRAYS, FILL = C.COUNTS, C.ARRAYS, C.FILL
NAMES = ARRAYS + ("keys", "digests", "consumed")


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(autouse=True)
def small_segments(monkeypatch):
    monkeypatch.setenv("SDCAS_CHUNK_SEG_BYTES", str(SEG))


def device_call(eng, img, offs, lens, final=None, params=P, outputs=(True,) * 8, stream=0):
    """sdcas_dev_chunk_windows over guarded buffers of exactly the planned
    capacities; outputs: which of file_chunks, chunk_off, chunk_len,
    chunk_file, keys, digests, consumed, counts are passed; final: None for a
    null d_final. Asserts the guards, that the inputs are unchanged and that
    nothing past `chunks` (and no null output) was written."""
    n = len(lens)
    mc, ms = eng.chunk_plan(lens, params)
    blob = guarded_from(img)
    d_offs, d_lens = guarded_from(np.asarray(offs, np.uint64), align=8), guarded_from(np.asarray(lens, np.uint64), align=8)
    d_final = None if final is None else guarded_from(np.asarray(final, np.uint8), align=1)
    sizes = (8 * (n + 1), 8 * mc, 8 * mc, 4 * mc, 8 * mc, 32 * mc, 8 * n, 48)
    aligns = (8, 8, 8, 4, 8, 16, 8, 8)
    outs = [Guarded(s, align=a, fill=FILL) for s, a in zip(sizes, aligns)]
    torch.cuda.synchronize()
    ptr = [o.ptr if outputs[j] else 0 for j, o in enumerate(outs)]
    eng.dev_chunk_windows(blob.ptr, d_offs.ptr if n else 0, d_lens.ptr if n else 0,
                          d_final.ptr if d_final is not None and n else 0, n, mc, ms, params, *ptr, stream=stream)
    eng.dev_sync(stream)
    torch.cuda.synchronize()
    ins = [blob, d_offs, d_lens] + ([d_final] if d_final is not None else [])
    for g in ins + outs:
        assert g.check() == []
    assert all(g.unchanged() for g in ins)
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {j} was written"
    got = {"file_chunks": outs[0].download(np.uint64), "chunk_off": outs[1].download(np.uint64),
           "chunk_len": outs[2].download(np.uint64), "chunk_file": outs[3].download(np.uint32),
           "keys": outs[4].download(np.uint64), "digests": outs[5].download(np.uint8).reshape(-1, 32),
           "consumed": outs[6].download(np.uint64),
           "counts": dict(zip(COUNTS, (int(x) for x in outs[7].download(np.uint64))))}
    if outputs[7]:
        m = got["counts"]["chunks"]
        per = (None, 8, 8, 4, 8, 32)
        for j in range(1, 6):
            if outputs[j]:
                assert outs[j].untouched(per[j] * m), f"output {j} was written past its {m} chunks"
    return got


def check(got, want, oracle=None, img=None):
    C.check(got, want, oracle, img)
    assert (got["consumed"] == want["consumed"]).all()


def rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


RANDOM_LENS = (0, 1, 63, 64, 65, 1024, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1, 5 * SEG + 17, 40001)


@pytest.fixture(scope="module")
def corpus(oracle):
    """the files of the all-final and the streamed tests, their whole-file
    reference and the oracle's digest of every reference chunk, computed once"""
    files = [rand(n, 100 + i) for i, n in enumerate(RANDOM_LENS)]
    files += [np.full(40000, 138, np.uint8), np.zeros(40000, np.uint8), (np.arange(40000) % 97).astype(np.uint8)]
    img, offs, lens = C.lay_out(files)
    nr = len(RANDOM_LENS)
    # the random files themselves keep the MAX cuts rare: the input exercises the hash cuts
    C.reference(files[:nr], offs[:nr], P, 0.02)
    want = R.chunk_files(files, offs, P)
    want["consumed"] = lens.copy()
    digests = [bytes.fromhex(oracle.hash(img[int(o):int(o) + int(n)].tobytes()))
               for o, n in zip(want["chunk_off"], want["chunk_len"])]
    return files, img, offs, lens, want, np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32)


def check_digests(got, m, digests):
    assert (got["digests"][:m] == digests[:m]).all()
    keys = [int.from_bytes(bytes(d[:8]), "big") for d in digests[:m]]
    assert got["keys"][:m].tolist() == keys


# ---- all windows final: sdcas_dev_chunk's results ------------------------------------------

@pytest.mark.parametrize("flags", ["null", "ones"])
def test_all_final_equals_the_reference_and_dev_chunk(eng, corpus, flags):
    assert eng.chunk_seg_bytes(P) == SEG
    files, img, offs, lens, want, digests = corpus
    final = None if flags == "null" else np.ones(len(files), np.uint8)
    got = device_call(eng, img, offs, lens, final)
    check(got, want)
    m = want["counts"]["chunks"]
    check_digests(got, m, digests)
    plain = C.device_call(eng, img, offs, lens)
    assert got["counts"] == plain["counts"] and (got["file_chunks"] == plain["file_chunks"]).all()
    for name in ARRAYS[1:] + ("keys", "digests"):
        assert (got[name][:m] == plain[name][:m]).all(), name


def test_the_host_call_gives_the_same(eng, corpus):
    files, img, offs, lens, want, digests = corpus
    fc, off, ln, fl, keys, dig, counts, consumed = eng.chunk_windows(img, offs, lens, None, P)
    got = {"file_chunks": fc, "chunk_off": off, "chunk_len": ln, "chunk_file": fl, "keys": keys, "digests": dig,
           "counts": counts, "consumed": consumed}
    check(got, want)
    check_digests(got, want["counts"]["chunks"], digests)


# ---- a file window by window -------------------------------------------------------------------

@pytest.mark.parametrize("window", [1024, 1025, 2048, 4097, 3 * SEG])
def test_streamed_windows_give_the_whole_file_chunks(eng, corpus, window):
    """every file on its own sequence of windows, each restarting at the
    consumed of the one before; one call holds the current window of every
    file that is not finished"""
    files, img, offs, lens, want, digests = corpus
    nf = len(files)
    pos, size, done = [0] * nf, [window] * nf, [False] * nf
    ends, digs, keys = [[] for _ in files], [[] for _ in files], [[] for _ in files]
    total = dict.fromkeys(COUNTS, 0)
    rounds = 0
    while not all(done):
        live = [i for i in range(nf) if not done[i]]
        wins = [files[i][pos[i]:pos[i] + size[i]] for i in live]
        final = [pos[i] + w.size >= files[i].size for i, w in zip(live, wins)]
        wimg, woffs, wlens = C.lay_out(wins)
        got = device_call(eng, wimg, woffs, wlens, final)
        check(got, W.window_files(wins, woffs, final, P))
        fc = got["file_chunks"]
        for k, i in enumerate(live):
            a, b = int(fc[k]), int(fc[k + 1])
            ends[i] += (got["chunk_off"][a:b] - woffs[k] + got["chunk_len"][a:b] + np.uint64(pos[i])).tolist()
            digs[i] += [bytes(d) for d in got["digests"][a:b]]
            keys[i] += got["keys"][a:b].tolist()
            used = int(got["consumed"][k])
            assert final[k] or used >= wins[k].size - P[2] + 1 or used == 0
            if final[k]:
                done[i] = True
            elif used == 0:
                size[i] *= 2
            else:
                pos[i], size[i] = pos[i] + used, window
        for name in COUNTS:
            total[name] += got["counts"][name]
        rounds += 1
        assert rounds < 400
    assert total == want["counts"]
    wfc = want["file_chunks"]
    for i in range(nf):
        a, b = int(wfc[i]), int(wfc[i + 1])
        assert ends[i] == (want["chunk_off"][a:b] - offs[i] + want["chunk_len"][a:b]).tolist(), i
        assert digs[i] == [bytes(d) for d in digests[a:b]], i
        assert keys[i] == [int.from_bytes(d[:8], "big") for d in digs[i]], i


# ---- the stop rule at its edges --------------------------------------------------------------------

def test_the_stop_rule_at_its_edges(eng, oracle):
    x = rand(5000, 7)
    ends, kinds = R.cuts(x, P)
    nth = int(np.flatnonzero(kinds == R.KIND_HASH)[2])
    at_cut = int(ends[nth])  # a window that ends exactly at a hash cut: e == W
    wins = [np.zeros(1023, np.uint8), np.zeros(1024, np.uint8), x[:at_cut], rand(63, 8), np.zeros(0, np.uint8)]
    img, offs, lens = C.lay_out(wins)
    final = [0] * len(wins)
    want = W.window_files(wins, offs, final, P)
    got = device_call(eng, img, offs, lens, final)
    check(got, want, oracle, img)
    assert got["consumed"].tolist() == [0, 1024, at_cut, 0, 0]
    assert np.diff(got["file_chunks"]).tolist() == [0, 1, nth + 1, 0, 0]
    c = got["counts"]
    assert (c["files"], c["end_chunks"], c["max_cuts"], c["hash_cuts"]) == (0, 0, 1 + nth - 2, 3)
    assert c["total_bytes"] == 1024 + at_cut
    # each alone gives the same
    for k, w in enumerate(wins):
        i1, o1, l1 = C.lay_out([w])
        one = device_call(eng, i1, o1, l1, [0])
        assert int(one["consumed"][0]) == int(want["consumed"][k]), k
        assert one["counts"]["chunks"] == int(want["file_chunks"][k + 1] - want["file_chunks"][k]), k


# ---- final and not final in one call; the memory contract -------------------------------------------

def mixed():
    wins = [rand(5 * SEG + 17, 21), rand(3000, 22), rand(2 * SEG, 23), np.full(3 * SEG + 5, 138, np.uint8),
            rand(1, 24), np.zeros(0, np.uint8), rand(2 * SEG + 700, 25)]
    final = [0, 1, 1, 0, 0, 1, 0]
    starts, cur = [], 16  # every window at an odd multiple of 16
    for w in wins:
        starts.append(cur)
        cur += (w.size + 64 + 31) // 32 * 32
    assert all(s % 32 == 16 for s in starts)
    img, offs, lens = C.lay_out(wins, starts)
    return wins, final, img, offs, lens, W.window_files(wins, offs, final, P)


def test_mixed_final_flags_in_one_call(eng, oracle):
    wins, final, img, offs, lens, want = mixed()
    got = device_call(eng, img, offs, lens, final)
    check(got, want, oracle, img)
    assert want["counts"]["files"] == 3 and want["counts"]["end_chunks"] == 2
    # another poison between the windows: the same results
    img2 = img.copy()
    gap = np.ones(img.size, bool)
    for s, w in zip(offs, wins):
        gap[int(s):int(s) + w.size] = False
    img2[gap] = 0x00
    got2 = device_call(eng, img2, offs, lens, final)
    check(got2, want, oracle, img2)
    m = want["counts"]["chunks"]
    assert (got2["digests"][:m] == got["digests"][:m]).all()


def test_each_output_null_in_turn_and_no_hashes_without_a_wait(eng):
    wins, final, img, offs, lens, want = mixed()
    full = device_call(eng, img, offs, lens, final)
    m = want["counts"]["chunks"]
    for j in range(8):
        got = device_call(eng, img, offs, lens, final, outputs=tuple(k != j for k in range(8)))
        for k, name in enumerate(NAMES):
            if k != j:
                size = len(lens) + 1 if k == 0 else len(lens) if k == 6 else m
                assert (got[name][:size] == full[name][:size]).all(), (j, name)
        if j != 7:
            assert got["counts"] == want["counts"]
    # no keys and no digests: the call never plans a hash batch, and never waits
    got = device_call(eng, img, offs, lens, final, outputs=(True, True, True, True, False, False, True, True))
    check({**got, "digests": None, "keys": None}, want)


def test_misaligned_arguments_are_refused_before_anything_runs(eng):
    x = rand(5000, 3)
    img, offs, lens = C.lay_out([x])
    blob = guarded_from(img)
    d_offs, d_lens = guarded_from(offs, align=8), guarded_from(lens, align=8)
    d_final = guarded_from(np.zeros(1, np.uint8), align=1)
    mc, ms = eng.chunk_plan(lens, P)
    out = Guarded(64 * mc + 64, align=16, fill=FILL)
    for kw in ({"blob": blob.ptr + 8}, {"digests": out.ptr + 8}, {"keys": out.ptr + 4}, {"chunk_file": out.ptr + 2},
               {"consumed": out.ptr + 4}, {"counts": out.ptr + 4}, {"file_chunks": out.ptr + 4}):
        args = {"blob": blob.ptr, **kw}
        with pytest.raises(N.SdcasError) as e:
            eng.dev_chunk_windows(args.pop("blob"), d_offs.ptr, d_lens.ptr, d_final.ptr, 1, mc, ms, P, **args)
        assert e.value.code == N.SDCAS_E_INVALID
    with pytest.raises(N.SdcasError) as e:
        eng.dev_chunk_windows(blob.ptr, d_offs.ptr, d_lens.ptr, d_final.ptr, 1, mc, ms, (31, 8, 1024), counts=out.ptr)
    assert e.value.code == N.SDCAS_E_INVALID
    torch.cuda.synchronize()
    assert out.untouched() and out.check() == []
    # d_final at any address
    fin = guarded_from(np.zeros(8, np.uint8), align=8)
    cons = Guarded(8, align=8, fill=FILL)
    eng.dev_chunk_windows(blob.ptr, d_offs.ptr, d_lens.ptr, fin.ptr + 3, 1, mc, ms, P, consumed=cons.ptr)
    eng.dev_sync(0)
    assert int(cons.download(np.uint64)[0]) == W.window_cuts(x, P, False)[2]


def test_no_windows(eng):
    got = device_call(eng, np.zeros(64, np.uint8), [], [], [])
    assert got["counts"] == dict.fromkeys(COUNTS, 0) and got["file_chunks"][0] == 0
    fc, off, ln, fl, keys, dig, counts, consumed = eng.chunk_windows(np.zeros(0, np.uint8), [], [], None, P)
    assert fc.tolist() == [0] and off.size == 0 and consumed.size == 0 and counts == dict.fromkeys(COUNTS, 0)


# ---- the default parameters and the default segment -------------------------------------------------

def test_a_3_mib_file_at_the_default_parameters(eng, oracle, monkeypatch):
    monkeypatch.delenv("SDCAS_CHUNK_SEG_BYTES")
    assert eng.chunk_seg_bytes() == 1 << 20
    DP = R.DEFAULT_PARAMS
    x = rand((3 << 20) + 17, 31)
    img, offs, lens = C.lay_out([x])
    want = C.reference([x], offs, DP, 0.02)
    want["consumed"] = lens.copy()
    got = device_call(eng, img, offs, lens, [1], DP)  # four segments
    check(got, want, oracle, img)
    m = want["counts"]["chunks"]
    whole_ends = (want["chunk_off"] - offs[0] + want["chunk_len"]).tolist()
    # windows of 1 MiB + 1, each below two segments
    pos, ends, digs = 0, [], []
    total = dict.fromkeys(COUNTS, 0)
    while True:
        w = x[pos:pos + (1 << 20) + 1]
        final = pos + w.size >= x.size
        wimg, woffs, wlens = C.lay_out([w])
        one = device_call(eng, wimg, woffs, wlens, [final], DP)
        k = one["counts"]["chunks"]
        ends += (one["chunk_off"][:k] - woffs[0] + one["chunk_len"][:k] + np.uint64(pos)).tolist()
        digs += [bytes(d) for d in one["digests"][:k]]
        for name in COUNTS:
            total[name] += one["counts"][name]
        if final:
            break
        assert int(one["consumed"][0]) > 0
        pos += int(one["consumed"][0])
    assert ends == whole_ends and total == want["counts"]
    assert digs == [bytes(d) for d in got["digests"][:m]]
