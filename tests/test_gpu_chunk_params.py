"""The chunking kernels (csrc/cdc.hip) over the width of the parameters the
C ABI accepts, at exact thresholds and at the bounds of their outputs: the
inputs of tests/_cdc_param_cases.py (tests/test_cdc_param_cases.py shows
without a GPU that each meets its condition) through sdcas_chunk_messages,
sdcas_dev_chunk and sdcas_dev_chunk_windows, the last at the smallest segment
the parameters allow. Every array, file_chunks and all six counts against
tests/_cdc_ref.py, every digest against the oracle's BLAKE3 of the chunk's
bytes, every key against its digest. The device calls run over guarded
buffers of exactly the planned capacities (tests/test_gpu_chunks.py,
tests/test_gpu_chunk_windows.py), which the dense cases fill to the last
element."""
import numpy as np
import pytest

from tests import _cdc_param_cases as K
from tests import _cdc_ref as R
from tests import _cdc_win_ref as W
from tests import test_gpu_chunk_windows as WN
from tests import test_gpu_chunks as C

pytestmark = pytest.mark.gpu

COUNTS, ARRAYS = C.COUNTS, C.ARRAYS

BUILDERS = {"sweep": K.sweep, "planted": K.planted, "dense": K.dense, "dense_mixed": K.dense_mixed}
CASES = ([("sweep", p) for p in K.SWEEP_PARAMS] + [("planted", p) for p in K.PLANTED_PARAMS]
         + [("dense",), ("dense_mixed",)])
SHORT_CHUNKS = [("sweep", (32, 6, 65)), ("dense",), ("dense_mixed",)]  # chunks of 32..65 bytes, thousands of them


def case_id(case):
    return case[0] + ("" if len(case) == 1 else "-%d-%d-%d" % case[1])


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


_loaded, _plain = {}, {}


def load(case, oracle):
    """the case laid out in a blob, its reference and the oracle's digest of
    every reference chunk, computed once"""
    if case not in _loaded:
        files, params, expect = BUILDERS[case[0]](*case[1:])
        img, offs, lens = C.lay_out(files)
        want = R.chunk_files(files, offs, params, known=expect["cuts"])
        for name in ("chunks", "hash_cuts", "max_cuts", "end_chunks"):
            assert want["counts"][name] == expect["counts"][name]
        assert want["counts"]["total_bytes"] == int(lens.sum())
        want["consumed"] = lens.copy()
        digests = [bytes.fromhex(oracle.hash(img[int(o):int(o) + int(n)].tobytes()))
                   for o, n in zip(want["chunk_off"], want["chunk_len"])]
        digests = np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32)
        _loaded[case] = (files, params, img, offs, lens, want, digests)
    return _loaded[case]


def plain_call(eng, case, oracle):
    """sdcas_dev_chunk's results for the case, computed once"""
    if case not in _plain:
        files, params, img, offs, lens, want, digests = load(case, oracle)
        _plain[case] = C.device_call(eng, img, offs, lens, params)
    return _plain[case]


def check(got, want, digests):
    C.check(got, want)
    WN.check_digests(got, want["counts"]["chunks"], digests)


# ---- whole files ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_whole_files_through_the_host_and_the_device_call(eng, oracle, case):
    files, params, img, offs, lens, want, digests = load(case, oracle)
    mc, _ = eng.chunk_plan(lens, params)
    assert mc == R.chunk_plan(lens, params)[0]
    if case[0] == "dense":
        assert want["counts"]["chunks"] == mc  # every output is filled to its last element
    check(C.host_call(eng, img, offs, lens, params), want, digests)
    check(plain_call(eng, case, oracle), want, digests)


@pytest.mark.parametrize("case", SHORT_CHUNKS, ids=case_id)
def test_short_chunks_across_many_hash_batches(eng, oracle, case, monkeypatch):
    files, params, img, offs, lens, want, digests = load(case, oracle)
    assert want["counts"]["chunks"] > 300 and int(want["chunk_len"].max()) <= 65
    assert int(want["chunk_len"].sum()) > 4 * 4096  # (a batch holds 4096 packed bytes)
    monkeypatch.setenv("SDCAS_CHUNK_PACK_BYTES", "4096")
    check(C.device_call(eng, img, offs, lens, params), want, digests)


# ---- the same files as final windows, at the smallest segment --------------------------------------

@pytest.fixture
def smallest_segments(monkeypatch):
    monkeypatch.setenv("SDCAS_CHUNK_SEG_BYTES", "1")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_final_windows_at_the_smallest_segment(eng, oracle, case, smallest_segments):
    files, params, img, offs, lens, want, digests = load(case, oracle)
    seg = eng.chunk_seg_bytes(params)
    assert seg == (2 * params[2] + 63) // 64 * 64 == K.seg_bytes(params)
    if params[1] < 24:  # (a file of two segments at avg_bits 24 is 64 MiB: that one takes the one-wave pass)
        assert int(lens.max()) >= 2 * seg
    if case[0] == "planted" and params[1] < 24:
        assert int(lens.min()) >= 2 * seg
    got = WN.device_call(eng, img, offs, lens, None, params)
    WN.check(got, want)
    m = want["counts"]["chunks"]
    WN.check_digests(got, m, digests)
    plain = plain_call(eng, case, oracle)
    assert got["counts"] == plain["counts"] and (got["file_chunks"] == plain["file_chunks"]).all()
    for name in ARRAYS[1:] + ("keys", "digests"):
        assert (got[name][:m] == plain[name][:m]).all(), name


# ---- files window by window -------------------------------------------------------------------------

def window_sizes(params):
    return (params[0], params[0] + 1, params[2], params[2] + 1, 2 * K.seg_bytes(params) + 1)


STREAMED = [(p, k) for p in K.STREAMED_PARAMS for k in range(5)]


@pytest.mark.parametrize("params,which", STREAMED, ids=lambda v: "%d-%d-%d" % v if isinstance(v, tuple) else "w%d" % v)
def test_streamed_windows_give_the_whole_file_chunks(eng, oracle, params, which, smallest_segments):
    """tests/test_gpu_chunk_windows.py's loop at other parameters: every file on
    its own sequence of windows, each restarting at the consumed of the one
    before, a window that consumed nothing doubled"""
    files, P, expect = K.streamed(params)
    window = window_sizes(P)[which]
    assert eng.chunk_seg_bytes(P) == K.seg_bytes(P)
    img, offs, lens = C.lay_out(files)
    want = R.chunk_files(files, offs, P, known=expect["cuts"])
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
        got = WN.device_call(eng, wimg, woffs, wlens, final, P)
        WN.check(got, W.window_files(wins, woffs, final, P))  # consumed per call among it
        fc = got["file_chunks"]
        for k, i in enumerate(live):
            a, b = int(fc[k]), int(fc[k + 1])
            ends[i] += (got["chunk_off"][a:b] - woffs[k] + got["chunk_len"][a:b] + np.uint64(pos[i])).tolist()
            digs[i] += [bytes(d) for d in got["digests"][a:b]]
            keys[i] += got["keys"][a:b].tolist()
            used = int(got["consumed"][k])
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
        for c in range(a, b):
            o, n = int(want["chunk_off"][c]), int(want["chunk_len"][c])
            assert digs[i][c - a].hex() == oracle.hash(img[o:o + n].tobytes()), (i, c)
        assert keys[i] == [int.from_bytes(d[:8], "big") for d in digs[i]], i


@pytest.mark.parametrize("params", K.STREAMED_PARAMS, ids=lambda p: "%d-%d-%d" % p)
def test_windows_of_min_len_and_one_byte_less(eng, oracle, params, smallest_segments):
    """a window that is not final: min_len - 1 bytes decide nothing, min_len
    bytes decide a cut only where the last position is a STRICT candidate"""
    mn, ab, mx = params
    rng = np.random.default_rng([0xE, mn, ab, mx])
    strict = np.concatenate([rng.integers(0, 256, mn - 32, dtype=np.uint8), R.window_with_hash(0, rng)])
    loose = np.concatenate([rng.integers(0, 256, mn - 32, dtype=np.uint8),
                            R.window_with_hash(K.limits(params)[0], rng)])  # LOOSE only: no cut below avg
    wins = [strict[1:], strict, loose, np.zeros(mn - 1, np.uint8), np.zeros(mn, np.uint8), np.zeros(mx - 1, np.uint8),
            np.zeros(mx, np.uint8)]
    final = [0] * len(wins)
    img, offs, lens = C.lay_out(wins)
    want = W.window_files(wins, offs, final, params)
    assert want["consumed"].tolist() == [0, mn, 0, 0, 0, 0, mx]
    assert want["kinds"].tolist() == [R.KIND_HASH, R.KIND_MAX]
    got = WN.device_call(eng, img, offs, lens, final, params)
    WN.check(got, want, oracle, img)
    assert got["counts"]["files"] == 0 and got["counts"]["end_chunks"] == 0
    # the same windows as final ones: each is a whole file
    whole = W.window_files(wins, offs, [1] * len(wins), params)
    assert whole["consumed"].tolist() == lens.tolist()
    WN.check(WN.device_call(eng, img, offs, lens, [1] * len(wins), params), whole, oracle, img)
