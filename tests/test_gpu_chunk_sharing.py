"""The sharing pass over content-defined chunks on the GPU (sdcas_chunk_sharing /
sdcas_dev_chunk_sharing, csrc/cdc.hip) against the dict-based reference of
tests/_cdc_ref.py, through the host call and through the device call with
guarded buffers; then Engine.similar_files on real files and the three device
calls on one stream."""
import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests import _cdc_ref as R
from tests._guarded import Guarded, guarded_from
from tests._oracle import content, content_key

pytestmark = pytest.mark.gpu

COUNTS = ("files", "chunks", "distinct_chunks", "total_bytes", "stored_bytes", "files_with_peer")
NAMES = ("new_bytes", "self_bytes", "other_bytes", "peer", "peer_bytes")
FILL = 0xFE


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def host_call(eng, chunk_file, chunk_len, rep, n_files):
    new, own, other, peer, peer_bytes, counts = eng.chunk_sharing(chunk_file, chunk_len, rep, n_files)
    return {"new_bytes": new, "self_bytes": own, "other_bytes": other, "peer": peer, "peer_bytes": peer_bytes,
            "counts": counts}


def device_call(eng, chunk_file, chunk_len, rep, n_files, outputs=(True,) * 6, stream=0):
    """sdcas_dev_chunk_sharing over guarded buffers; outputs: which of the five
    arrays and the counts are passed"""
    m = len(chunk_file)
    ins = [guarded_from(np.asarray(chunk_file, np.uint32), align=4), guarded_from(np.asarray(chunk_len, np.uint64), align=8),
           guarded_from(np.asarray(rep, np.int64), align=8)]
    outs = [Guarded(8 * n_files, align=8, fill=FILL) for _ in range(5)] + [Guarded(48, align=8, fill=FILL)]
    torch.cuda.synchronize()
    ptr = [o.ptr if outputs[j] else 0 for j, o in enumerate(outs)]
    eng.dev_chunk_sharing(*(g.ptr if m else 0 for g in ins), m, n_files, *ptr, stream=stream)
    eng.dev_sync(stream)
    torch.cuda.synchronize()
    for g in ins + outs:
        assert g.check() == []
    assert all(g.unchanged() for g in ins)
    for j, o in enumerate(outs):
        if not outputs[j]:
            assert o.untouched(), f"null output {j} was written"
    got = {name: outs[j].download(np.int64 if name == "peer" else np.uint64) for j, name in enumerate(NAMES)}
    got["counts"] = dict(zip(COUNTS, (int(x) for x in outs[5].download(np.uint64))))
    return got


def agree(got, want, outputs=(True,) * 6):
    for j, name in enumerate(NAMES):
        if outputs[j]:
            assert (got[name] == want[name]).all(), name
    if outputs[5]:
        assert got["counts"] == want["counts"]


def both(eng, chunk_file, chunk_len, rep, n_files):
    want = R.sharing(chunk_file, chunk_len, rep, n_files)
    agree(host_call(eng, chunk_file, chunk_len, rep, n_files), want)
    agree(device_call(eng, chunk_file, chunk_len, rep, n_files), want)
    return want


# ---- fixed cases ------------------------------------------------------------------------

def test_no_chunks(eng):
    want = both(eng, [], [], [], 3)
    assert want["peer"].tolist() == [-1, -1, -1] and want["counts"]["files"] == 3
    both(eng, [], [], [], 0)


def test_all_chunks_distinct(eng):
    m = 1000
    want = both(eng, np.arange(m) // 10, np.arange(m) + 1, np.arange(m), 100)
    assert want["counts"]["distinct_chunks"] == m and want["counts"]["files_with_peer"] == 0


def test_one_file_of_4096_equal_chunks(eng):
    want = both(eng, np.zeros(4096, np.uint32), np.full(4096, 300), np.zeros(4096, np.int64), 1)
    assert want["self_bytes"].tolist() == [4095 * 300] and want["new_bytes"].tolist() == [300]


def test_two_identical_files(eng):
    k = 500
    lens = np.r_[np.arange(k) + 64, np.arange(k) + 64]
    want = both(eng, np.r_[np.zeros(k), np.ones(k)], lens, np.r_[np.arange(k), np.arange(k)], 2)
    assert want["peer"].tolist() == [-1, 0] and want["peer_bytes"][1] == lens[:k].sum() == want["other_bytes"][1]


def test_three_origins_and_a_two_way_tie(eng):
    # files 0..2 hold one chunk each; file 3 draws 50 from 0, 70 from 1 (twice 35), 60 from 2
    # file 4 draws 80 from 2 and 80 from 1: the tie goes to file 1
    chunk_file = [0, 1, 2, 3, 3, 3, 3, 4, 4]
    chunk_len = [50, 35, 60, 50, 35, 35, 60, 80, 80]
    rep = [0, 1, 2, 0, 1, 1, 2, 2, 1]
    # (chunk 7 and 8 carry another length than their rep: the pass takes the inputs as they are)
    want = both(eng, chunk_file, chunk_len, rep, 5)
    assert want["peer"].tolist() == [-1, -1, -1, 1, 1] and want["peer_bytes"].tolist() == [0, 0, 0, 70, 80]
    assert want["other_bytes"].tolist() == [0, 0, 0, 180, 160]


def test_stray_reps_count_as_first_occurrences(eng):
    chunk_file = [0, 0, 1, 1, 1, 2]
    chunk_len = [10, 20, 30, 40, 50, 60]
    rep = [-1, 2, 6, 1 << 40, 0, -(1 << 62)]  # c + 1, m, 2^40 and negatives; chunk 4 is really chunk 0 again
    want = both(eng, chunk_file, chunk_len, rep, 3)
    assert want["new_bytes"].tolist() == [30, 70, 60] and want["other_bytes"].tolist() == [0, 50, 0]
    assert want["counts"]["distinct_chunks"] == 5


def test_sums_pass_2_to_the_32_and_wrap_at_2_to_the_64(eng):
    big = 1 << 40
    want = both(eng, [0, 0, 1, 1, 1], [big, big, big, big, big], [0, 0, 0, 0, 0], 2)
    assert want["self_bytes"][0] == big and want["other_bytes"][1] == 3 * big and want["counts"]["total_bytes"] == 5 * big
    huge = (1 << 63) + 5
    want = both(eng, [0, 1, 1, 1], [huge, huge, huge, 7], [0, 0, 0, 3], 2)
    assert want["other_bytes"][1] == 10 and want["peer_bytes"][1] == 10 and want["counts"]["total_bytes"] == 3 * 5 + 7 + (1 << 63)


# ---- larger cases ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def large():
    """100 003 chunks over 3 000 files with random classes, members of some
    classes in the first and in the last workgroup"""
    rng = np.random.default_rng(7)
    m, nf = 100003, 3000
    chunk_file = np.sort(rng.integers(0, nf, m)).astype(np.uint32)
    cls = rng.integers(0, 30000, m)
    cls[:5] = [1, 2, 3, 1, 2]
    cls[-5:] = [1, 2, 3, 40000, 40000]
    first = {}
    rep = np.array([first.setdefault(int(c), i) for i, c in enumerate(cls)], np.int64)
    chunk_len = (rng.integers(1, 5000, 30000 + 10001))[np.minimum(cls, 40000)].astype(np.uint64)
    return chunk_file, chunk_len, rep, nf, R.sharing(chunk_file, chunk_len, rep, nf)


def test_a_hundred_thousand_chunks(eng, large):
    chunk_file, chunk_len, rep, nf, want = large
    assert want["counts"]["files_with_peer"] > 2000 and (want["self_bytes"] > 0).any()
    agree(host_call(eng, chunk_file, chunk_len, rep, nf), want)
    agree(device_call(eng, chunk_file, chunk_len, rep, nf), want)


def test_a_smaller_call_after_a_larger_one_and_null_outputs(eng, large):
    chunk_file, chunk_len, rep, nf, _ = large
    device_call(eng, chunk_file, chunk_len, rep, nf)  # leaves the workspace dirty
    cf, cl, rp = chunk_file[:700], chunk_len[:700], rep[:700]
    n2 = int(cf.max()) + 1
    want = R.sharing(cf, cl, rp, n2)
    agree(device_call(eng, cf, cl, rp, n2), want)
    for j in range(6):
        outputs = tuple(k != j for k in range(6))
        agree(device_call(eng, cf, cl, rp, n2, outputs), want, outputs)


def test_misaligned_and_oversized_arguments_are_refused(eng):
    g = Guarded(256, align=16, fill=FILL)
    for kw in ({"new_bytes": g.ptr + 4}, {"peer": g.ptr + 2}, {"counts": g.ptr + 4}):
        with pytest.raises(N.SdcasError) as e:
            eng.dev_chunk_sharing(g.ptr, g.ptr, g.ptr, 1, 1, **kw)
        assert e.value.code == N.SDCAS_E_INVALID
    with pytest.raises(N.SdcasError) as e:
        eng.dev_chunk_sharing(g.ptr + 2, g.ptr, g.ptr, 1, 1)
    assert e.value.code == N.SDCAS_E_INVALID
    with pytest.raises(N.SdcasError) as e:
        eng.dev_chunk_sharing(g.ptr, g.ptr, g.ptr, (1 << 30) + 1, 1)
    assert e.value.code == N.SDCAS_E_CAPACITY
    torch.cuda.synchronize()
    assert g.untouched() and g.check() == []


# ---- end to end ----------------------------------------------------------------------------

def near_files():
    a = content("synth", 0, 65536, content_key(0xCDC1, 1))
    b = np.concatenate([a[:1000], np.array([0x42], np.uint8), a[1000:]])
    c = a.copy()
    c[20000:24000] = content("synth", 0, 4000, content_key(0xCDC1, 2))
    d = content("synth", 0, 30000, content_key(0xCDC1, 3))
    return [a, b, c, d, np.concatenate([a, d])]


def test_the_input_is_one_where_an_insertion_keeps_most_chunks():
    files = near_files()
    offs = np.r_[0, np.cumsum([f.size for f in files])[:-1]]
    blob = np.concatenate(files)
    want = R.chunk_files(files, offs, R.DEFAULT_PARAMS)
    rep = R.chunk_reps(blob, want["chunk_off"], want["chunk_len"])
    s = R.sharing(want["chunk_file"], want["chunk_len"], rep, 5)
    assert s["peer"][1] == 0 and s["peer_bytes"][1] >= 0.9 * files[0].size


def test_similar_files_on_real_files(eng, tmp_path):
    files = near_files()
    paths = []
    for name, f in zip("ABCDE", files):
        p = tmp_path / name
        p.write_bytes(f.tobytes())
        paths.append(p)
    for params in (None, R.TEST_PARAMS):
        got = eng.similar_files(paths, params)
        pr = R.DEFAULT_PARAMS if params is None else params
        want = R.chunk_files(files, [0] * 5, pr)  # offsets in the file
        assert got["chunk_counts"] == want["counts"] and got["sizes"].tolist() == [f.size for f in files]
        for name in ("file_chunks", "chunk_off", "chunk_len", "chunk_file"):
            assert (got[name] == want[name]).all(), name
        offs = np.r_[0, np.cumsum([f.size for f in files])[:-1]].astype(np.uint64)
        rep = R.chunk_reps(np.concatenate(files), want["chunk_off"] + offs[want["chunk_file"]], want["chunk_len"])
        assert (got["rep"] == rep).all()
        agree({**got, "counts": got["sharing_counts"]}, R.sharing(want["chunk_file"], want["chunk_len"], rep, 5))
        assert got["peer"].tolist()[:3] == [-1, 0, 0] and got["peer"][4] in (0, 3)
    with pytest.raises(ValueError, match="max_bytes"):
        eng.similar_files(paths, max_bytes=1000)


def test_chunk_confirm_and_sharing_on_one_stream(eng):
    files = near_files()
    lens = np.array([f.size for f in files], np.uint64)
    starts = np.r_[0, np.cumsum((lens + 64 + 15) // 16 * 16)[:-1]].astype(np.uint64)
    img = np.zeros(int(starts[-1] + lens[-1]) + 64, np.uint8)
    for s, f in zip(starts, files):
        img[int(s):int(s) + f.size] = f
    mc, ms = eng.chunk_plan(lens, R.TEST_PARAMS)
    want = R.chunk_files(files, starts, R.TEST_PARAMS)
    m = want["counts"]["chunks"]
    rep_want = R.chunk_reps(img, want["chunk_off"], want["chunk_len"])
    share_want = R.sharing(want["chunk_file"], want["chunk_len"], rep_want, 5)
    st = torch.cuda.Stream()
    blob, d_offs, d_lens = (torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in (img, starts, lens))
    i64 = lambda k: torch.zeros(max(k, 1), dtype=torch.int64, device="cuda")
    fc, off, ln, keys, rep, ccnt, scnt = i64(6), i64(mc), i64(mc), i64(mc), i64(mc), i64(6), i64(6)
    fl = torch.zeros(mc, dtype=torch.int32, device="cuda")
    dig = torch.zeros(32 * mc, dtype=torch.uint8, device="cuda")
    outs = [i64(5) for _ in range(5)]
    torch.cuda.synchronize()
    s = st.cuda_stream
    eng.dev_chunk(blob.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), 5, mc, ms, R.TEST_PARAMS, fc.data_ptr(),
                  off.data_ptr(), ln.data_ptr(), fl.data_ptr(), keys.data_ptr(), dig.data_ptr(), ccnt.data_ptr(), s)
    # (the chunk count came down with dev_chunk's one wait; a caller that stays on the device passes the bound)
    eng.dev_confirm_duplicates(keys.data_ptr(), dig.data_ptr(), 0, m, rep.data_ptr(), stream=s)
    eng.dev_chunk_sharing(fl.data_ptr(), ln.data_ptr(), rep.data_ptr(), m, 5, *(o.data_ptr() for o in outs),
                          scnt.data_ptr(), s)
    eng.dev_sync(s)
    torch.cuda.synchronize()
    assert (rep.cpu().numpy()[:m] == rep_want).all()
    got = {name: o.cpu().numpy().view(np.int64 if name == "peer" else np.uint64) for name, o in zip(NAMES, outs)}
    got["counts"] = dict(zip(COUNTS, (int(x) for x in scnt.cpu().numpy().view(np.uint64))))
    agree(got, share_want)
