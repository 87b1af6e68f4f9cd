"""Engine.similar_files_indexed through a ChunkHolders: the law of
tests/test_gpu_similar_indexed.py holds with it (ids ascending in scan order,
any split into consecutive batches, the one call's results), and the new one:
after remove(R), later batches get exactly the results of the one call over the
surviving files plus the batch, and the index is the one built from the
survivors' chunks with all their holders. Parameters (64, 8, 1024): files of
20-200 KiB give hundreds of chunks."""
import numpy as np
import pytest

from spacedrive_amd import ChunkHolders
from tests import _chunk_holders_ref as H

pytestmark = pytest.mark.gpu

P = (64, 8, 1024)
NAMES = ("sizes", "new_bytes", "self_bytes", "other_bytes", "peer", "peer_bytes")


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(eng, tmp_path_factory):
    """12 listed files (one path twice), their ids, and the one-call result"""
    rng = np.random.default_rng(70)
    kib = lambda lo, hi: int(rng.integers(lo * 1024, hi * 1024))
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8)
    a, b, c = rand(kib(60, 200)), rand(kib(20, 60)), rand(kib(100, 200))
    ins = int(rng.integers(1, a.size))
    over = c.copy()
    over[30000:34096] = rand(4096)  # an overwritten block
    files = [a, b, a.copy(),                                  # a copy
             np.concatenate([a[:ins], rand(1), a[ins:]]),     # one byte inserted
             c, np.zeros(0, np.uint8), over,
             np.concatenate([b, c[:50000]]),                  # the whole of one file, half of another
             rand(kib(20, 40)),
             np.concatenate([rand(1), over]),                 # one byte in front
             np.concatenate([b[:10000], b[:10000]])]          # a file that repeats itself
    d = tmp_path_factory.mktemp("holders")
    paths = []
    for i, x in enumerate(files):
        p = d / f"f{i:02d}.bin"
        p.write_bytes(x.tobytes())
        paths.append(p)
    paths.append(paths[1])  # a file listed twice
    ids = (1000 + 7 * np.arange(len(paths))).astype(np.uint64)  # ascending in scan order, not the positions
    want = eng.similar_files_streamed(paths, params=P)
    assert want["chunk_counts"]["chunks"] > 1000 and want["sharing_counts"]["files_with_peer"] >= 6
    return paths, ids, want


def assert_index_is(index, want, ids):
    """the index holds the chunks of `want` (a similar_files_streamed result
    over the files with `ids`) with all their holders"""
    k, d, v, dr, bits = index.arrays()
    ref = H.build(want["keys"], want["digests"], ids[want["chunk_file"]])
    assert H.from_arrays(k, d, v) == ref and index.n == len(ref)
    assert dr.tolist() == H.directory(ref, bits)
    return ref


def run_batches(eng, index, paths, ids, cuts):
    got = {k: [] for k in NAMES + ("indexed_bytes",)}
    for lo, hi in zip(cuts, cuts[1:]):
        r = eng.similar_files_indexed(paths[lo:hi], ids[lo:hi], index, P)
        for k in got:
            assert r[k].shape == (hi - lo,)
            got[k].append(r[k])
    return {k: np.concatenate(v) for k, v in got.items()}


@pytest.mark.parametrize("cuts", [[0, 12], [0, 5, 12], [0, 3, 3, 7, 12], [0, 1, 2, 6, 12]])
def test_batches_equal_one_call(eng, corpus, cuts):
    paths, ids, want = corpus
    index = ChunkHolders(eng)
    got = run_batches(eng, index, paths, ids, cuts)
    peer = np.where(want["peer"] >= 0, ids[np.maximum(want["peer"], 0)].astype(np.int64), -1)
    for k in NAMES:
        w = peer if k == "peer" else want[k]
        assert got[k].dtype == w.dtype and (got[k] == w).all(), k
    first_of_batch = np.repeat(cuts[:-1], np.diff(cuts))
    fl, rep, ln = want["chunk_file"], want["rep"], want["chunk_len"]
    early = fl[rep] < first_of_batch[fl]
    wi = np.zeros(len(paths), np.uint64)
    np.add.at(wi, fl[early], ln[early])
    assert (got["indexed_bytes"] == wi).all()
    ref = assert_index_is(index, want, ids)
    assert len(ref) > len({e[:2] for e in ref})  # some pair has more than one holder


@pytest.mark.parametrize("k,gone,cuts", [(5, [0, 4], [5, 12]), (8, [1, 4, 6], [8, 9, 12])])
def test_later_batches_after_a_remove(eng, corpus, k, gone, cuts):
    """the first k files indexed, the files `gone` removed, the rest indexed:
    the later files' results are the one call's over the survivors and them"""
    paths, ids, full = corpus
    # a removed file is, in the full run, the peer of a later one
    assert any(int(full["peer"][i]) in gone for i in range(k, 12))
    index = ChunkHolders(eng)
    run_batches(eng, index, paths, ids, [0, k])
    n_before = index.n
    counts = index.remove(ids[gone])
    assert counts["values"] == len(gone) and counts["entries_old"] == n_before and index.n == counts["entries_new"]
    got = run_batches(eng, index, paths, ids, cuts)
    keep = [i for i in range(12) if i not in gone]
    s_paths, s_ids = [paths[i] for i in keep], ids[keep]
    want = eng.similar_files_streamed(s_paths, params=P)
    later = np.array([j for j, i in enumerate(keep) if i >= k])
    peer = np.where(want["peer"] >= 0, s_ids[np.maximum(want["peer"], 0)].astype(np.int64), -1)
    for name in NAMES:
        w = (peer if name == "peer" else want[name])[later]
        assert got[name].dtype == w.dtype and (got[name] == w).all(), name
    assert not np.isin(got["peer"], ids[gone].astype(np.int64)).any()
    assert_index_is(index, want, s_ids)


def test_an_edited_file_under_its_old_id(eng, corpus):
    """a file indexed under an id, the id removed, the edited bytes indexed
    under the same id: as a fresh run that never saw the first version"""
    paths, ids, _ = corpus
    index = ChunkHolders(eng)
    run_batches(eng, index, paths, ids, [0, 5])
    index.remove([ids[4]])
    got = eng.similar_files_indexed([paths[6]], [ids[4]], index, P)  # c with a block overwritten, as c's next version
    fresh = ChunkHolders(eng)
    run_batches(eng, fresh, paths, ids, [0, 4])
    want = eng.similar_files_indexed([paths[6]], [ids[4]], fresh, P)
    for name in NAMES + ("indexed_bytes",):
        assert (got[name] == want[name]).all(), name
    a, b = index.arrays(), fresh.arrays()
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    # nothing of the first version is left: its chunks that the edit dropped are held by nobody
    pos, val, hold, _ = index.match(*(np.concatenate([w[k] for w in eng.chunk_stream([paths[4]], 1 << 20, P)])
                                      for k in ("keys", "digests")))
    assert (hold == 0).any() and (hold > 0).any()
