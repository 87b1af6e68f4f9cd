"""Engine.similar_files_indexed(..., peers=k) through a ChunkHolders: the law of
tests/test_gpu_similar_holders.py for the peers keys (ids ascending in scan
order, any split into consecutive batches, the one call's rows; after
remove(R), the later batches' rows are those of one run over the survivors),
the three versions of a growing log as real files, and peers=0 as before.
Parameters (64, 8, 1024): files of 20-200 KiB give hundreds of chunks."""
import numpy as np
import pytest

from spacedrive_amd import ChunkHolders, ChunkIndex
from tests import _chunk_holders_ref as H
from tests import _chunk_peers_ref as R

pytestmark = pytest.mark.gpu

P = (64, 8, 1024)
K = 3
PER_FILE = ("peers", "peers_bytes", "peer_count", "shared_bytes", "common_bytes")
TODAY = ["sizes", "new_bytes", "self_bytes", "other_bytes", "indexed_bytes", "peer", "peer_bytes", "chunk_counts",
         "match_counts", "add_counts"]
V1, V2, V3 = 7, 8, 9  # the log's versions among the 12 files


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(eng, tmp_path_factory):
    """12 files, the three versions of a log among them, their ids, and the
    reference's peers over the chunks of all of them"""
    rng = np.random.default_rng(80)
    kib = lambda lo, hi: int(rng.integers(lo * 1024, hi * 1024))
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8)
    a, b, c = rand(kib(60, 200)), rand(kib(20, 60)), rand(kib(100, 200))
    ins = int(rng.integers(1, a.size))
    over = c.copy()
    over[30000:34096] = rand(4096)  # an overwritten block
    log_a, log_b, log_c = rand(kib(80, 100)), rand(kib(20, 30)), rand(kib(8, 12))
    files = [a, b, a.copy(),                                  # a copy
             np.concatenate([a[:ins], rand(1), a[ins:]]),     # one byte inserted
             c, np.zeros(0, np.uint8), over,
             log_a, np.concatenate([log_a, log_b]), np.concatenate([log_a, log_b, log_c]),  # v1 = A, v2 = A B, v3 = A B C
             np.concatenate([b, c[:50000]]),                  # the whole of one file, half of another
             np.concatenate([b[:10000], b[:10000]])]          # a file that repeats itself
    d = tmp_path_factory.mktemp("peers")
    paths = []
    for i, x in enumerate(files):
        p = d / f"f{i:02d}.bin"
        p.write_bytes(x.tobytes())
        paths.append(p)
    ids = (1000 + 7 * np.arange(len(paths))).astype(np.uint64)  # ascending in scan order, not the positions
    return paths, ids, reference(eng, paths, ids)


def reference(eng, paths, ids):
    """tests/_chunk_peers_ref.py over the files' chunks, against the index of all of them"""
    s = eng.similar_files_streamed(paths, params=P)
    entries = H.build(s["keys"], s["digests"], ids[s["chunk_file"]])
    return R.peers(entries, s["keys"], s["digests"], s["chunk_file"], s["chunk_len"], ids, K, 64, R.EARLIER)


def run_batches(eng, index, paths, ids, cuts):
    got = {k: [] for k in PER_FILE + ("peer",)}
    for lo, hi in zip(cuts, cuts[1:]):
        r = eng.similar_files_indexed(paths[lo:hi], ids[lo:hi], index, P, peers=K)
        assert sorted(r) == sorted(TODAY + list(PER_FILE) + ["peers_counts"])
        assert r["peers"].shape == r["peers_bytes"].shape == (hi - lo, K) and r["peers"].dtype == np.uint64
        assert r["peers_counts"]["files"] == hi - lo and r["peers_counts"]["overflow"] == 0
        for k in got:
            got[k].append(r[k])
    return {k: np.concatenate(v) for k, v in got.items()}


@pytest.mark.parametrize("cuts", [[0, 12], [0, 5, 12], [0, 3, 3, 7, 12], [0, 1, 2, 6, 12]])
def test_batches_equal_one_call(eng, corpus, cuts):
    paths, ids, want = corpus
    got = run_batches(eng, ChunkHolders(eng), paths, ids, cuts)
    for k in PER_FILE:
        assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), k
    assert want["counts"]["files_with_peer"] >= 6 and want["peer_count"].max() == K


def test_later_batches_after_a_remove(eng, corpus):
    """the first 5 files indexed, files 0 and 4 removed, the rest indexed: the
    later files' rows are those of one run over the survivors and them"""
    paths, ids, full = corpus
    gone, k = [0, 4], 5
    assert any(int(v) in ids[gone] for i in range(k, 12) for v in full["peers"][i, :full["peer_count"][i]])
    index = ChunkHolders(eng)
    run_batches(eng, index, paths, ids, [0, k])
    index.remove(ids[gone])
    got = run_batches(eng, index, paths, ids, [k, 9, 12])
    keep = [i for i in range(12) if i not in gone]
    s_paths, s_ids = [paths[i] for i in keep], ids[keep]
    want = reference(eng, s_paths, s_ids)
    one = run_batches(eng, ChunkHolders(eng), s_paths, s_ids, [0, len(keep)])
    later = np.array([j for j, i in enumerate(keep) if i >= k])
    for name in PER_FILE:
        assert (got[name] == want[name][later]).all() and (one[name] == want[name]).all(), name
    assert not np.isin(got["peers"], ids[gone]).any()


def test_the_third_version_of_a_log_is_nearest_to_the_second(eng, corpus):
    paths, ids, want = corpus
    got = run_batches(eng, ChunkHolders(eng), paths, ids, [0, 12])
    sizes = [p.stat().st_size for p in paths]
    assert got["peers"][V3, 0] == ids[V2] and got["peers"][V3, 1] == ids[V1] and got["peer_count"][V3] == 2
    assert got["peers"][V2, 0] == ids[V1] and got["peer_count"][V1] == 0
    # v2 holds v3's chunks up to v2's last cut (its end chunk, at most max_len bytes, is not one of v3's);
    # v1 holds them up to v1's last cut
    assert sizes[V2] - 1024 <= got["peers_bytes"][V3, 0] <= sizes[V2]
    assert sizes[V1] - 1024 <= got["peers_bytes"][V3, 1] <= sizes[V1]
    # the lowest-holder answer is unchanged: most of v3's chunks have v1 as their origin
    plain = eng.similar_files_indexed(paths, ids, ChunkHolders(eng), P)
    assert plain["peer"][V3] == got["peer"][V3] == int(ids[V1]) and sorted(plain) == sorted(TODAY)
    assert plain["peer_bytes"][V3] == got["peers_bytes"][V3, 1]


def test_peers_0_returns_the_dict_it_did_and_a_chunk_index_is_refused(eng, corpus):
    paths, ids, _ = corpus
    a = eng.similar_files_indexed(paths[:4], ids[:4], ChunkHolders(eng), P)
    b = eng.similar_files_indexed(paths[:4], ids[:4], ChunkHolders(eng), P, peers=0, max_holders=5)
    assert sorted(a) == sorted(b) == sorted(TODAY)
    for k in TODAY:
        assert a[k] == b[k] if isinstance(a[k], dict) else (a[k] == b[k]).all(), k
    ci = ChunkIndex(eng)
    with pytest.raises(ValueError):
        eng.similar_files_indexed(paths[:2], ids[:2], ci, P, peers=1)
    assert ci.n == 0  # refused before anything was chunked or added
    eng.similar_files_indexed(paths[:2], ids[:2], ci, P)
    got = eng.similar_files_indexed(paths[2:4], ids[2:4], ChunkHolders.from_index(ci), P, peers=1)  # from_index converts
    assert got["peers"][0, 0] == ids[0] and got["peer_count"].tolist() == [1, 1]
