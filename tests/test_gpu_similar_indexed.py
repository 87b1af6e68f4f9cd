"""Engine.similar_files_indexed through one ChunkIndex against
similar_files_streamed over all the files at once: for ids ascending in scan
order and any split into consecutive batches, the per-batch results, one after
the other, are the one call's, entry for entry, with its peer mapped through
the ids; and the final index is the sorted distinct set of all chunks, each
with its first owner. Parameters (64, 8, 1024): files of 20-200 KiB give
hundreds of chunks."""
import numpy as np
import pytest

from spacedrive_amd import ChunkIndex
from tests import _chunk_index_ref as R

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
    rng = np.random.default_rng(50)
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
    d = tmp_path_factory.mktemp("indexed")
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


def check_law(eng, paths, ids, want, cuts, window_bytes=256 << 20, reload_at=None, tmp_path=None):
    index = ChunkIndex(eng)
    got = {k: [] for k in NAMES + ("indexed_bytes",)}
    for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        if reload_at == j:
            f = tmp_path / "index.npz"
            index.save(f)
            index = ChunkIndex.load(eng, f)
        r = eng.similar_files_indexed(paths[lo:hi], ids[lo:hi], index, P, window_bytes)
        for k in got:
            assert r[k].shape == (hi - lo,)
            got[k].append(r[k])
    got = {k: np.concatenate(v) for k, v in got.items()}
    peer = np.where(want["peer"] >= 0, ids[np.maximum(want["peer"], 0)].astype(np.int64), -1)
    for k in NAMES:
        w = peer if k == "peer" else want[k]
        assert got[k].dtype == w.dtype and (got[k] == w).all(), k
    # the bytes an earlier batch had stored: the chunks whose first copy lies before this file's batch
    first_of_batch = np.repeat(cuts[:-1], np.diff(cuts))
    fl, rep, ln = want["chunk_file"], want["rep"], want["chunk_len"]
    early = fl[rep] < first_of_batch[fl]
    wi = np.zeros(len(paths), np.uint64)
    np.add.at(wi, fl[early], ln[early])
    assert (got["indexed_bytes"] == wi).all()
    # the final index: the sorted distinct chunks, each with its first owner
    k, d, v, dr, bits = index.arrays()
    ref = R.build(want["keys"], want["digests"], ids[fl])
    assert R.from_arrays(k, d, v) == ref and index.n == len(ref)
    assert dr.tolist() == R.directory(ref, bits)
    return index


@pytest.mark.parametrize("cuts", [[0, 12], [0, 5, 12], [0, 3, 3, 7, 12], [0, 1, 2, 6, 12]])
def test_batches_equal_one_call(eng, corpus, cuts):
    paths, ids, want = corpus
    check_law(eng, paths, ids, want, cuts)


def test_save_and_load_between_batches(eng, corpus, tmp_path):
    paths, ids, want = corpus
    check_law(eng, paths, ids, want, [0, 4, 12], reload_at=1, tmp_path=tmp_path)


def test_a_file_larger_than_the_window(eng, corpus):
    paths, ids, want = corpus
    assert max(int(s) for s in want["sizes"]) > 3 * 16384
    check_law(eng, paths, ids, want, [0, 6, 12], window_bytes=16384)


def test_a_loaded_file_with_a_flipped_byte_is_refused(eng, corpus, tmp_path):
    paths, ids, _ = corpus
    index = ChunkIndex(eng)
    eng.similar_files_indexed(paths[:2], ids[:2], index, P)
    f = tmp_path / "index.npz"
    index.save(f)
    assert ChunkIndex.load(eng, f).n == index.n
    with np.load(f) as z:
        arrays = {k: z[k].copy() for k in z.files}
    g = tmp_path / "flipped.npz"
    # a byte of the file itself (in the digests, the largest member): the archive's checksum
    raw = bytearray(f.read_bytes())
    raw[len(raw) // 2] ^= 0x01
    g.write_bytes(bytes(raw))
    with pytest.raises(ValueError):
        ChunkIndex.load(eng, g)
    # a byte of an array saved as it is: an entry out of order (the key's top
    # byte), a slot that no longer holds its count
    assert index.n > 100
    for name, at, bit in (("keys", index.n // 2, np.uint64(1 << 63)), ("dir", 1, np.uint32(0x80))):
        bad = {k: v.copy() for k, v in arrays.items()}
        bad[name][at] ^= bit
        with open(g, "wb") as out:
            np.savez(out, **bad)
        with pytest.raises(ValueError):
            ChunkIndex.load(eng, g)
