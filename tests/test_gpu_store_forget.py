"""FamilyStore.remove on real files, with the corpus and chunk parameters of
tests/test_gpu_store_files.py (versions of a growing log, unrelated files,
parameters (64, 8, 1024)) and two more logs, so that there are three families
to take from: the oldest version of one, a middle version of another, a whole
family. No file is read by remove; the originals are read here only to say what
the new store must hold."""
import numpy as np
import pytest

from spacedrive_amd import FamilyStore
from spacedrive_amd.recipes import pack_store
from tests import _family_recipes_ref as R

pytestmark = pytest.mark.gpu

P = (64, 8, 1024)
# rows: log a 0-4, log b 5-7, log c 8-9, unrelated 10-12
GONE = [0, 6, 8, 9]


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    rng = np.random.default_rng(77)
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    contents = []
    for size, versions in ((190 << 10, 5), (90 << 10, 3), (70 << 10, 2)):  # logs that grow
        log = rand(size)
        for _ in range(versions):
            contents.append(log)
            log = log + rand(5 << 10)
    contents += [rand(60 << 10), rand(33333), rand(100 << 10)]
    d = tmp_path_factory.mktemp("store_forget")
    paths = []
    for i, x in enumerate(contents):
        p = d / f"f{i}.bin"
        p.write_bytes(x)
        paths.append(p)
    return paths, contents


@pytest.fixture(scope="module")
def fs(eng, corpus):
    return eng.store_files(corpus[0], params=P)


@pytest.fixture(scope="module")
def removed(fs):
    return fs.remove(GONE)


def same_store(a, b):
    assert R.same(a.recipes, b.recipes) and np.array_equal(a.recipes["chunk_off"], b.recipes["chunk_off"])
    assert np.array_equal(a.layout["op_store_off"], b.layout["op_store_off"])
    assert a.layout["counts"] == b.layout["counts"]
    assert a.store.tobytes() == b.store.tobytes()
    assert np.array_equal(a.sizes, b.sizes) and np.array_equal(a.digests, b.digests)
    for name in ("chunk_file", "chunk_len", "rep", "family"):
        assert np.array_equal(a.chunks[name], b.chunks[name]), name


def test_the_corpus_has_the_three_families(fs):
    fam = fs.chunks["family"]
    assert fam[:5].tolist() == [0] * 5 and fam[5:8].tolist() == [5] * 3 and fam[8:10].tolist() == [8] * 2
    assert fs.chunks["chunk_file"].size == fs.recipes["chunk_op"].size > 1000
    assert fs.verify() == []


def test_the_new_store_gives_the_surviving_files_back(fs, removed, corpus):
    paths, contents = corpus
    new, row_from = removed
    left = [r for r in range(len(contents)) if r not in GONE]
    assert isinstance(new, FamilyStore) and row_from.dtype == np.uint32 and row_from.tolist() == left
    assert new.verify() == []
    assert new.restore() == {j: contents[r] for j, r in enumerate(left)}
    assert new.sizes.tolist() == [len(contents[r]) for r in left]
    assert np.array_equal(new.digests, fs.digests[left])
    assert len(new.store) == new.recipes["counts"]["literal_bytes"] < len(fs.store)
    assert new.layout["counts"]["uncovered_ops"] == 0
    # the store of the surviving files, read from the originals
    files = [open(paths[r], "rb").read() for r in left]
    want = pack_store(new.recipes, new.layout, lambda row, at, n: files[row][at:at + n])
    assert new.store.tobytes() == want.tobytes()
    # the first survivor of log a now keeps what version 0 kept; log c is gone from the store
    assert new.chunks["family"].tolist() == [0] * 4 + [4] * 2 + [6, 7, 8]
    # the original is as it was
    assert fs.sizes.size == len(contents) and fs.verify() == []


def test_nothing_and_everything(fs):
    same, row_from = fs.remove([])
    assert row_from.tolist() == list(range(fs.sizes.size))
    same_store(same, fs.remove(np.array([], np.int64))[0])
    assert same.store.tobytes() == fs.store.tobytes() and R.same(same.recipes, fs.recipes)
    assert np.array_equal(same.layout["op_store_off"], fs.layout["op_store_off"]) and same.verify() == []
    none, row_from = fs.remove(range(fs.sizes.size))
    assert row_from.size == 0 and none.store.size == 0 and none.sizes.size == 0
    assert none.recipes["counts"]["ops"] == 0 and none.chunks["chunk_file"].size == 0
    assert none.verify() == [] and none.restore() == {}
    with pytest.raises(ValueError):
        fs.remove([fs.sizes.size])


def test_two_steps_equal_one(fs, removed):
    first, from1 = fs.remove([0, 9])
    # rows 6 and 8 of the original are 5 and 7 of `first`
    assert from1.tolist()[5] == 6 and from1.tolist()[7] == 8
    second, from2 = first.remove([5, 7])
    same_store(second, removed[0])
    assert from1[from2].tolist() == removed[1].tolist()


def test_the_result_saves_and_loads(removed, tmp_path, corpus):
    _, contents = corpus
    new, row_from = removed
    new.save(tmp_path / "forgot.npz")
    back = FamilyStore.load(tmp_path / "forgot.npz", new.engine)
    same_store(back, new)
    assert back.verify() == [] and back.restore(rows=[0]) == {0: contents[int(row_from[0])]}
    again, _ = back.remove([0])  # a loaded store forgets as well
    assert again.verify() == []
