"""Engine.store_files and FamilyStore on real files: five versions of a growing
log (about 200 KiB each) and three unrelated files. The store holds the literal
bytes alone, every file comes back from it, verify proves that by checksum and
names exactly the rows a damaged store byte reaches. Parameters (64, 8, 1024):
the files have hundreds of chunks."""
import numpy as np
import pytest

from spacedrive_amd import FamilyStore
from tests import _family_store_ref as S

pytestmark = pytest.mark.gpu

P = (64, 8, 1024)


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
    log = rand(190 << 10)
    contents = []
    for _ in range(5):  # a log that grows
        contents.append(log)
        log = log + rand(5 << 10)
    contents += [rand(60 << 10), rand(33333), rand(100 << 10)]
    d = tmp_path_factory.mktemp("store_files")
    paths = []
    for i, x in enumerate(contents):
        p = d / f"f{i}.bin"
        p.write_bytes(x)
        paths.append(p)
    return paths, contents


@pytest.fixture(scope="module")
def fs(eng, corpus):
    return eng.store_files(corpus[0], params=P)


def test_the_store_holds_the_literal_bytes_and_gives_every_file_back(fs, corpus):
    _, contents = corpus
    assert isinstance(fs, FamilyStore) and fs.store.dtype == np.uint8
    assert len(fs.store) == fs.recipes["counts"]["literal_bytes"] < sum(int(s) for s in fs.sizes)
    assert fs.sizes.tolist() == [len(c) for c in contents]
    assert len(fs.store) < (190 << 10) + 5 * (5 << 10) + (60 << 10) + 33333 + (100 << 10) + (64 << 10)
    assert fs.layout["counts"]["uncovered_ops"] == 0
    # the store is the reference's, from the same recipes
    assert fs.store.tobytes() == bytes(S.pack_all(fs.recipes, S.layout(fs.recipes), contents))
    assert fs.restore() == dict(enumerate(contents))
    assert fs.restore(rows=[3]) == {3: contents[3]}
    assert fs.verify() == []


def test_small_windows_and_pieces(fs, corpus):
    _, contents = corpus
    assert fs.restore(window_bytes=512 << 10) == dict(enumerate(contents))  # two rows a window
    assert fs.restore(rows=[1, 6], window_bytes=50000) == {1: contents[1], 6: contents[6]}  # row 1 in pieces
    assert fs.verify(window_bytes=150000) == []  # the versions in pieces, hashed through the host path


def test_store_files_in_small_windows(eng, fs, corpus):
    other = eng.store_files(corpus[0], params=P, window_bytes=150000)  # the versions packed piece by piece
    assert other.store.tobytes() == fs.store.tobytes()
    assert np.array_equal(other.digests, fs.digests)


def test_a_flipped_store_byte_is_found(fs):
    for byte in (0, len(fs.store) // 2, len(fs.store) - 1):
        hurt = FamilyStore(fs.recipes, fs.layout, fs.store.copy(), fs.sizes, fs.digests, fs.engine)
        hurt.store[byte] ^= 0x40
        want = S.rows_reading(fs.recipes, S.layout(fs.recipes), byte)
        assert want and hurt.verify() == want
    assert len(S.rows_reading(fs.recipes, S.layout(fs.recipes), 0)) == 5  # every version reads the log's head


def test_save_and_load_verify_clean(fs, corpus, tmp_path):
    _, contents = corpus
    fs.save(tmp_path / "store.npz")
    back = FamilyStore.load(tmp_path / "store.npz", fs.engine)
    assert back.verify() == [] and back.restore(rows=[4, 7]) == {4: contents[4], 7: contents[7]}
