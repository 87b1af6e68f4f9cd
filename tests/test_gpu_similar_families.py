"""Engine.families_of over Engine.similar_files_indexed(..., peers=4) on real
files: five versions of a growing log, three versions of a second document, a
large file that embeds the first log, and two unrelated files. The families
are the two sets of versions, whatever the split into batches, and the log's
family survives the removal of its middle version. Every result is also the
reference's (tests/_families_ref.py) over the same rows, exactly. Parameters
(64, 8, 1024): files of 100 KiB and more give hundreds of chunks."""
import numpy as np
import pytest

from spacedrive_amd import ChunkHolders
from tests import _families_ref as F

pytestmark = pytest.mark.gpu

P = (64, 8, 1024)
K = 4
KEYS = ("sizes", "peer_count", "peers", "peers_bytes")
LOG = [0, 2, 4, 6, 7]  # the log's five versions among the 11 files, oldest first
DOC = [1, 5, 8]
EMBED, LONE = 9, [3, 10]


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    rng = np.random.default_rng(310)
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8)  # noqa: E731
    log = [rand(100 << 10)] + [rand(10 << 10) for _ in range(4)]
    logs = [np.concatenate(log[:v + 1]) for v in range(5)]  # v1 = A, v2 = A B, ... v5 = A B C D E
    d1 = rand(150 << 10)
    d2 = d1.copy()
    d2[70000:74096] = rand(4096)  # an overwritten block
    d3 = np.concatenate([d2, rand(10 << 10)])
    embed = np.concatenate([rand(1 << 20), logs[0], rand(1 << 20)])  # the first log inside 20 times as much
    files = [logs[0], d1, logs[1], rand(120 << 10), logs[2], d2, logs[3], logs[4], d3, embed, rand(200 << 10)]
    d = tmp_path_factory.mktemp("families")
    paths = []
    for i, x in enumerate(files):
        p = d / f"f{i:02d}.bin"
        p.write_bytes(x.tobytes())
        paths.append(p)
    ids = (1000 + 7 * np.arange(len(paths))).astype(np.uint64)  # ascending in scan order, not the positions
    return paths, ids


def run_batches(eng, index, paths, ids, cuts):
    out = []
    for lo, hi in zip(cuts, cuts[1:]):
        out.append((eng.similar_files_indexed(paths[lo:hi], ids[lo:hi], index, P, peers=K), ids[lo:hi]))
    return out


def families(eng, batches, num=1, den=2):
    """families_of, checked against the reference over the same concatenated rows"""
    got = eng.families_of([r for r, _ in batches], [i for _, i in batches], num, den)
    rows = [np.concatenate([np.asarray(r[key]) for r, _ in batches]) for key in KEYS]
    want = F.families(np.concatenate([i for _, i in batches]), *rows, num, den)
    assert F.same(got, want), (got["counts"], want["counts"])
    w_rep, w_off, w_members = F.sets_of(want["family"])
    assert np.array_equal(got["set_rep"], w_rep) and np.array_equal(got["set_offsets"], w_off)
    assert np.array_equal(got["members"], w_members)
    return got


def sets(got):
    off = got["set_offsets"].astype(np.int64)
    return [got["members"][off[s]:off[s + 1]].tolist() for s in range(got["set_rep"].size)]


@pytest.mark.parametrize("cuts", [[0, 11], [0, 4, 8, 11]])
def test_the_versions_are_the_two_families(eng, corpus, cuts):
    paths, ids = corpus
    batches = run_batches(eng, ChunkHolders(eng), paths, ids, cuts)
    got = families(eng, batches)
    assert sets(got) == [LOG, DOC] and got["set_rep"].tolist() == [0, 1]
    assert got["family"].tolist() == [0, 1, 0, 3, 0, 1, 0, 0, 1, 9, 10]
    assert got["family_size"].tolist() == [5, 3, 5, 1, 5, 3, 5, 5, 3, 1, 1]
    c = got["counts"]
    assert (c["families"], c["members"], c["largest"], c["unsorted"], c["files"]) == (2, 8, 5, 0, 11)
    # the file that embeds the first log shares its bytes with the versions, far below half of its own size
    assert c["weak"] >= 4 and c["missing"] == 0 and c["self_slots"] == 0
    # without a threshold it joins them
    loose = families(eng, batches, 0, 1)
    assert sets(loose) == [LOG + [EMBED], DOC] and loose["counts"]["weak"] == 0
    assert all(loose["family"][i] == i for i in LONE)


def test_one_batch_and_three_give_the_same_families(eng, corpus):
    paths, ids = corpus
    a = families(eng, run_batches(eng, ChunkHolders(eng), paths, ids, [0, 11]))
    b = families(eng, run_batches(eng, ChunkHolders(eng), paths, ids, [0, 4, 8, 11]))
    for key in ("family", "family_size", "set_rep", "set_offsets", "members"):
        assert np.array_equal(a[key], b[key]), key
    assert a["counts"] == b["counts"]


def test_the_log_survives_the_removal_of_its_middle_version(eng, corpus):
    """the first 7 files indexed (the fourth version lists the third), the third
    version removed, the rest indexed: with its row dropped the removed id is a
    missing slot of the fourth version's row, and the later versions link past
    it to the second"""
    paths, ids = corpus
    gone = LOG[2]
    index = ChunkHolders(eng)
    (first, first_ids), = run_batches(eng, index, paths, ids, [0, 7])
    assert int(ids[gone]) in first["peers"][LOG[3], :first["peer_count"][LOG[3]]].tolist()
    index.remove(ids[[gone]])
    (rest, rest_ids), = run_batches(eng, index, paths, ids, [7, 11])
    assert not np.isin(rest["peers"], ids[gone]).any()
    kept = {key: np.delete(np.asarray(first[key]), gone, axis=0) for key in KEYS}
    got = families(eng, [(kept, np.delete(first_ids, gone)), (rest, rest_ids)])
    # rows are renumbered without the removed one: 0 1 2 3 | 5 6 7 8 9 10 -> 0 .. 9
    assert sets(got) == [[0, 2, 5, 6], [1, 4, 7]]
    assert got["counts"]["missing"] >= 1 and got["counts"]["largest"] == 4 and got["counts"]["files"] == 10
