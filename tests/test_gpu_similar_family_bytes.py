"""Engine.similar_families and Engine.family_bytes_of on real files, the corpus of
tests/test_gpu_similar_families.py: five versions of a growing log, three
versions of a second document, a large file that embeds the first log, and two
unrelated files. The two sets are the versions, the log's first (it gives most
back); every byte count is also the reference's (tests/_family_bytes_ref.py)
over the chunk arrays the calls return, exactly. Parameters (64, 8, 1024): no
chunk is longer than 1024 bytes."""
import numpy as np
import pytest

from spacedrive_amd import ChunkHolders
from tests import _family_bytes_ref as R

pytestmark = pytest.mark.gpu

P = (64, 8, 1024)
MAX_CHUNK = 1024
K = 4
LOG = [0, 2, 4, 6, 7]  # the log's five versions among the 11 files, oldest first
DOC = [1, 5, 8]
EMBED, LONE = 9, [3, 10]
CHUNK_KEYS = ("chunk_file", "chunk_len", "chunk_keys", "chunk_digests")
BEFORE = {"sizes", "new_bytes", "self_bytes", "other_bytes", "indexed_bytes", "peer", "peer_bytes", "chunk_counts",
          "match_counts", "add_counts"}
BEFORE_PEERS = BEFORE | {"peers", "peers_bytes", "peer_count", "shared_bytes", "common_bytes", "peers_counts"}


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
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
    d = tmp_path_factory.mktemp("family_bytes")
    out = []
    for i, x in enumerate(files):
        p = d / f"f{i:02d}.bin"
        p.write_bytes(x.tobytes())
        out.append(p)
    return out


@pytest.fixture(scope="module")
def whole(eng, paths):
    """similar_families over all the files, once"""
    return eng.similar_families(paths, K, params=P)


@pytest.fixture(scope="module")
def batches(eng, paths):
    """three similar_files_indexed calls on a fresh holders index, chunks kept"""
    index, ids, out = ChunkHolders(eng), np.arange(len(paths), dtype=np.uint64), []
    for lo, hi in ((0, 4), (4, 8), (8, 11)):
        out.append((eng.similar_files_indexed(paths[lo:hi], ids[lo:hi], index, P, peers=K, chunks=True), ids[lo:hi]))
    return out


def chunks_of(batches):
    """the batches' chunk arrays as one corpus, and rep by a dict over (key, digest)"""
    fl, ln, pairs, row0 = [], [], [], 0
    for r, ids in batches:
        fl += [int(f) + row0 for f in r["chunk_file"]]
        ln += [int(x) for x in r["chunk_len"]]
        pairs += [(int(k), bytes(d)) for k, d in zip(r["chunk_keys"], r["chunk_digests"])]
        row0 += ids.size
    first, rep = {}, []
    for c, p in enumerate(pairs):
        rep.append(first.setdefault(p, c))
    return fl, ln, rep


def sets(got):
    off = got["set_offsets"].astype(np.int64)
    return [got["members"][off[s]:off[s + 1]].tolist() for s in range(got["set_rep"].size)]


def test_one_call_equals_three_batches_and_the_reference(eng, whole, batches):
    got = eng.family_bytes_of([r for r, _ in batches], [i for _, i in batches])
    assert set(whole) == set(got) | {"sizes"}
    for key in got:
        if isinstance(got[key], dict):
            assert got[key] == whole[key], key
        else:
            assert np.array_equal(got[key], whole[key]), key
    assert np.array_equal(whole["sizes"], np.concatenate([r["sizes"] for r, _ in batches]))
    fl, ln, rep = chunks_of(batches)
    want = R.family_bytes(fl, ln, rep, got["family"])
    for name in R.ROWS + R.SETS + ("set_reclaimable",):
        assert np.array_equal(got[name], want[name]) and np.array_equal(whole[name], want[name]), name
    assert got["counts"] == want["counts"] == whole["counts"]
    w_off, w_members = R.members_of(got["family"], want["set_rep"])
    assert np.array_equal(got["set_offsets"], w_off) and np.array_equal(got["members"], w_members)
    assert np.array_equal(whole["file_bytes"], whole["sizes"])  # every byte of a file lies in one chunk


def test_the_two_sets_are_the_versions_the_logs_first(whole, batches):
    assert sets(whole) == [LOG, DOC] and whole["set_rep"].tolist() == [0, 1]
    assert whole["set_files"].tolist() == [5, 3]
    assert whole["set_reclaimable"][0] > whole["set_reclaimable"][1] > 0
    # families_of's form of the same sets, by rep, under its own names
    assert whole["families_set_rep"].tolist() == [0, 1] and whole["families_counts"]["families"] == 2
    assert whole["families_members"].tolist() == LOG + DOC and whole["families_set_offsets"].tolist() == [0, 5, 8]
    c = whole["counts"]
    assert (c["files"], c["sets"], c["members"]) == (11, 2, 8) and c["largest_reclaimable"] == whole["set_reclaimable"][0]
    assert c["set_reclaimable_bytes"] == int(whole["set_reclaimable"].sum())
    assert c["total_bytes"] == int(whole["sizes"].sum())


def test_the_logs_set_stores_its_largest_version_and_little_more(whole, batches):
    sizes = whole["sizes"]
    assert int(whole["set_total"][0]) == int(sizes[LOG].sum())
    # what the reference finds over the same cuts: the sum of the first-occurrence lengths in the log's rows
    fl, ln, rep = chunks_of(batches)
    want = R.family_bytes(fl, ln, rep, whole["family"])
    stored = int(want["set_stored"][0])
    assert stored == sum(int(want["delta_bytes"][i]) for i in LOG) == int(whole["set_stored"][0])
    # a version appended to another re-cuts only the chunk at the old end, and no chunk exceeds 1024
    # bytes: the closed form is asserted where the reference over these cuts confirms it
    largest = int(sizes[LOG].max())
    print("log set: stored", stored, "largest version", largest, "bound", largest + 5 * MAX_CHUNK)
    if largest <= stored <= largest + 5 * MAX_CHUNK:
        assert largest <= int(whole["set_stored"][0]) <= largest + 5 * MAX_CHUNK
    for v, row in enumerate(LOG[1:], start=1):  # each later version inherits all but its tail
        assert int(whole["inherited_bytes"][row]) >= int(sizes[LOG[v - 1]]) - MAX_CHUNK


def test_the_embedding_file_and_the_lone_files_are_in_no_set(whole):
    for row in [EMBED] + LONE:
        assert whole["family"][row] == row and whole["inherited_bytes"][row] == 0
        assert row not in whole["members"].tolist()
        assert whole["delta_bytes"][row] + whole["self_bytes"][row] == whole["sizes"][row]
    # the embedding file shares the first log's chunks, but across labels nothing is reclaimed
    assert whole["delta_bytes"][EMBED] == whole["sizes"][EMBED]


def test_without_chunks_the_dict_is_what_it_was(eng, paths, batches):
    ids = np.arange(4, dtype=np.uint64)
    plain = eng.similar_files_indexed(paths[:4], ids, ChunkHolders(eng), P)
    assert set(plain) == BEFORE
    near = eng.similar_files_indexed(paths[:4], ids, ChunkHolders(eng), P, peers=K)
    assert set(near) == BEFORE_PEERS
    kept = batches[0][0]
    assert set(kept) == BEFORE_PEERS | set(CHUNK_KEYS)
    for key in BEFORE_PEERS:
        if isinstance(near[key], dict):
            assert near[key] == kept[key], key
        else:
            assert np.array_equal(near[key], kept[key]), key
    m = kept["chunk_file"].size
    assert kept["chunk_file"].dtype == np.uint32 and kept["chunk_len"].dtype == np.uint64
    assert kept["chunk_keys"].shape == (m,) and kept["chunk_digests"].shape == (m, 32)
    assert int(kept["chunk_len"].sum()) == int(kept["sizes"].sum())
    with pytest.raises(ValueError):
        eng.family_bytes_of([near], [ids])  # no chunk arrays
    with pytest.raises(ValueError):
        eng.family_bytes_of([kept], [ids[:3]])  # rows that do not match the ids
