"""Engine.similar_recipes and Engine.family_recipes_of on real files: three
versions of one document (v2 is v1 with an insertion in the middle, v3 is v2
with a tail appended), a file that repeats one of its own blocks, an unrelated
file and an empty file. The recipes rebuild every file byte for byte through
rebuild_files, reading only the literal ranges; the versions take far fewer ops
than chunks. Parameters (64, 8, 1024): files of 50 to 200 KiB have hundreds of
chunks."""
import numpy as np
import pytest

from spacedrive_amd import ChunkHolders, rebuild_files
from tests import _family_recipes_ref as R

pytestmark = pytest.mark.gpu

P = (64, 8, 1024)
K = 4
V1, V2, V3, REPEAT, LONE, EMPTY = range(6)
OP_KEYS = R.OPS + ("op_literal", "chunk_op", "chunk_off") + R.ROWS


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    rng = np.random.default_rng(312)
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    v1 = rand(150 << 10)
    v2 = v1[:70000] + rand(4096) + v1[70000:]
    v3 = v2 + rand(10 << 10)
    block = rand(20 << 10)
    repeat = rand(30 << 10) + block + rand(25 << 10) + block + rand(5 << 10)
    contents = [v1, v2, v3, repeat, rand(120 << 10), b""]
    d = tmp_path_factory.mktemp("similar_recipes")
    paths = []
    for i, x in enumerate(contents):
        p = d / f"f{i}.bin"
        p.write_bytes(x)
        paths.append(p)
    return paths, contents


@pytest.fixture(scope="module")
def whole(eng, corpus):
    return eng.similar_recipes(corpus[0], K, params=P)


def chunks_per_row(rec, n):
    on = rec["chunk_op"] != R.NONE
    return np.bincount(rec["op_row"][rec["chunk_op"][on]], minlength=n)


def test_the_recipes_rebuild_every_file_from_the_literal_ranges(whole, corpus):
    paths, contents = corpus
    rec = whole["recipes"]
    reads = []

    def read(row, off, n):  # from the files themselves: only what a literal op names
        reads.append((row, off, n))
        with open(paths[row], "rb") as f:
            f.seek(off)
            return f.read(n)
    built = rebuild_files(rec, read)
    assert [built[i] for i in range(len(contents))] == contents
    lit = rec["op_literal"]
    assert sorted(reads) == sorted(zip(rec["op_row"][lit].tolist(), rec["op_dst_off"][lit].tolist(),
                                       rec["op_len"][lit].tolist()))
    total = sum(len(x) for x in contents)
    assert sum(r[2] for r in reads) == rec["counts"]["literal_bytes"] < total
    assert rec["counts"]["literal_bytes"] + rec["counts"]["copy_bytes"] == total
    assert rec["counts"]["files"] == 6 and rec["counts"]["chunks"] == rec["chunk_op"].size
    assert (rec["chunk_op"] != R.NONE).all()  # every chunk takes part
    assert np.array_equal(rec["chunk_off"][rec["op_chunk"]], rec["op_dst_off"])


def test_the_versions_take_far_fewer_ops_than_chunks(whole, corpus):
    rec = whole["recipes"]
    chunks = chunks_per_row(rec, 6)
    print("chunks per row", chunks.tolist(), "ops per row", rec["row_ops"].tolist())
    assert chunks[V1] > 100
    for row in (V2, V3):
        assert rec["row_ops"][row] < chunks[row]
    assert rec["row_ops"][V1] == 1  # the first version keeps itself: one literal op
    # the family's literal bytes are what the same dict says the family stores
    assert whole["family"][[V1, V2, V3]].tolist() == [V1, V1, V1]
    s = whole["set_rep"].tolist().index(V1)
    in_family = np.isin(rec["op_row"], [V1, V2, V3]) & rec["op_literal"]
    assert int(rec["op_len"][in_family].sum()) == int(whole["set_stored"][s])
    for row in (V1, V2, V3):  # and per row, the family bytes of the same call (law 1)
        mine = rec["op_row"] == row
        assert int(rec["op_len"][mine & rec["op_literal"]].sum()) == int(whole["delta_bytes"][row])
        assert int(rec["op_len"][mine & ~rec["op_literal"]].sum()) == \
            int(whole["self_bytes"][row]) + int(whole["inherited_bytes"][row])
        k, at = int(rec["row_ops"][row]), int(rec["row_first_op"][row])
        assert (rec["op_row"][at:at + k] == row).all()  # adjacent chunks: adjacent ops


def test_the_other_files(whole, corpus):
    _, contents = corpus
    rec = whole["recipes"]
    at = int(rec["row_first_op"][LONE])
    assert rec["row_ops"][LONE] == 1 and rec["op_literal"][at] and rec["op_len"][at] == len(contents[LONE])
    assert rec["op_dst_off"][at] == 0 and rec["op_src_row"][at] == LONE
    assert rec["row_ops"][EMPTY] == 0 and rec["row_first_op"][EMPTY] == R.NONE
    mine = rec["op_row"] == REPEAT  # the repeated block comes from the file itself
    assert (rec["op_src_row"][mine] == REPEAT).all() and (~rec["op_literal"][mine]).any()
    assert int(rec["op_len"][mine & ~rec["op_literal"]].sum()) == int(whole["self_bytes"][REPEAT]) > 15 << 10
    assert rec["row_ops"][REPEAT] < chunks_per_row(rec, 6)[REPEAT]


def test_three_batches_give_the_same_recipes(eng, whole, corpus):
    paths, _ = corpus
    index, ids, batches = ChunkHolders(eng), np.arange(len(paths), dtype=np.uint64), []
    for lo, hi in ((0, 2), (2, 4), (4, 6)):
        batches.append(eng.similar_files_indexed(paths[lo:hi], ids[lo:hi], index, P, peers=K, chunks=True))
    got = eng.family_recipes_of(batches, [ids[0:2], ids[2:4], ids[4:6]])
    assert set(whole) == set(got) | {"sizes"}
    for key in OP_KEYS:
        assert np.array_equal(got["recipes"][key], whole["recipes"][key]), key
    assert got["recipes"]["counts"] == whole["recipes"]["counts"]
    assert set(got["recipes"]) == set(OP_KEYS) | {"counts"}
    plain = eng.family_bytes_of(batches, [ids[0:2], ids[2:4], ids[4:6]])  # its dict is family_bytes_of's, plus one key
    assert set(got) == set(plain) | {"recipes"}
    for key in plain:
        if isinstance(plain[key], dict):
            assert plain[key] == got[key], key
        else:
            assert np.array_equal(plain[key], got[key]), key
