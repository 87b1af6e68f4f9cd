"""The family recipes' definition, GPU-free: the Python reference of
tests/_family_recipes_ref.py against the header's worked example, against the
definition read literally, and against its four laws on seeded corpora of
versions with edits (law 1 against tests/_family_bytes_ref.py, law 3 over real
bytes through spacedrive_amd.rebuild_files). The kernels' tests are
tests/test_gpu_family_recipes.py and tests/test_gpu_similar_recipes.py."""
import numpy as np
import pytest

from spacedrive_amd import rebuild_files
from tests import _family_bytes_ref as B
from tests import _family_recipes_ref as R

I64_MIN = -(1 << 63)
SEEDS = range(40)


def example():
    return tuple(R.EXAMPLE[k] for k in ("chunk_file", "chunk_off", "chunk_len", "rep", "family"))


def reader(contents, reads=None):
    def read(row, off, n):
        if reads is not None:
            reads.append((row, off, n))
        assert off + n <= len(contents[row])
        return contents[row][off:off + n]
    return read


def covered(rec):
    """every copy's source range lies inside the union of its source row's literal ranges"""
    lit = {}
    for o in np.flatnonzero(rec["op_literal"]):
        lit.setdefault(int(rec["op_row"][o]), set()).update(
            range(int(rec["op_dst_off"][o]), int(rec["op_dst_off"][o]) + int(rec["op_len"][o])))
    for o in np.flatnonzero(~rec["op_literal"]):
        at, n = int(rec["op_src_off"][o]), int(rec["op_len"][o])
        if not set(range(at, at + n)) <= lit.get(int(rec["op_src_row"][o]), set()):
            return False
    return True


def test_the_worked_example():
    got = R.family_recipes(*example())
    for name in R.OPS:
        assert got[name].tolist() == R.EXAMPLE_OPS[name], name
    for name, want in R.EXAMPLE_REST.items():
        assert got[name].tolist() == want, name
    assert got["op_literal"].tolist() == [True, False, True, False]
    assert got["counts"] == R.EXAMPLE_COUNTS
    assert R.same(R.literal_reading(*example()), got)
    assert R.running_offsets(R.EXAMPLE["chunk_file"], R.EXAMPLE["chunk_len"]).tolist() == R.EXAMPLE["chunk_off"]
    v1, v2 = bytes(range(60)), bytes(range(30)) + b"XXXXX" + bytes(range(30, 60))
    reads = []
    assert rebuild_files(got, reader([v1, v2], reads)) == {0: v1, 1: v2}
    assert sorted(reads) == [(0, 0, 60), (1, 30, 5)]  # the literal ranges alone: 65 bytes


@pytest.mark.parametrize("seed", SEEDS)
def test_the_reference_against_the_literal_reading(seed):
    _, cf, off, ln, rep, fam = R.versions(seed)
    assert R.same(R.literal_reading(cf, off, ln, rep, fam), R.family_recipes(cf, off, ln, rep, fam))
    rng = np.random.default_rng(seed)  # and with everything scrambled: any input is defined
    m, n = cf.size, fam.size
    cf2 = rng.integers(0, n + 2, m).astype(np.uint32)
    off2 = rng.integers(0, 50, m).astype(np.uint64)
    rep2 = rng.integers(-2, m + 2, m).astype(np.int64)
    fam2 = rng.integers(-1, n + 1, n).astype(np.int64)
    assert R.same(R.literal_reading(cf2, off2, ln, rep2, fam2), R.family_recipes(cf2, off2, ln, rep2, fam2))


@pytest.mark.parametrize("seed", SEEDS)
def test_laws_1_to_3(seed):
    contents, cf, off, ln, rep, fam = R.versions(seed)
    assert np.array_equal(off, R.running_offsets(cf, ln))
    rec = R.family_recipes(cf, off, ln, rep, fam)
    fb = B.family_bytes(cf, ln, rep, fam)
    n = fam.size
    lit, cp = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    np.add.at(lit, rec["op_row"][rec["op_literal"]], rec["op_len"][rec["op_literal"]])
    np.add.at(cp, rec["op_row"][~rec["op_literal"]], rec["op_len"][~rec["op_literal"]])
    assert np.array_equal(lit, fb["delta_bytes"])  # law 1
    assert np.array_equal(cp, fb["self_bytes"] + fb["inherited_bytes"])
    assert rec["counts"]["literal_bytes"] == fb["counts"]["stored_bytes"]
    assert rec["counts"]["files"] == fb["counts"]["files"] and rec["counts"]["chunks"] == fb["counts"]["chunks"]
    assert covered(rec)  # law 2
    assert rec["op_literal"][rec["chunk_op"][rec["op_src_chunk"]]].all()  # depth one: a source chunk is kept
    reads = []
    built = rebuild_files(rec, reader(contents, reads))  # law 3
    taking_part = [i for i in range(n) if 0 <= fam[i] < n]
    for i in taking_part:
        assert built[i] == contents[i], i
    assert sum(r[2] for r in reads) == rec["counts"]["literal_bytes"]
    for i in range(n):
        if i not in taking_part:
            assert built[i] == b"" and rec["row_ops"][i] == 0 and rec["row_first_op"][i] == R.NONE
    # a row's chunks are adjacent here: its ops are [row_first_op, row_first_op + row_ops)
    for i in taking_part:
        k, at = int(rec["row_ops"][i]), int(rec["row_first_op"][i])
        assert (k == 0 and at == R.NONE) or (rec["op_row"][at:at + k] == i).all()
    assert int(rec["row_ops"].sum()) == rec["counts"]["ops"]


@pytest.mark.parametrize("seed", SEEDS)
def test_law_4_every_row_its_own_label(seed):
    contents, cf, off, ln, rep, fam = R.versions(seed)
    n = fam.size
    rec = R.family_recipes(cf, off, ln, rep, np.arange(n))
    assert np.array_equal(rec["op_src_row"], rec["op_row"])
    assert rebuild_files(rec, reader(contents)) == dict(enumerate(contents))
    together = R.family_recipes(cf, off, ln, rep, fam)
    assert rec["counts"]["literal_bytes"] >= together["counts"]["literal_bytes"]


def test_the_laws_bite():
    """the corpora have what the laws speak of"""
    seen = dict(copies=0, other=0, own=0, merged=0)
    for seed in SEEDS:
        _, cf, off, ln, rep, fam = R.versions(seed)
        rec = R.family_recipes(cf, off, ln, rep, fam)
        cp = ~rec["op_literal"]
        seen["copies"] += int(cp.sum())
        seen["other"] += int((cp & (rec["op_src_row"] != rec["op_row"])).sum())
        seen["own"] += int((cp & (rec["op_src_row"] == rec["op_row"])).sum())
        seen["merged"] += rec["counts"]["chunks"] - rec["counts"]["ops"]
    assert all(v >= 10 for v in seen.values()), seen


def test_inputs_outside_the_ranges():
    # labels outside [0, n) and files at or above n take no part, and cut runs
    cf = [0, 0, 5, 0, 1, 1, 2, 0xFFFFFFFF]
    off = [0, 4, 0, 8, 0, 4, 0, 0]
    ln = [4] * 8
    rec = R.family_recipes(cf, off, ln, list(range(8)), [0, -1, 4, I64_MIN])
    assert R.same(R.literal_reading(cf, off, ln, list(range(8)), [0, -1, 4, I64_MIN]), rec)
    assert rec["chunk_op"].tolist() == [0, 0, R.NONE, 1, R.NONE, R.NONE, R.NONE, R.NONE]
    assert rec["op_len"].tolist() == [8, 4] and rec["counts"]["files"] == 1 and rec["counts"]["chunks"] == 3
    assert rec["row_ops"].tolist() == [2, 0, 0, 0] and rec["row_first_op"].tolist() == [0, R.NONE, R.NONE, R.NONE]
    # reps outside [0, c] are the chunk's own number: every chunk a literal, one run
    rec = R.family_recipes([0] * 4, [0, 1, 2, 3], [1] * 4, [-1, 2, I64_MIN, 1 << 40], [0])
    assert rec["op_len"].tolist() == [4] and rec["op_literal"].tolist() == [True]
    # zero-length chunks continue a run and add nothing; a run of them has length 0
    rec = R.family_recipes([0, 0, 0, 1, 1], [0, 3, 3, 0, 0], [3, 0, 2, 0, 0], [0, 1, 2, 1, 1], [0, 0])
    assert rec["op_len"].tolist() == [5, 0] and rec["op_literal"].tolist() == [True, False]
    assert rec["counts"]["longest_op"] == 5 and rec["counts"]["copy_bytes"] == 0
    assert rebuild_files(rec, lambda r, o, n: b"abcde"[o:o + n]) == {0: b"abcde", 1: b""}


def test_two_chunks_of_one_row_at_one_offset():
    """why literal-or-copy is part of continuation. Chunk 1 repeats chunk 0 at chunk 0's own offset, chunk
    2 is new and follows: every offset test lets the literal chunk 2 continue the copy chunk 1 (its
    source (row 0, 4) is chunk 1's source (row 0, 0) plus 4), and its bytes would be kept by nobody."""
    cf, off, ln, rep, fam = [0, 0, 0], [0, 0, 4], [4, 4, 4], [0, 0, 2], [0]
    rec = R.family_recipes(cf, off, ln, rep, fam)
    assert R.same(R.literal_reading(cf, off, ln, rep, fam), rec)
    assert rec["op_literal"].tolist() == [True, False, True] and rec["op_len"].tolist() == [4, 4, 4]
    assert rec["counts"]["literal_bytes"] == 8 and rec["counts"]["copy_bytes"] == 4
    # the other way round: a zero-length literal and its copy at one offset
    cf, off, ln, rep, fam = [0, 0], [0, 0], [0, 0], [0, 0], [0]
    rec = R.family_recipes(cf, off, ln, rep, fam)
    assert R.same(R.literal_reading(cf, off, ln, rep, fam), rec)
    assert rec["counts"]["ops"] == 2 and rec["op_literal"].tolist() == [True, False]
    assert rec["op_src_chunk"].tolist() == [0, 0] and rec["op_dst_off"].tolist() == [0, 0]


def test_interleaved_rows():
    cf = [0, 1, 0, 1]
    rec = R.family_recipes(cf, [0, 0, 4, 4], [4] * 4, [0, 0, 2, 2], [0, 0])
    assert rec["op_row"].tolist() == [0, 1, 0, 1] and rec["row_ops"].tolist() == [2, 2]
    assert rec["row_first_op"].tolist() == [0, 1]  # exact, but a row's ops are not adjacent
    data = b"abcdefgh"
    assert rebuild_files(rec, lambda r, o, n: data[o:o + n]) == {0: data, 1: data}


def test_rebuild_files_refuses_what_literals_do_not_cover():
    rec = R.family_recipes(*example())
    v1, v2 = bytes(range(60)), bytes(range(30)) + b"XXXXX" + bytes(range(30, 60))
    bad = dict(rec, op_src_off=rec["op_src_off"].copy())
    bad["op_src_off"][3] = 31  # reads one byte past row 0's literal
    with pytest.raises(ValueError, match="do not cover"):
        rebuild_files(bad, reader([v1, v2]))
    bad = dict(rec, op_src_row=rec["op_src_row"].copy())
    bad["op_src_row"][1] = 1  # row 1 keeps only [30, 35)
    with pytest.raises(ValueError, match="do not cover"):
        rebuild_files(bad, reader([v1, v2]))
    with pytest.raises(ValueError, match="returned"):
        rebuild_files(rec, lambda r, o, n: b"")
    with pytest.raises(ValueError, match="differ in length"):
        rebuild_files(dict(rec, op_len=rec["op_len"][:2]), reader([v1, v2]))
    no_flag = {k: v for k, v in rec.items() if k not in ("op_literal", "row_ops")}
    assert rebuild_files(no_flag, reader([v1, v2])) == {0: v1, 1: v2}  # literal: op_chunk == op_src_chunk
