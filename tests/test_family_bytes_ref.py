"""The family bytes' plain-Python reference (tests/_family_bytes_ref.py) against
the worked example of the header, an O(m^2) brute force and the laws the
definition implies. No GPU."""
import random

import numpy as np

from tests import _family_bytes_ref as R

M64 = (1 << 64) - 1
I64_MIN = -(1 << 63)


def check_rows(got, want):
    for name in R.ROWS:
        assert [int(x) for x in got[name]] == [int(x) for x in want[name]], name


def random_case(rng, m, n, labels=None, bad=True):
    chunk_file = [rng.randrange(n + (2 if bad else 0)) if n else rng.randrange(3) for _ in range(m)]
    chunk_len = [rng.choice([0, 1, 7, 1 << 20, 1 << 63, M64]) for _ in range(m)]
    rep = []
    for c in range(m):
        x = rng.random()
        rep.append(c if x < .3 else rng.randrange(c + 1) if x < .8 or not bad else rng.choice([-1, c + 1, m + 5, I64_MIN]))
    if labels is None:
        labels = [rng.choice([rng.randrange(max(n, 1)), rng.randrange(max(n, 1)), i] + ([-1, n, I64_MIN] if bad else []))
                  for i in range(n)]
    return chunk_file, chunk_len, rep, labels


def test_the_worked_example():
    got = R.family_bytes(**R.EXAMPLE)
    check_rows(got, R.EXAMPLE_ROWS)
    for name in R.SETS:
        assert list(got[name]) == R.EXAMPLE_SETS[name], name
    assert list(got["set_reclaimable"]) == [25]
    assert got["counts"] == R.EXAMPLE_COUNTS and tuple(got["counts"]) == R.COUNTS
    offs, members = R.members_of(R.EXAMPLE["family"], got["set_rep"])
    assert list(offs) == [0, 3] and list(members) == [0, 1, 3]


def test_against_the_brute_force():
    rng = random.Random(11)
    for t in range(300):
        m, n = rng.randrange(0, 40), rng.randrange(0, 9)
        case = random_case(rng, m, n)
        got = R.family_bytes(*case)
        rows, classes = R.brute_force(*case)
        check_rows(got, rows)
        assert got["counts"]["classes"] == classes, t
        for i in range(n):  # file = delta + self + inherited
            assert int(got["file_bytes"][i]) == (int(got["delta_bytes"][i]) + int(got["self_bytes"][i]) +
                                                 int(got["inherited_bytes"][i])) & M64


def test_law_1_one_label_is_chunk_sharing():
    rng = random.Random(12)
    for t in range(50):
        m, n = rng.randrange(1, 60), rng.randrange(1, 7)
        chunk_file = sorted(rng.randrange(n) for _ in range(m))
        chunk_len = [rng.randrange(1, 1000) for _ in range(m)]
        rep = list(range(m))
        for c in range(m):  # confirm-style: rep[rep[c]] == rep[c] <= c
            if rng.random() < .5:
                rep[c] = rep[rng.randrange(c + 1)]
        got = R.family_bytes(chunk_file, chunk_len, rep, [rng.randrange(n)] * n if t % 2 else [0] * n)
        new, own, other, stored = R.sharing(chunk_file, chunk_len, rep, n)
        check_rows(got, dict(file_bytes=[a + b + c for a, b, c in zip(new, own, other)], delta_bytes=new,
                             self_bytes=own, inherited_bytes=other))
        assert got["counts"]["stored_bytes"] == stored


def test_law_2_every_row_its_own_label():
    rng = random.Random(13)
    for _ in range(50):
        m, n = rng.randrange(0, 60), rng.randrange(1, 9)
        case = random_case(rng, m, n, labels=list(range(n)))
        got = R.family_bytes(*case)
        assert not got["inherited_bytes"].any() and got["set_rep"].size == 0
        c = got["counts"]
        assert (c["sets"], c["members"], c["set_reclaimable_bytes"], c["largest_reclaimable"]) == (0, 0, 0, 0)


def test_law_3_stored_is_the_sum_of_delta_per_label():
    rng = random.Random(14)
    for _ in range(50):
        n = rng.randrange(2, 9)
        case = random_case(rng, rng.randrange(0, 60), n)
        got = R.family_bytes(*case)
        family = case[3]
        for s, r in enumerate(got["set_rep"]):
            rows = [i for i in range(n) if family[i] == family[int(r)]]
            assert rows[0] == int(r) and len(rows) == int(got["set_files"][s])
            assert sum(int(got["delta_bytes"][i]) for i in rows) & M64 == int(got["set_stored"][s])
            assert sum(int(got["file_bytes"][i]) for i in rows) & M64 == int(got["set_total"][s])


def test_labels_outside_the_range_take_no_part():
    # rows 1, 3 and 4 carry -1, n and INT64_MIN: they and their chunks count for nothing
    family = [0, -1, 0, 5, I64_MIN]
    chunk_file = [0, 1, 2, 3, 4, 2]
    got = R.family_bytes(chunk_file, [3, 100, 3, 100, 100, 4], [0, 0, 0, 0, 0, 5], family)
    check_rows(got, dict(file_bytes=[3, 0, 7, 0, 0], delta_bytes=[3, 0, 4, 0, 0], self_bytes=[0] * 5,
                         inherited_bytes=[0, 0, 3, 0, 0]))
    assert got["counts"] == dict(files=2, chunks=3, classes=2, total_bytes=10, stored_bytes=7, sets=1, members=2,
                                 set_reclaimable_bytes=3, largest_reclaimable=3)
    # the class's first occurrence is its lowest PARTICIPATING chunk: chunk 0 of a row outside does not shadow
    got = R.family_bytes([1, 0, 2], [9, 9, 9], [0, 0, 0], [0, -1, 0])
    check_rows(got, dict(file_bytes=[9, 0, 9], delta_bytes=[9, 0, 0], self_bytes=[0] * 3, inherited_bytes=[0, 0, 9]))
    # a label that is not its set's lowest row: the rep is still the lowest member
    got = R.family_bytes([], [], [], [2, 2, 1, 2])
    assert list(got["set_rep"]) == [0] and list(got["set_files"]) == [3]


def test_chunk_files_outside_the_rows_take_no_part():
    got = R.family_bytes([0, 2, (1 << 32) - 1, 1], [5, 50, 50, 5], [0, 0, 0, 0], [0, 0])
    check_rows(got, dict(file_bytes=[5, 5], delta_bytes=[5, 0], self_bytes=[0, 0], inherited_bytes=[0, 5]))
    assert got["counts"]["chunks"] == 2 and got["counts"]["classes"] == 1
    assert R.family_bytes([0, 1], [1, 2], [0, 0], [])["counts"] == dict.fromkeys(R.COUNTS, 0)


def test_reps_outside_zero_to_c_are_the_chunks_own_number():
    # rep 2 at chunk 1 is above it, -1 and INT64_MIN are below 0: each such chunk is its own class;
    # chunk 3's rep 1 names the NUMBER 1, the class chunk 1 fell back to
    got = R.family_bytes([0, 0, 0, 1, 1], [1, 2, 4, 8, 16], [0, 2, -1, 1, I64_MIN], [0, 0])
    check_rows(got, dict(file_bytes=[7, 24], delta_bytes=[7, 16], self_bytes=[0, 0], inherited_bytes=[0, 8]))
    assert got["counts"]["classes"] == 4


def test_lengths_zero_and_wrapping():
    got = R.family_bytes([0, 0, 1, 1], [1 << 63, 1 << 63, 0, 1 << 63], [0, 1, 2, 0], [0, 0])
    check_rows(got, dict(file_bytes=[0, 1 << 63], delta_bytes=[0, 0], self_bytes=[0, 0], inherited_bytes=[0, 1 << 63]))
    c = got["counts"]
    assert (c["total_bytes"], c["stored_bytes"], c["classes"]) == (1 << 63, 0, 3)
    assert list(got["set_total"]) == [1 << 63] and list(got["set_stored"]) == [0]
    # reclaimable is total - stored modulo 2^64, also when a sum wrapped below the other
    got = R.family_bytes([0, 1, 1], [M64, 2, M64], [0, 1, 0], [0, 0])
    assert list(got["set_total"]) == [(M64 + 2 + M64) & M64]
    assert list(got["set_stored"]) == [(M64 + 2) & M64]
    assert list(got["set_reclaimable"]) == [M64]


def test_ties_in_the_set_order_go_to_the_lowest_row():
    # labels 5 (rows 0, 3), 1 (rows 1, 2), 4 (rows 4, 5), 7 (rows 6, 7): reclaimable 0, 6, 6, 0
    family = [5, 1, 1, 5, 4, 4, 7, 7]
    chunk_file = [1, 2, 4, 5, 0, 6]
    got = R.family_bytes(chunk_file, [6, 6, 6, 6, 3, 3], [0, 0, 2, 2, 4, 5], family)
    assert list(got["set_rep"]) == [1, 4, 0, 6]
    assert list(got["set_reclaimable"]) == [6, 6, 0, 0]
    assert list(got["set_files"]) == [2, 2, 2, 2]
    c = got["counts"]
    assert (c["sets"], c["members"], c["set_reclaimable_bytes"], c["largest_reclaimable"]) == (4, 8, 12, 6)
    # m == 0: the rows still form sets, with zero bytes, ordered by rep
    got = R.family_bytes([], [], [], [3, 1, 1, 3, 4])
    assert list(got["set_rep"]) == [0, 1] and list(got["set_total"]) == [0, 0]
