"""The chunk windows' numpy model (tests/_cdc_win_ref.py) against the whole-file
cuts of tests/_cdc_ref.py: a file chunked window by window, and a window cut
segment by segment and stitched, give exactly the cuts of the whole file."""
import numpy as np
import pytest

from tests import _cdc_ref as R
from tests import _cdc_win_ref as W

P = R.TEST_PARAMS
LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4096, 40000, 40001)
CONTENTS = ("random", "two_valued", "constant138", "zeros", "period97")
WINDOWS = (1024, 1025, 2048, 4096, 5000)
SEGMENTS = (2048, 2112, 4096, 4160)


def make(kind, n):
    rng = np.random.default_rng(97 + n)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "two_valued":
        return rng.choice(np.array([3, 138], np.uint8), n)
    if kind == "constant138":
        return np.full(n, 138, np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    return (np.arange(n) % 97).astype(np.uint8)


_whole = {}


def whole(kind, n):
    if (kind, n) not in _whole:
        _whole[kind, n] = (make(kind, n),) + R.cuts(make(kind, n), P)
    return _whole[kind, n]


@pytest.mark.parametrize("kind", CONTENTS)
def test_a_final_window_is_the_whole_file(kind):
    for n in LENGTHS:
        x, ends, kinds = whole(kind, n)
        e, k, used = W.window_cuts(x, P, True)
        assert (e == ends).all() and (k == kinds).all() and used == n, (kind, n)


@pytest.mark.parametrize("kind", CONTENTS)
def test_windows_that_restart_at_consumed_give_the_whole_file_cuts(kind):
    for n in LENGTHS:
        x, ends, kinds = whole(kind, n)
        for w in WINDOWS:
            e, k, windows = W.streamed_cuts(x, P, w)
            assert e.tolist() == ends.tolist() and k.tolist() == kinds.tolist(), (kind, n, w)
            assert W.kind_counts(k) == W.kind_counts(kinds)
            assert windows >= 1 and (n <= w or windows > 1)


def test_a_window_that_is_not_final_stops_where_it_cannot_decide():
    z = np.zeros(1023, np.uint8)
    e, k, used = W.window_cuts(z, P, False)
    assert e.size == 0 and used == 0
    e, k, used = W.window_cuts(np.zeros(1024, np.uint8), P, False)
    assert e.tolist() == [1024] and k.tolist() == [W.KIND_MAX] and used == 1024
    e, k, used = W.window_cuts(np.zeros(63, np.uint8), P, False)
    assert e.size == 0 and used == 0
    e, k, used = W.window_cuts(np.zeros(0, np.uint8), P, False)
    assert e.size == 0 and used == 0
    # a window that ends exactly at a hash cut: the cut is taken and is no END chunk
    x, ends, kinds = whole("random", 40000)
    first_hash = int(ends[np.flatnonzero(kinds == R.KIND_HASH)[3]])
    e, k, used = W.window_cuts(x[:first_hash], P, False)
    assert used == first_hash and e[-1] == first_hash and k[-1] == W.KIND_HASH
    assert e.tolist() == ends[:e.size].tolist()


@pytest.mark.parametrize("kind", CONTENTS)
def test_segments_stitched_give_the_whole_file_cuts(kind):
    for n in LENGTHS:
        x, ends, kinds = whole(kind, n)
        for seg in SEGMENTS:
            e, k, used, walks, taken = W.segmented_cuts(x, P, seg)
            assert e.tolist() == ends.tolist() and k.tolist() == kinds.tolist() and used == n, (kind, n, seg)
            assert W.kind_counts(k) == W.kind_counts(kinds)
            assert (len(walks) == 0) == (n < 2 * seg)


def test_constant_content_never_merges_and_walks_every_segment():
    """constant 138 cuts every 256 bytes from wherever a chain starts, and 2112
    is no multiple of 256: in a segment that does not begin at a multiple of
    256 the true chain never lands on a listed cut, and the walk is the
    segment's whole result. Every fourth segment begins at one (4 * 2112 =
    33 * 256); there the true chain enters at the segment's start and the
    whole list is taken"""
    x, ends, kinds = whole("constant138", 40000)
    assert (np.diff(np.concatenate([[0], ends]))[:-1] == 256).all()
    e, k, used, walks, taken = W.segmented_cuts(x, P, 2112)
    assert e.tolist() == ends.tolist()
    assert len(walks) == -(-40000 // 2112)
    for j in range(len(walks)):
        # the segment's chunks: the cuts after the true entry cut up to the first at or past its end
        chunks = int(((ends > walk_start(ends, j)) & (ends <= walk_end(ends, j))).sum())
        if j % 4 == 0:
            assert walks[j] == 0 and taken[j] == chunks, j
        else:
            assert taken[j] == 0 and walks[j] == chunks and chunks >= 8, j
    assert sum(walks) + sum(taken) == ends.size


def walk_start(ends, j):
    """the true chain's entry cut of segment j: the first cut at or past j * 2112 (segment 0: the file's start)"""
    return int(ends[ends >= j * 2112][0]) if j else 0


def walk_end(ends, j):
    past = ends[ends >= (j + 1) * 2112]
    return int(past[0]) if past.size else int(ends[-1])


def test_random_content_merges_after_about_one_cut():
    walked = []
    for n in (40000, 40001):
        x, ends, kinds = whole("random", n)
        for seg in SEGMENTS:
            walks = W.segmented_cuts(x, P, seg)[3]
            walked += walks[1:]
    assert len(walked) > 50 and np.mean(walked) < 3, np.mean(walked)


def test_windows_that_are_not_final_are_segmented_exactly_too():
    for kind in ("random", "constant138"):
        x, ends, kinds = whole(kind, 40001)
        for cut in (20000, 5 * 2112, 5 * 2112 + 17):
            want = W.window_cuts(x[:cut], P, False)
            got = W.segmented_cuts(x[:cut], P, 2112, False)
            assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2] == want[2]
            assert want[0].tolist() == ends[:want[0].size].tolist()


def test_the_default_parameters_at_a_1_mib_segment():
    x = np.random.default_rng(5).integers(0, 256, (3 << 20) + 17, dtype=np.uint8)
    ends, kinds = R.cuts(x, R.DEFAULT_PARAMS)
    e, k, used, walks, taken = W.segmented_cuts(x, R.DEFAULT_PARAMS, 1 << 20)
    assert e.tolist() == ends.tolist() and k.tolist() == kinds.tolist() and len(walks) == 4
    e, k, windows = W.streamed_cuts(x, R.DEFAULT_PARAMS, (1 << 20) + 1)
    assert e.tolist() == ends.tolist() and k.tolist() == kinds.tolist() and windows >= 3


def test_window_files_sums_to_the_whole_files_counts():
    files = [make("random", 5000), make("zeros", 3000), make("period97", 0), make("random", 100)]
    want = R.chunk_files(files, [0] * 4, P)["counts"]
    total = dict.fromkeys(want, 0)
    for x in files:
        pos = 0
        while True:
            w = x[pos:pos + 2048]
            final = pos + w.size >= x.size
            got = W.window_files([w], [0], [final], P)
            for name, v in got["counts"].items():
                total[name] += v
            if final:
                break
            pos += int(got["consumed"][0])
    assert total == want
