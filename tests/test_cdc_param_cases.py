"""The inputs of tests/test_gpu_chunk_params.py meet the conditions they were
built for (tests/_cdc_param_cases.py): every builder is called, which asserts
its own conditions against tests/_cdc_ref.py, and what the GPU tests rely on
beyond that is asserted here. No GPU."""
import numpy as np
import pytest

from tests import _cdc_param_cases as K
from tests import _cdc_ref as R
from tests import _cdc_win_ref as W


def same(a, b):
    return a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


@pytest.mark.parametrize("params", K.SWEEP_PARAMS, ids=str)
def test_sweep_inputs(params):
    files, p, expect = K.sweep(params)
    assert p == params and R.params_valid(p)
    mn, ab, mx = p
    assert [f.size for f in files[:-1]] == [0, 1, mn - 1, mn, mn + 1, mx - 1, mx, mx + 1]
    assert expect["long"]["hash_cuts"] >= 8
    if mx <= 2 << ab:
        assert expect["long"]["max_cuts"] >= 8
    assert all(f.size < 20 << 20 and not f.flags.writeable for f in files)
    assert files[-1].size >= 2 * K.seg_bytes(p)  # the windows' cut pass takes it in segments
    # the short files: one END chunk up to min_len, a cut at max_len at the latest
    for f, (ends, kinds) in zip(files[1:5], expect["cuts"][1:5]):
        if f.size <= mn:
            assert ends.tolist() == [f.size] and kinds.tolist() == [R.KIND_END]
    ends, kinds = expect["cuts"][7]
    assert ends[0] <= mx and ends.size >= 2 and kinds[-1] == R.KIND_END


def test_sweep_has_the_narrow_and_the_odd_sets():
    got = set(K.SWEEP_PARAMS)
    assert len(got) == 14 and all(R.params_valid(p) for p in got)
    assert {(32, 6, 65), (63, 6, 65), (127, 7, 129), (255, 8, 257), (4095, 12, 4097), (32, 20, (1 << 20) + 1)} <= got
    assert any(mn == (1 << ab) - 1 and mx == (1 << ab) + 1 for mn, ab, mx in got)  # one strict and two loose positions


@pytest.mark.parametrize("params", K.PLANTED_PARAMS, ids=str)
def test_planted_inputs(params):
    files, p, expect = K.planted(params)
    mn, ab, mx = p
    avg = 1 << ab
    sl, ll = K.limits(p)
    assert (sl, ll) == (1 << (31 - ab), 1 << (33 - ab))
    cases = K.planted_cases(p)
    assert expect["names"] == [c[0] for c in cases] and len(set(expect["names"])) == len(cases)
    H, M, E = R.KIND_HASH, R.KIND_MAX, R.KIND_END
    for x, s, (ends, kinds), (name, plants, rel_len, want_rel) in zip(files, expect["starts"], expect["cuts"], cases):
        assert s > 0 and s % 64 and int(s) in ends.tolist(), name  # the chunk under test starts at a cut, off every 64
        k = ends.tolist().index(s)
        assert kinds[k] == H and s - (ends[k - 1] if k else 0) >= mn
        got = [(int(e) - s, int(kd)) for e, kd in zip(ends[k + 1:], kinds[k + 1:])]
        assert got == want_rel and x.size == s + rel_len, name
        h = R.window_hash(x[s - 32:]) if ab < 24 else None
        for d, t in plants:
            assert int(R.window_hash(x[s + d - 32:s + d])[31]) == t, name
            if h is not None:
                assert int(h[32 + d - 1]) == t
        # the background holds no candidate: everything but the planted windows is zero
        mask = np.ones(x.size, bool)
        for e in [s] + [s + d for d, _ in plants]:
            mask[e - 32:e] = False
        assert not x[mask].any(), name
        if ab < 24:
            assert x.size >= 2 * K.seg_bytes(p), name
    if ab == 24:
        assert len(files) == 1 and (1 << 24) < files[0].size < (1 << 24) + (1 << 12)
        return
    by = dict(zip(expect["names"], (c[1:] for c in cases)))
    # each threshold at each edge of its range, as the definition states them
    assert by["zero_at_min_minus_1_ignored"] == ([(mn - 1, 0)], mx + 7, [(mx, M), (mx + 7, E)])
    assert by["zero_at_min_taken_then_min_left"] == ([(mn, 0)], 2 * mn, [(mn, H), (2 * mn, E)])
    assert by["zero_at_min_taken_then_one_byte"] == ([(mn, 0)], mn + 1, [(mn, H), (mn + 1, E)])
    assert by["strict_limit_at_avg_minus_1_ignored"][0] == [(avg - 1, sl)]
    assert by["below_strict_limit_at_avg_minus_1_taken"][0] == [(avg - 1, sl - 1)]
    assert by["strict_limit_at_avg_taken"][0] == [(avg, sl)] and by["strict_limit_at_avg_taken"][2][0] == (avg, H)
    assert by["loose_limit_at_avg_ignored"][0] == [(avg, ll)] and by["loose_limit_at_avg_ignored"][2][0] == (mx, M)
    assert by["below_loose_limit_at_avg_taken"][0] == [(avg, ll - 1)]
    assert by["loose_only_at_max_is_a_hash_cut"][0] == [(mx, sl)] and by["loose_only_at_max_is_a_hash_cut"][2][0] == (mx, H)
    assert by["loose_only_at_max_plus_1_is_a_max_cut"][0] == [(mx + 1, sl)]
    assert by["loose_only_at_max_plus_1_is_a_max_cut"][2][0] == (mx, M)
    assert by["candidate_at_the_end_is_an_end_chunk"] == ([(avg, 0)], avg, [(avg, E)])
    assert by["min_left_is_one_end_chunk"] == ([], mn, [(mn, E)])
    assert sl < ll and sl - 1 < sl  # the LOOSE-only window is not STRICT


def test_dense_inputs_fill_every_bound():
    files, p, expect = K.dense()
    assert p == (32, 6, 65) and [f.size for f in files] == [32, 33, 64, 65, 96, 97, 4096, 4097, 20001]
    total = 0
    for f, (ends, kinds) in zip(files, expect["cuts"]):
        assert (f == 138).all()
        room = R.chunk_plan([f.size], p)[0]
        assert ends.size == room == -(-f.size // 32)
        total += room
    assert expect["counts"]["chunks"] == total == R.chunk_plan([f.size for f in files], p)[0]
    assert expect["counts"]["max_cuts"] == 0  # strict-dense: every cut a hash cut at min_len


def test_dense_inputs_in_segments():
    """the segmented model of the windows' cut pass at the smallest segment:
    full lists in the dense files, walked segments in the changed ones"""
    files, p, expect = K.dense_mixed()
    seg = K.seg_bytes(p)
    assert seg == 192
    spl = -(-seg // p[0])
    seen = {"dense": 0, "changed": 0, "random": 0}
    for x, name, known in zip(files, expect["names"], expect["cuts"]):
        if x.size < 2 * seg:
            continue
        ends, kinds, used, walks, taken = W.segmented_cuts(x, p, seg)
        assert same((ends, kinds), known) and used == x.size, name
        kind = name.rstrip("0123456789")
        seen[kind] += 1
        if kind == "dense":
            # every segment's list is full and taken whole; the last holds what is left
            assert walks == [0] * len(walks) and taken[:-1] == [spl] * (len(taken) - 1), name
            assert taken[-1] == -(-(x.size - (len(taken) - 1) * seg) // p[0]), name
        elif kind == "changed":
            # one byte changed in the first segment: the true chain enters no later segment at its
            # start, meets none of its cuts and is walked to the end
            assert taken[0] > 0 and walks[0] == 0, name
            assert all(w > 0 for w in walks[1:]) and taken[1:] == [0] * (len(taken) - 1), name
    assert seen["dense"] == 3 and seen["changed"] == 3 and seen["random"] >= 3
    # the issue's example: 992 bytes are five full lists and one cut
    assert W.segmented_cuts(np.full(5 * seg + 32, 138, np.uint8), p, seg)[4] == [6, 6, 6, 6, 6, 1]


def test_dense_mixed_puts_full_files_between_others():
    files, p, expect = K.dense_mixed()
    names = expect["names"]
    assert sum(n.startswith("dense") for n in names) == 9 and sum(n.startswith("changed") for n in names) == 3
    for i, n in enumerate(names):
        if n.startswith("dense"):
            assert expect["cuts"][i][0].size == R.chunk_plan([files[i].size], p)[0]
            assert 0 < i < len(names) - 1
    for i, n in enumerate(names):
        if n.startswith("changed"):
            d = files[names.index("dense" + n[len("changed"):])]
            assert int((files[i] != d).sum()) == 1 and files[i][100] != d[100]


@pytest.mark.parametrize("params", K.STREAMED_PARAMS, ids=str)
def test_streamed_inputs(params):
    files, p, expect = K.streamed(params)
    seg = K.seg_bytes(p)
    assert max(f.size for f in files) >= 4 * seg  # windows of 2 * seg + 1 bytes are cut in segments
    for x, known in zip(files, expect["cuts"]):
        for w in (p[0], p[0] + 1, p[2], p[2] + 1, 2 * seg + 1):
            ends, kinds, _ = W.streamed_cuts(x, p, w)
            assert same((ends, kinds), known) or x.size == 0
