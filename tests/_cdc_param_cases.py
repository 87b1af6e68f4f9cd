"""Test infrastructure: the inputs of tests/test_gpu_chunk_params.py, built and
checked without a GPU (tests/test_cdc_param_cases.py calls every builder).

Every builder returns (files, params, expect) with fixed seeds and asserts the
conditions its input is meant to meet against tests/_cdc_ref.py: expect["cuts"]
holds R.cuts(file, params) of every file (pass it to R.chunk_files as `known`),
expect["names"] a name per file, and the arrays are read-only.

sweep(params)      random content at one of SWEEP's parameter sets: files of the lengths around
                   min_len and max_len and a long one that shows 8 hash cuts at least and, where
                   max_len <= 2 * avg, 8 MAX cuts at least
planted(params)    one file per case of PLANTED_CASES: a background of zero bytes (no candidate at any
                   avg_bits), a chunk that starts at a planted cut, and windows of chosen hashes at
                   chosen distances from it; the reference's ends and kinds are the intended ones
dense()            files of byte 138 at (32, 6, 65): every chunk 32 bytes, chunks == max_chunks
dense_mixed()      those, the same with one byte changed and random files in one call
streamed(params)   short files for the window-by-window runs
"""
import functools

import numpy as np

from tests import _cdc_ref as R

KIND_END, KIND_HASH, KIND_MAX = R.KIND_END, R.KIND_HASH, R.KIND_MAX

# params -> the long file: random bytes, and before them chunks that end at planted
# windows of hash 0 and MAX chunks of zero bytes, where random bytes alone would
# have to be many MiB long to show 8 cuts of a kind
SWEEP = {
    (32, 6, 65): (20000, 0, 0),
    (33, 6, 65): (20000, 0, 0),
    (63, 6, 65): (20000, 0, 0),
    (32, 6, 1000): (20000, 0, 0),
    (100, 7, 129): (20000, 0, 0),
    (127, 7, 129): (40000, 0, 0),
    (65, 8, 1025): (40000, 0, 0),
    (64, 8, 1023): (40000, 0, 0),
    (255, 8, 257): (300000, 0, 0),
    (1000, 10, 1025): (400000, 8, 0),
    (32, 10, 4097): (100000, 0, 0),
    (4095, 12, 4097): (160000, 8, 0),
    (2048, 16, 1 << 17): (2 << 20, 0, 8),
    (32, 20, (1 << 20) + 1): (4 << 20, 8, 8),
}
SWEEP_PARAMS = tuple(SWEEP)

PLANTED_PARAMS = ((32, 6, 65), (33, 7, 129), (64, 8, 1024), (2048, 13, 65536), ((1 << 16) - 1, 16, (1 << 16) + 1),
                  (32, 24, (1 << 24) + 1))

DENSE_PARAMS = (32, 6, 65)
DENSE_LENS = (32, 33, 64, 65, 96, 97, 4096, 4097, 20001)
DENSE_BYTE, CHANGED_AT = 138, 100

STREAMED_PARAMS = ((32, 6, 65), (127, 7, 129), (65, 8, 1025))


def seg_bytes(params):
    """the smallest segment the windows' cut pass takes at these parameters"""
    return (2 * int(params[2]) + 63) // 64 * 64


def limits(params):
    """(strict_lim, loose_lim): STRICT(p) is h(p) < strict_lim, LOOSE(p) is h(p) < loose_lim"""
    return 1 << (31 - int(params[1])), 1 << (33 - int(params[1]))


def _frozen(files):
    for f in files:
        f.setflags(write=False)
    return files


def _rng(params, salt):
    return np.random.default_rng([salt] + [int(v) for v in params])


def _rand(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8)


def _counts(cuts):
    kinds = np.concatenate([k for _, k in cuts]) if cuts else np.zeros(0, np.uint8)
    return {"chunks": int(kinds.size), "hash_cuts": int((kinds == KIND_HASH).sum()),
            "max_cuts": int((kinds == KIND_MAX).sum()), "end_chunks": int((kinds == KIND_END).sum())}


def _cuts_of(files, params):
    return [R.cuts(f, params) if f.size else (np.zeros(0, np.int64), np.zeros(0, np.uint8)) for f in files]


# ---- a. the parameter sweep ---------------------------------------------------------------

def sweep_lens(params):
    mn, _, mx = params
    return [0, 1, mn - 1, mn, mn + 1, mx - 1, mx, mx + 1]


@functools.lru_cache(maxsize=None)
def sweep(params):
    mn, ab, mx = params
    avg = 1 << ab
    n_rand, k_hash, k_max = SWEEP[params]
    rng = _rng(params, 0xA)
    files = [_rand(rng, n) for n in sweep_lens(params)]
    # the long file: from offset 0, k_hash chunks that each end at a window of hash 0 (a cut at any
    # length in [min_len, max_len]), k_max * max_len zero bytes, then the random bytes
    head = []
    for i in range(k_hash):
        d = mn + (37 * i) % (mx - mn + 1)
        head.append(np.concatenate([np.zeros(d - 32, np.uint8), R.window_with_hash(0, rng)]))
    head.append(np.zeros(k_max * mx, np.uint8))
    files.append(np.concatenate(head + [_rand(rng, n_rand)]))
    assert all(f.size < 20 << 20 for f in files)
    cuts = _cuts_of(files, params)
    long_counts = _counts(cuts[-1:])
    assert long_counts["hash_cuts"] >= 8, (params, long_counts)
    if mx <= 2 * avg:
        assert long_counts["max_cuts"] >= 8, (params, long_counts)
    names = [f"len{n}" for n in sweep_lens(params)] + ["long"]
    return _frozen(files), params, {"cuts": cuts, "names": names, "counts": _counts(cuts), "long": long_counts}


# ---- b. exact thresholds at exact positions -------------------------------------------------

def planted_cases(params):
    """-> [(name, [(distance of the window's end from the chunk's start s, hash)], L - s,
    [(the intended end - s, kind)])]"""
    mn, ab, mx = params
    avg = 1 << ab
    sl, ll = limits(params)
    E, H, M = KIND_END, KIND_HASH, KIND_MAX
    if ab == 24:
        # one file: a MAX chunk here is 16 MiB. A window at the strict limit below avg is ignored; one
        # that is LOOSE only, one below the loose limit, at max_len is a HASH cut there; hash 0 at
        # min_len after it is a cut, and one byte is left
        return [("strict_limit_below_avg_ignored_loose_at_max_then_min_then_one_byte",
                 [(1000, sl), (mx, ll - 1), (mx + mn, 0)], mx + mn + 1, [(mx, H), (mx + mn, H), (mx + mn + 1, E)])]
    return [
        ("zero_at_min_minus_1_ignored", [(mn - 1, 0)], mx + 7, [(mx, M), (mx + 7, E)]),
        ("zero_at_min_taken_then_min_left", [(mn, 0)], 2 * mn, [(mn, H), (2 * mn, E)]),
        ("zero_at_min_taken_then_one_byte", [(mn, 0)], mn + 1, [(mn, H), (mn + 1, E)]),
        ("min_left_is_one_end_chunk", [], mn, [(mn, E)]),
        ("strict_limit_at_avg_minus_1_ignored", [(avg - 1, sl)], mx + 7, [(mx, M), (mx + 7, E)]),
        ("below_strict_limit_at_avg_minus_1_taken", [(avg - 1, sl - 1)], avg + 8, [(avg - 1, H), (avg + 8, E)]),
        ("strict_limit_at_avg_taken", [(avg, sl)], avg + 9, [(avg, H), (avg + 9, E)]),
        ("loose_limit_at_avg_ignored", [(avg, ll)], mx + 7, [(mx, M), (mx + 7, E)]),
        ("below_loose_limit_at_avg_taken", [(avg, ll - 1)], avg + 9, [(avg, H), (avg + 9, E)]),
        ("loose_only_at_max_is_a_hash_cut", [(mx, sl)], mx + 9, [(mx, H), (mx + 9, E)]),
        ("loose_only_at_max_plus_1_is_a_max_cut", [(mx + 1, sl)], mx + 9, [(mx, M), (mx + 9, E)]),
        ("candidate_at_the_end_is_an_end_chunk", [(avg, 0)], avg, [(avg, E)]),
    ]


def _planted_file(params, plants, rel_len, rng):
    """zero bytes; MAX chunks lead up to a window below the strict limit, whose cut at s begins
    the chunk under test; `plants` from there -> (file, s, the lead's intended cuts)"""
    mn, ab, mx = params
    sl, _ = limits(params)
    lead = 0 if ab == 24 else 5  # (five MAX chunks: the file is longer than two of the smallest segments)
    s = lead * mx + mn + 1
    if s % 64 == 0:
        s += 1
    assert s % 64 and mn <= s - lead * mx <= mx
    x = np.zeros(s + rel_len, np.uint8)
    spans = sorted((s + d, h) for d, h in plants)
    for (e0, _), (e1, _) in zip(spans, spans[1:]):
        assert e1 - 32 >= e0, "planted windows overlap"
    wins = {e: R.window_with_hash(h, rng) for e, h in spans}
    if spans and spans[0][0] - 32 == s - 1:
        # min_len 32 and a window that ends at s + 31: it begins on the last byte of the lead's
        # window, whose hash is then the strict value that byte's table entry allows
        b = int(wins[spans[0][0]][0])
        t = sl - 1 if (int(R.gear_table()[b]) ^ (sl - 1)) & 1 == 0 else sl - 2
        lead_w = R.window_with_hash(t, rng, last=b)
    else:
        assert not spans or spans[0][0] - 32 >= s
        lead_w = R.window_with_hash(sl - 1, rng)
    x[s - 32:s] = lead_w
    for e, w in wins.items():
        x[e - 32:e] = w
    lead_cuts = [(j * mx, KIND_MAX) for j in range(1, lead + 1)] + [(s, KIND_HASH)]
    return x, s, lead_cuts


@functools.lru_cache(maxsize=None)
def planted(params):
    assert params in PLANTED_PARAMS
    rng = _rng(params, 0xB)
    files, cuts, names, starts = [], [], [], []
    for name, plants, rel_len, want_rel in planted_cases(params):
        # a window's bytes enter the 31 hashes before and after its own and can make a stray
        # candidate: its free choices are drawn again until the reference's cuts are the intended ones
        for attempt in range(2000):
            x, s, lead_cuts = _planted_file(params, plants, rel_len, rng)
            want = lead_cuts + [(s + d, k) for d, k in want_rel]
            ends, kinds = R.cuts(x, params)
            if ends.tolist() == [e for e, _ in want] and kinds.tolist() == [k for _, k in want]:
                break
        else:
            raise AssertionError(f"no draw of {name} at {params} gives the intended cuts")
        # the planted hashes are where they were meant to be
        assert all(int(R.window_hash(x[s + d - 32:s + d])[31]) == t for d, t in plants), name
        assert s > 0 and s % 64 and x.size == s + rel_len
        files.append(x), cuts.append((ends, kinds)), names.append(name), starts.append(s)
    return _frozen(files), params, {"cuts": cuts, "names": names, "counts": _counts(cuts), "starts": starts}


# ---- c. the bounds the code calls "never" ---------------------------------------------------------

def _dense(n):
    return np.full(n, DENSE_BYTE, np.uint8)


def _changed(n):
    x = _dense(n)
    x[CHANGED_AT] ^= 0xFF
    return x


def _assert_full(files, cuts, names):
    mn = DENSE_PARAMS[0]
    for f, (ends, _), name in zip(files, cuts, names):
        if name.startswith("dense"):
            assert ends.size == R.chunk_plan([f.size], DENSE_PARAMS)[0], name
            assert (np.diff(np.concatenate([[0], ends]))[:-1] == mn).all(), name


@functools.lru_cache(maxsize=None)
def dense():
    files = [_dense(n) for n in DENSE_LENS]
    names = [f"dense{n}" for n in DENSE_LENS]
    cuts = _cuts_of(files, DENSE_PARAMS)
    _assert_full(files, cuts, names)
    counts = _counts(cuts)
    assert counts["chunks"] == R.chunk_plan([f.size for f in files], DENSE_PARAMS)[0]  # the whole call is full
    return _frozen(files), DENSE_PARAMS, {"cuts": cuts, "names": names, "counts": counts}


@functools.lru_cache(maxsize=None)
def dense_mixed():
    rng = _rng(DENSE_PARAMS, 0xC)
    files, names = [], []
    rand_lens = iter((777, 0, 5000, 100, 33, 2049, 1, 4096, 300))
    for n in DENSE_LENS:
        files.append(_rand(rng, next(rand_lens))), names.append(f"random{files[-1].size}")
        files.append(_dense(n)), names.append(f"dense{n}")
        if n > CHANGED_AT:
            files.append(_changed(n)), names.append(f"changed{n}")
    cuts = _cuts_of(files, DENSE_PARAMS)
    _assert_full(files, cuts, names)
    assert names[-1].startswith("changed") and names[-2].startswith("dense") and names[0].startswith("random")
    # a changed file is cut like the dense one up to the change and not after it
    for f, (ends, _), name in zip(files, cuts, names):
        if name.startswith("changed"):
            full = R.cuts(_dense(f.size), DENSE_PARAMS)[0]
            assert ends[:3].tolist() == full[:3].tolist() and ends.tolist() != full.tolist(), name
    return _frozen(files), DENSE_PARAMS, {"cuts": cuts, "names": names, "counts": _counts(cuts)}


# ---- the files of the window-by-window runs --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def streamed(params):
    assert params in STREAMED_PARAMS
    rng = _rng(params, 0xD)
    lens = sweep_lens(params) + [2 * seg_bytes(params) - 1, 4 * seg_bytes(params) + 17]
    files = [_rand(rng, n) for n in lens] + [_dense(2 * seg_bytes(params) + 5), np.zeros(2 * params[2] + 3, np.uint8)]
    names = [f"len{n}" for n in lens] + ["dense", "zeros"]
    cuts = _cuts_of(files, params)
    counts = _counts(cuts)
    assert counts["chunks"] >= 24 and counts["hash_cuts"] and counts["max_cuts"]
    return _frozen(files), params, {"cuts": cuts, "names": names, "counts": counts}
