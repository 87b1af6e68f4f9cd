"""Test infrastructure: a numpy restatement of the chunk windows (include/sdcas.h
"chunk windows"). The checker of tests/test_gpu_chunk_windows.py;
it never calls the code under test, and tests/test_cdc_win_ref.py pins it
against tests/_cdc_ref.py's whole-file cuts.

next_cut(...)              one step of a chain: (e, kind), or None where a window that is not final stops
window_cuts(x, p, final)   the literal rule of one window -> (ends, kinds, consumed); x holds the window's bytes only
streamed_cuts(x, p, w)     a file in windows of w bytes, each starting at the consumed of the one before
                           (a window that consumed nothing is doubled) -> (ends, kinds, windows)
segmented_cuts(x, p, seg)  the speculate-and-stitch model of one window -> (ends, kinds, consumed, walks, taken):
                           per segment, the cuts the true chain walked and those taken from the segment's own list
window_files(...)          the arrays and counts sdcas_chunk_windows returns for a list of windows
"""
import numpy as np

from tests import _cdc_ref as R

KIND_END, KIND_HASH, KIND_MAX = R.KIND_END, R.KIND_HASH, R.KIND_MAX


def _bits(x, params):
    avg_bits = int(params[1])
    h = R.window_hash(x)
    strict = (h >> np.uint32(32 - (avg_bits + 1))) == 0
    loose = (h >> np.uint32(32 - (avg_bits - 1))) == 0
    return strict, loose


def next_cut(strict, loose, s, W, params, final):
    min_len, avg_bits, max_len = (int(v) for v in params)
    avg = 1 << avg_bits
    left = W - s
    if final and left <= min_len:
        return W, KIND_END
    if not final and left < min_len:
        return None
    hi = min(s + max_len, W)
    mid = min(s + avg, hi + 1)
    cand = np.concatenate([strict[s + min_len - 1:mid - 1], loose[mid - 1:hi]])
    hit = np.flatnonzero(cand)
    if hit.size:
        e = s + min_len + int(hit[0])
        return e, KIND_END if final and e == W else KIND_HASH
    if s + max_len <= W:
        return s + max_len, KIND_END if final and s + max_len == W else KIND_MAX
    return (W, KIND_END) if final else None


def window_cuts(x, params=R.DEFAULT_PARAMS, final=True):
    assert R.params_valid(params), params
    x = np.asarray(x, np.uint8)
    strict, loose = _bits(x, params)
    W, s = int(x.size), 0
    ends, kinds = [], []
    while s < W:
        step = next_cut(strict, loose, s, W, params, final)
        if step is None:
            break
        ends.append(step[0]), kinds.append(step[1])
        s = step[0]
    return np.array(ends, np.int64), np.array(kinds, np.uint8), (W if final else s)


def streamed_cuts(x, params, window_bytes):
    """-> (ends relative to the file, kinds, the number of windows that made progress or were final)"""
    x = np.asarray(x, np.uint8)
    L, pos, want, windows = int(x.size), 0, int(window_bytes), 0
    ends, kinds = [], []
    while True:
        w = x[pos:pos + want]
        final = pos + w.size >= L
        e, k, used = window_cuts(w, params, final)
        if not final and used == 0:
            want *= 2
            continue
        windows += 1
        ends += [pos + int(v) for v in e]
        kinds += [int(v) for v in k]
        if final:
            break
        pos, want = pos + used, int(window_bytes)
    return np.array(ends, np.int64), np.array(kinds, np.uint8), windows


def segmented_cuts(x, params, seg, final=True):
    """One window cut as the device does: a speculative chain per segment of
    seg bytes from the segment's start, and one true chain that walks only
    until it lands on a listed cut. -> (ends, kinds, consumed, walks, taken),
    the last two per segment (empty for a window below 2 * seg)"""
    assert R.params_valid(params) and seg >= 2 * int(params[2])
    x = np.asarray(x, np.uint8)
    strict, loose = _bits(x, params)
    W = int(x.size)
    if W < 2 * seg:
        e, k, used = window_cuts(x, params, final)
        return e, k, used, [], []
    nseg = -(-W // seg)
    lists = []
    for j in range(nseg):
        s, lst = j * seg, []
        while s < W:
            step = next_cut(strict, loose, s, W, params, final)
            if step is None:
                break
            lst.append(step)
            s = step[0]
            if s >= (j + 1) * seg:
                break
        lists.append(lst)
    out, walks, taken = [], [0] * nseg, [0] * nseg
    s = 0
    while s < W:
        j = s // seg
        lst, limit = lists[j], (j + 1) * seg
        stopped = False
        if s == j * seg:
            take = lst
        else:
            take, k = [], 0
            while True:
                step = next_cut(strict, loose, s, W, params, final)
                if step is None:
                    stopped = True
                    break
                out.append(step)
                walks[j] += 1
                s = step[0]
                while k < len(lst) and lst[k][0] < s:
                    k += 1
                if k < len(lst) and lst[k][0] == s:
                    take = lst[k + 1:]
                    break
                if s >= limit:
                    break
        if take:
            out += take
            taken[j] = len(take)
            s = take[-1][0]
        if stopped or s < limit:
            break
    ends = np.array([e for e, _ in out], np.int64)
    kinds = np.array([k for _, k in out], np.uint8)
    return ends, kinds, (W if final else s), walks, taken


def kind_counts(kinds):
    kinds = np.asarray(kinds, np.uint8)
    return {"hash_cuts": int((kinds == KIND_HASH).sum()), "max_cuts": int((kinds == KIND_MAX).sum()),
            "end_chunks": int((kinds == KIND_END).sum())}


def window_files(windows, offsets, finals, params=R.DEFAULT_PARAMS):
    """windows: list of uint8 arrays -> R.chunk_files' dict for windows, with
    "consumed" uint64[n]; counts.files counts the final windows and
    counts.total_bytes is the sum of consumed"""
    fc, off, ln, fl, kd, consumed = [0], [], [], [], [], []
    for i, (x, o, fin) in enumerate(zip(windows, offsets, finals)):
        ends, kinds, used = window_cuts(x, params, bool(fin))
        starts = np.concatenate([[0], ends[:-1]]) if ends.size else ends
        off += [int(o) + int(s) for s in starts]
        ln += [int(e - s) for s, e in zip(starts, ends)]
        fl += [i] * len(ends)
        kd += [int(k) for k in kinds]
        consumed.append(used)
        fc.append(len(off))
    counts = {"files": int(sum(1 for f in finals if f)), "chunks": len(off), "total_bytes": int(sum(consumed)),
              **kind_counts(kd)}
    return {"file_chunks": np.array(fc, np.uint64), "chunk_off": np.array(off, np.uint64),
            "chunk_len": np.array(ln, np.uint64), "chunk_file": np.array(fl, np.uint32),
            "kinds": np.array(kd, np.uint8), "consumed": np.array(consumed, np.uint64), "counts": counts}
