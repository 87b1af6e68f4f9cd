"""The chunk index's add and the holders index's add place the old entries,
build the directory and write the totals with the same three kernels
(k_ix_place_old, k_ix_dir, k_ix_add_totals in csrc/chunk_index.hip), called
with different arguments from two files. For a batch whose pairs are distinct
and whose already-stored pairs carry their stored value, the two adds are
defined to give the same index; this file pins that they do, byte for byte, at
the sizes where a workgroup of 256 entries begins and ends.

The CPU test checks the cases themselves with the two Python references alone,
so that the GPU test can only fail for the GPU's reasons."""
import functools

import numpy as np
import pytest

from tests import _chunk_holders_ref as H
from tests import _chunk_index_ref as R

N_OLD = (0, 255, 256, 257)
BATCH = (1, 256, 257)
BITS_OLD = (0, 3)
CASES = [(n, m, b) for n in N_OLD for m in BATCH for b in BITS_OLD]
ADD_COUNTS = ("queries", "hits", "added", "batch_duplicates", "entries_old", "entries_new")
FILL = 0xFE


@functools.lru_cache(maxsize=None)
def case(n_old, m, bits_old):
    """-> (old entries, batch keys, digests [m, 32], values, bits_new, the
    reference's (new entries, pos, flags, counts)). Shared: read, never written.

    The old keys ascend in even steps from 2^61 to below 7 * 2^61, so a 3-bit
    directory has entries in six buckets and none in the first and the last.
    About a third of the batch is stored already (entries 0, 255, 256 and the
    last among them, with their stored values); the rest is new: keys below
    entry 0, above the last entry, just below and just above entries 255 and
    256, entry 255's own key with another digest, and keys between other
    entries."""
    rng = np.random.default_rng(1000 * n_old + 10 * m + bits_old)
    step = (6 << 61) // max(n_old, 1)
    old_keys = [(1 << 61) + i * step for i in range(n_old)]
    dig = rng.integers(0, 256, (n_old + m, 32), dtype=np.uint8)
    dig[:, 0] = np.arange(n_old + m) & 0xFF  # distinct digests, whatever the generator gives
    dig[:, 1] = np.arange(n_old + m) >> 8
    old = [(k, dig[i].tobytes(), 1000 + i) for i, k in enumerate(old_keys)]
    assert old == sorted(old)

    n_hits = min(m // 3, n_old)
    edge = [i for i in (0, 255, 256, n_old - 1) if 0 <= i < n_old]
    rest = [int(i) for i in rng.permutation(n_old) if int(i) not in edge]
    hits = (list(dict.fromkeys(edge)) + rest)[:n_hits]
    batch = [old[i] for i in hits]

    def new_key(j):
        kind = j % 8
        if n_old == 0:
            return int(rng.integers(0, 1 << 63)) * 2 + (j & 1)
        if kind == 0:
            return old_keys[0] - 1 - j        # before entry 0
        if kind == 1:
            return old_keys[-1] + 1 + j       # after the last entry
        if kind == 2 and n_old > 255:
            return old_keys[255] - 1 - j      # just below entry 255
        if kind == 3 and n_old > 255:
            return old_keys[255] + 1 + j      # between entries 255 and 256
        if kind == 4 and n_old > 256:
            return old_keys[256] + 1 + j      # just above entry 256
        if kind == 5 and n_old > 255:
            return old_keys[255]              # entry 255's key, another digest
        return old_keys[int(rng.integers(0, n_old))] + 1 + j  # between two other entries

    for j in range(m - len(batch)):
        batch.append((new_key(j), dig[n_old + j].tobytes(), 5000 + j))
    batch = [batch[int(i)] for i in rng.permutation(m)]
    keys, bdig, values = H.batch_arrays(batch)
    bits_new = R.dir_bits(n_old + m)
    return old, keys, bdig, values, bits_new, R.add(old, keys, bdig, values)


@pytest.mark.parametrize("n_old,m,bits_old", CASES)
def test_cases_meet_their_preconditions(n_old, m, bits_old):
    old, keys, dig, values, bits_new, (want, wpos, wflags, wcounts) = case(n_old, m, bits_old)
    assert len(old) == n_old and len(keys) == m
    ps = R.pairs(keys, dig)
    assert len(set(ps)) == m                                    # the pairs are distinct
    stored = {(k, d): v for k, d, v in old}
    hits = [c for c, p in enumerate(ps) if p in stored]
    assert all(int(values[c]) == stored[ps[c]] for c in hits)   # a hit carries the stored value
    assert len(hits) == min(m // 3, n_old) and wcounts["hits"] == len(hits)
    assert wcounts["batch_duplicates"] == 0 and wcounts["entries_new"] == n_old + m - len(hits)
    if n_old and m > 1:
        new_keys = [k for c, (k, _) in enumerate(ps) if c not in set(hits)]
        assert min(new_keys) < old[0][0] and max(new_keys) > old[-1][0]
    if n_old > 256 and m > 8:
        lo, hi = old[255][0], old[256][0]
        assert any(old[254][0] < k < lo for k, _ in ps) and any(lo < k < hi for k, _ in ps)
        assert any(hi < k < hi + (1 << 20) for k, _ in ps)
    # pairs or triples: the same index, places, flags and counts
    hwant, hpos, hflags, hcounts = H.add(old, keys, dig, values)
    assert hwant == want and (hpos == wpos).all() and (hflags == wflags).all() and hcounts == wcounts
    assert H.check(want, R.directory(want, bits_new), bits_new) == (0, None)


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def dev_add(eng, call, old, bits_old, keys, dig, values, bits_new):
    """one device add over guarded buffers -> the bytes of (keys, digests,
    values) up to entries_new, dir, pos, flags and the six counts"""
    import torch

    from tests._guarded import Guarded, guarded_from
    m, n = len(keys), len(old)
    cap = n + m
    ok, od, ov, odir, _ = R.arrays(old, bits_old)
    ins = [guarded_from(ok, align=8), guarded_from(od, align=16), guarded_from(ov, align=8), guarded_from(odir, align=4),
           guarded_from(keys, align=8), guarded_from(dig, align=16), guarded_from(values, align=8)]
    new = [Guarded(8 * cap, align=8, fill=FILL), Guarded(32 * cap, align=16, fill=FILL),
           Guarded(8 * cap, align=8, fill=FILL), Guarded(4 * ((1 << bits_new) + 1), align=4, fill=FILL)]
    outs = [Guarded(8 * m, align=8, fill=FILL), Guarded(m, align=1, fill=FILL), Guarded(48, align=8, fill=FILL)]
    p = lambda g: g.ptr if g.nbytes else 0
    torch.cuda.synchronize()
    call(p(ins[0]), p(ins[1]), p(ins[2]), ins[3].ptr if n else 0, n, bits_old, p(ins[4]), p(ins[5]), p(ins[6]), 0, m,
         p(new[0]), p(new[1]), p(new[2]), new[3].ptr, bits_new, p(outs[0]), p(outs[1]), p(outs[2]))
    eng.dev_sync()
    torch.cuda.synchronize()
    for g in ins + new + outs:
        assert g.check() == []            # the guards are intact
    assert all(g.unchanged() for g in ins)
    counts = [int(x) for x in outs[2].download(np.uint64)]
    e = counts[5]
    assert e <= cap
    for g, size in zip(new[:3], (8, 32, 8)):
        assert g.untouched(size * e)      # nothing past entries_new
    return (new[0].download(np.uint8, 8 * e).tobytes(), new[1].download(np.uint8, 32 * e).tobytes(),
            new[2].download(np.uint8, 8 * e).tobytes(), new[3].download().tobytes(), outs[0].download().tobytes(),
            outs[1].download().tobytes(), counts)


@pytest.mark.gpu
@pytest.mark.parametrize("n_old,m,bits_old", CASES)
def test_both_adds_give_the_same_index(eng, n_old, m, bits_old):
    old, keys, dig, values, bits_new, (want, wpos, wflags, wcounts) = case(n_old, m, bits_old)
    pairs = dev_add(eng, eng.dev_chunk_index_add, old, bits_old, keys, dig, values, bits_new)
    triples = dev_add(eng, eng.dev_chunk_holders_add, old, bits_old, keys, dig, values, bits_new)
    names = ("keys", "digests", "values", "dir", "pos", "flags", "counts")
    for name, a, b in zip(names, pairs, triples):
        assert a == b, name
    wk, wd, wv, wdir, _ = R.arrays(want, bits_new)
    ref = (wk.tobytes(), wd.tobytes(), wv.tobytes(), wdir.tobytes(), wpos.tobytes(), wflags.tobytes(),
           [wcounts[c] for c in ADD_COUNTS])
    for name, a, b in zip(names, pairs, ref):
        assert a == b, name
