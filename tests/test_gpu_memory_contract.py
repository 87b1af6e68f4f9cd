"""The device API's memory contract (include/sdcas.h, "device-resident"
sections): what each call does to the memory AROUND its arguments.

Every device buffer of every call below is a tests/_guarded.py `Guarded`: its
own allocation with 4 KiB of patterned guard on both sides, the payload at the
alignment the header promises and not a byte more (16 and not 32 for blobs and
digests, 8 and not 16 for u64 arrays, 4 and not 8 for u32 / i32 arrays, an odd
address for byte arrays), outputs sized exactly. Four assertions per call:

  1. the outputs equal the CPU oracle's (bit-exact, no tolerances);
  2. every guard of every input and output is intact after dev_sync;
  3. every input is byte-identical to its snapshot, except the words the
     header names as scratch (the value words of resolve_buckets' received
     records) — an output the call was not given (NULL) costs nothing, and a
     non-NULL one keeps its guards in every NULL combination;
  4. blobs are laid out twice, the bytes between and after the messages 0x00
     and then 0xFF: both results are identical and correct. Messages start at
     addresses that are 16, 32, 48 and 0 mod 64.

Inputs are random bytes from a seeded numpy generator uploaded from the host;
expected values come from the oracle (oracle.hash, oracle.generate_cas_id,
oracle.file_checksum, oracle.identifier_job) and, for the confirm, from the
dict-based group_by of tests/test_gpu_confirm.py.

NOT tested: that a call reads at most 64 bytes past a message's end. Every
payload here has at least 4096 readable bytes behind it, so the over-read the
contract allows lands in guard memory; showing a longer one would need a
buffer at the end of an allocation, i.e. a fault provoked on purpose.

Kernel selection through sdcas_dev_hash_messages: the call sizes its launch by
the reserved workspace's slots, not by the batch, and a small-tile leaf kernel
(71, 73, 84, or the batch-size rule's choice) runs only when the workspace's
tile_first list covers those slots in 128-slot tiles. sdcas_dev_reserve sizes
that list from max_chunks alone, so by the arithmetic of reserve_ws and
batch_hash no reserve gets there: a small-tile variant selected here falls
back to the default 1024-slot kernel. The cases below still select every
variant and reserve on both sides of the 2^14-slot rule, as the other hash
tests do; whichever kernel the library then runs is held to the same
contract. The small-tile kernels write only the library's own staging buffers
(the host-path calls), where no caller memory is at stake.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from spacedrive_amd.dist_dedup import owner_of
from tests._guarded import Guarded, MessageBlob, guarded_from
from tests.test_gpu_confirm import COUNTS, digests_of, group_by
from tests.test_gpu_identify import reserve_for

pytestmark = pytest.mark.gpu

MiB = 1 << 20
ALL_ONES = np.uint64(2**64 - 1)
RESIDUES = [16, 32, 48, 0]
POISONS = (0x00, 0xFF)


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


# ---- plumbing ------------------------------------------------------------------

class Ledger:
    """every guarded buffer of one call (or one chain of calls), by name"""

    def __init__(self):
        self.bufs = {}
        self.inputs = set()

    def inp(self, name, arr, align):
        g = self.bufs[name] = guarded_from(arr, "cuda", align)
        self.inputs.add(name)
        return g

    def out(self, name, nbytes, align):
        g = self.bufs[name] = Guarded(nbytes, "cuda", align)
        return g

    def add(self, name, g, is_input):
        self.bufs[name] = g
        if is_input:
            self.inputs.add(name)
        return g

    def freeze(self, name):
        """an output becomes the next stage's input"""
        self.bufs[name].snapshot()
        self.inputs.add(name)

    def verify(self, what, scratch=()):
        for name, g in self.bufs.items():
            bad = g.check()
            assert not bad, f"{what}: guard of {name} ({g.nbytes} B) changed at offsets {bad[:8]} ({len(bad)} bytes)"
            if name in self.inputs and name not in scratch:
                ch = g.changed()
                assert not ch, f"{what}: input {name} changed at offsets {ch[:8]} ({len(ch)} bytes)"


def P(g):
    return None if g is None else g.ptr


def run(eng, fn, *args, what):
    """one library call on the context's stream, between two full syncs (the
    uploads before it and the downloads after it run on torch's stream)"""
    torch.cuda.synchronize()
    eng._check(fn(eng.ctx, *args, None), what)
    eng.dev_sync()


def u64s(a):
    return np.ascontiguousarray(a, np.uint64)


def key_of(hex32):
    return int(hex32[:16], 16)


# ---- sdcas_dev_hash_messages -------------------------------------------------------

CYCLE = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3 * 1024 + 1]
HASH_LENS = [CYCLE[i % len(CYCLE)] for i in range(129)]
HASH_LENS.insert(40, 130 * 1024 + 5)    # crosses a 128-slot tile
HASH_LENS.insert(90, 1025 * 1024 + 1)   # crosses a 1024-slot tile
HASH_CHUNKS = sum(max(1, -(-x // 1024)) for x in HASH_LENS)


@pytest.fixture(scope="module")
def hash_batch(oracle):
    """(messages, digests hex) of the one batch every hash case runs"""
    assert len(HASH_LENS) == 131 and HASH_CHUNKS + 3 * 131 + 2048 < (1 << 14)
    rng = np.random.default_rng(0x3E3)
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in HASH_LENS]
    return msgs, [oracle.hash(m) for m in msgs]


def hash_call(e, msgs, want, poison, out32=True, keys=True):
    n = len(msgs)
    led = Ledger()
    blob = MessageBlob(msgs, RESIDUES, poison)
    led.add("blob", blob.g, True)
    offs = led.inp("offsets", u64s(blob.offsets), 8)
    lens = led.inp("lens", u64s(blob.lengths), 8)
    o32 = led.out("out32", 32 * n, 16)
    ok = led.out("out_keys", 8 * n, 8)
    run(e, e.L.sdcas_dev_hash_messages, blob.ptr, offs.ptr, lens.ptr, n, P(o32) if out32 else None,
        P(ok) if keys else None, what="dev_hash_messages")
    led.verify(f"dev_hash_messages poison {poison:#x} out32={out32} keys={keys}")
    d, k = o32.download().reshape(n, 32), ok.download(np.uint64)
    if out32:
        bad = [i for i in range(n) if bytes(d[i]).hex() != want[i]]
        assert not bad, f"digests of messages {bad[:8]} (lengths {[len(msgs[i]) for i in bad[:8]]}), poison {poison:#x}"
    else:
        assert o32.untouched(), "a digest was written though d_out32 was not passed"
    if keys:
        bad = [i for i in range(n) if int(k[i]) != key_of(want[i])]
        assert not bad, f"keys of messages {bad[:8]} (lengths {[len(msgs[i]) for i in bad[:8]]}), poison {poison:#x}"
    else:
        assert ok.untouched(), "a key was written though d_out_keys was not passed"
    return d, k


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("variant,finish", [(None, "quad"), (52, "quad"), (67, "quad"), (71, "quad"), (73, "quad"),
                                            (84, "quad"), (67, "lane"), (73, "lane"), (84, "lane")])
def test_hash_messages(hash_batch, variant, finish, sort, side, monkeypatch):
    """131 messages (more than a 128-slot tile of single-chunk ones, no
    multiple of 64) with lengths around a block, a chunk and both tile sizes,
    per leaf variant, finish kernel, slot order and side of the 2^14-slot
    workspace rule"""
    from spacedrive_amd import Engine
    msgs, want = hash_batch
    if finish == "lane":
        monkeypatch.setenv("SDCAS_FINISH", "lane")
    with Engine() as e:
        if variant is not None:
            assert e.dev_set_leaf_variant(variant)
        if not sort:
            e.dev_set_sort(0)
        e.dev_reserve(len(msgs), HASH_CHUNKS if side == "below" else 4 * (1 << 14))
        a = hash_call(e, msgs, want, 0x00)
        b = hash_call(e, msgs, want, 0xFF)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        hash_call(e, msgs, want, 0xFF, keys=False)
        hash_call(e, msgs, want, 0x00, out32=False)


# ---- sdcas_dev_identify and the host path over the same files ------------------------

WHOLE = [0, 1, 56, 57, 1016, 1017, 1024, 102399, 102400]
# sampled lengths by the residue of the sample spacing mod 16: length -> (jump, jump % 16)
SAMPLED = {102404: (21505, 1), 102407: (21505, 1), 102408: (21506, 2), 102416: (21508, 4), 102432: (21512, 8),
           102460: (21519, 15), 1048596: (258053, 5), 3 * 2**20 + 17: (782340, 4)}
# interleaved, so that several sampled files share a batch with whole-file ones
IDENTIFY_LENS = [x for pair in itertools.zip_longest(WHOLE, SAMPLED) for x in pair if x is not None]
HOST_LENS = list(SAMPLED) + [1017, 102400]


def check_sample_spacing():
    """plain arithmetic, before anything touches the GPU: a typo in a length
    cannot quietly bring the 16-byte-aligned sample windows back"""
    for size, (jump, res) in SAMPLED.items():
        assert size > 102400 and (size - 16384) // 4 == jump and jump % 16 == res and res != 0, size
    assert (102407 - 8192) % 8 == 7  # the footer of this one starts at 7 mod 8
    assert sorted(j % 16 for j, _ in SAMPLED.values()) == [1, 1, 2, 4, 4, 5, 8, 15]
    assert len(IDENTIFY_LENS) == len(WHOLE) + len(SAMPLED)


@pytest.fixture(scope="module")
def files(oracle, tmp_path_factory):
    """every identify length as a real file of random bytes -> {length:
    (path, bytes, cas key or None, checksum hex)}, the expected values from
    the oracle's generate_cas_id(path, size) and file_checksum(path)"""
    check_sample_spacing()
    root = tmp_path_factory.mktemp("contract")
    rng = np.random.default_rng(0x1D)
    out = {}
    for size in IDENTIFY_LENS:
        data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        path = str(root / f"f{size}.bin")
        with open(path, "wb") as f:
            f.write(data)
        key = int(oracle.generate_cas_id(path, size), 16) if size else None
        out[size] = (path, data, key, oracle.file_checksum(path))
    return out


def identify_call(e, files, sizes, poison, keys=True, out32=True, has_key=True):
    n = len(sizes)
    led = Ledger()
    blob = MessageBlob([files[s][1] for s in sizes], RESIDUES, poison)
    led.add("blob", blob.g, True)
    offs = led.inp("offsets", u64s(blob.offsets), 8)
    lens = led.inp("lens", u64s(sizes), 8)
    ok = led.out("out_keys", 8 * n, 8)
    o32 = led.out("out32", 32 * n, 16)
    oh = led.out("has_key", n, 1)
    reserve_for(e, sizes)
    run(e, e.L.sdcas_dev_identify, blob.ptr, offs.ptr, lens.ptr, n, P(ok) if keys else None, P(o32) if out32 else None,
        P(oh) if has_key else None, what="dev_identify")
    what = f"dev_identify of {sizes if n < 4 else n} poison {poison:#x} keys={keys} out32={out32} has_key={has_key}"
    led.verify(what)
    k, d, h = ok.download(np.uint64), o32.download().reshape(n, 32), oh.download()
    for i, s in enumerate(sizes):
        _, _, wk, wd = files[s]
        if has_key:
            assert h[i] == (1 if s else 0), (what, i, s)
        if keys and s:
            assert f"{int(k[i]):016x}" == f"{wk:016x}", f"{what}: cas key of file {i}, {s} bytes"
        if out32:
            assert bytes(d[i]).hex() == wd, f"{what}: checksum of file {i}, {s} bytes"
    if not keys:
        assert ok.untouched(), f"{what}: a key was written though d_out_keys was not passed"
    if not out32:
        assert o32.untouched(), f"{what}: a digest was written though d_out32 was not passed"
    if not has_key:
        assert oh.untouched(), f"{what}: has_key was written though it was not passed"
    return k, d, h


def test_identify_batch(eng, files):
    """whole-file lengths around the two messages' block and chunk edges,
    interleaved with sampled files whose sample spacing is 1, 2, 4, 5, 8 and
    15 mod 16: the gather reads its four sample windows at addresses of every
    alignment"""
    a = identify_call(eng, files, IDENTIFY_LENS, 0x00)
    b = identify_call(eng, files, IDENTIFY_LENS, 0xFF)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    rev = IDENTIFY_LENS[::-1]
    identify_call(eng, files, rev, 0xFF)


@pytest.mark.parametrize("combo", [c for c in itertools.product([True, False], repeat=3) if not all(c)])
def test_identify_null_outputs(eng, files, combo):
    keys, out32, has_key = combo
    identify_call(eng, files, IDENTIFY_LENS, 0xFF, keys=keys, out32=out32, has_key=has_key)


@pytest.mark.parametrize("size", list(SAMPLED))
def test_identify_sampled_alone(eng, files, size):
    a = identify_call(eng, files, [size], 0x00)
    b = identify_call(eng, files, [size], 0xFF)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("direct_io", [True, False])
def test_odd_sample_windows_on_real_files(files, direct_io):
    """the host path's reads of the same sample windows: with O_DIRECT they
    start and end off the 4 KiB grid and go through the bounce buffer; keys and
    digests of the three path calls against the oracle"""
    from spacedrive_amd import Engine
    paths = [files[s][0] for s in HOST_LENS]
    want_k = [files[s][2] for s in HOST_LENS]
    want_d = [files[s][3] for s in HOST_LENS]
    both = N.SDCAS_META_HAS_CAS_ID | N.SDCAS_META_HAS_CHECKSUM
    with Engine(direct_io=direct_io) as e:
        keys, st = e.generate_cas_ids(paths, HOST_LENS)
        assert not st.any(), st
        assert [int(k) for k in keys] == want_k, "generate_cas_ids"
        sizes, keys, dig, st, fl = e.identify_checksums(paths)
        assert not st.any() and (fl == both).all() and [int(s) for s in sizes] == HOST_LENS
        assert [int(k) for k in keys] == want_k, "identify_checksums keys"
        assert [bytes(d).hex() for d in dig] == want_d, "identify_checksums digests"
        sizes, keys, st, fl = e.file_metadata(paths)
        assert not st.any() and (fl == N.SDCAS_META_HAS_CAS_ID).all() and [int(s) for s in sizes] == HOST_LENS
        assert [int(k) for k in keys] == want_k, "file_metadata"


# ---- sdcas_dev_stream_begin / _update / _finish ----------------------------------------

STREAM_LENS = [2**20 + 1, 2 * 2**20 + 1023, 3 * 2**20]


@pytest.fixture(scope="module")
def stream_files(oracle):
    rng = np.random.default_rng(0x57)
    data = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in STREAM_LENS]
    return data, [oracle.hash(d) for d in data]


@pytest.mark.parametrize("variant", [17, 19])
def test_stream_session(stream_files, variant):
    """three files cut into 1 MiB segments, each segment at its own place
    (16 mod 64) in one guarded blob with poison after it — after each file's
    ragged last segment too — delivered shuffled over two update calls"""
    from spacedrive_amd import Engine
    data, want = stream_files
    segs = [(f, o, min(MiB, len(d) - o)) for f, d in enumerate(data) for o in range(0, len(d), MiB)]
    order = np.random.default_rng(variant).permutation(len(segs))
    segs = [segs[i] for i in order]
    assert len(segs) == 8 and sorted(l for _, _, l in segs)[:2] == [1, 1023]
    got = []
    with Engine() as e:
        assert e.dev_set_piece_variant(variant)
        for poison in POISONS:
            led = Ledger()
            blob = MessageBlob([data[f][o:o + l] for f, o, l in segs], [16], poison)
            led.add("blob", blob.g, True)
            addrs = blob.addresses()
            assert all(a % 64 == 16 for a in addrs)
            out = led.out("out32", 32 * len(data), 16)
            torch.cuda.synchronize()
            e.dev_stream_begin(STREAM_LENS)
            for part in (slice(0, 3), slice(3, None)):
                sg = segs[part]
                e.dev_stream_update([f for f, _, _ in sg], [o for _, o, _ in sg], [l for _, _, l in sg], addrs[part])
            e.dev_stream_finish(out.ptr)
            e.dev_sync()
            led.verify(f"stream session, piece variant {variant}, poison {poison:#x}")
            d = out.download().reshape(len(data), 32)
            assert [bytes(x).hex() for x in d] == want, (variant, poison)
            got.append(d)
    assert np.array_equal(got[0], got[1])


# ---- alignment: rejected before anything is enqueued ------------------------------------

def _invalid(e, rc):
    with pytest.raises(N.SdcasError) as ei:
        e._check(rc, "call")
    assert ei.value.code == N.SDCAS_E_INVALID, ei.value


def test_misaligned_pointers_are_rejected(eng, hash_batch):
    """d_blob / d_out32 off 16 bytes and d_out_keys off 8 bytes: hash_messages,
    identify and stream_finish return SDCAS_E_INVALID and no kernel runs — the
    outputs keep their prefill"""
    msgs, _ = hash_batch
    msgs = msgs[:8]
    n = len(msgs)
    led = Ledger()
    blob = MessageBlob(msgs, RESIDUES, 0xA5)
    led.add("blob", blob.g, True)
    offs = led.inp("offsets", u64s(blob.offsets), 8)
    lens = led.inp("lens", u64s(blob.lengths), 8)
    # room for the shifted pointers: nothing may be written either way
    o32 = led.out("out32", 32 * n + 16, 16)
    ok = led.out("out_keys", 8 * n + 8, 8)
    oh = led.out("has_key", n, 1)
    eng.dev_reserve(n, 4096)
    reserve_for(eng, blob.lengths)
    torch.cuda.synchronize()
    L, ctx = eng.L, eng.ctx
    for d in (8, 4):
        _invalid(eng, L.sdcas_dev_hash_messages(ctx, blob.ptr + d, offs.ptr, lens.ptr, n, o32.ptr, ok.ptr, None))
        _invalid(eng, L.sdcas_dev_hash_messages(ctx, blob.ptr, offs.ptr, lens.ptr, n, o32.ptr + d, ok.ptr, None))
        _invalid(eng, L.sdcas_dev_hash_messages(ctx, blob.ptr, offs.ptr, lens.ptr, n, o32.ptr + d, None, None))
        _invalid(eng, L.sdcas_dev_identify(ctx, blob.ptr + d, offs.ptr, lens.ptr, n, ok.ptr, o32.ptr, oh.ptr, None))
        _invalid(eng, L.sdcas_dev_identify(ctx, blob.ptr, offs.ptr, lens.ptr, n, ok.ptr, o32.ptr + d, oh.ptr, None))
        _invalid(eng, L.sdcas_dev_identify(ctx, blob.ptr, offs.ptr, lens.ptr, n, None, o32.ptr + d, None, None))
    # u64 keys: 8 bytes off is still aligned, 4 is not
    _invalid(eng, L.sdcas_dev_hash_messages(ctx, blob.ptr, offs.ptr, lens.ptr, n, o32.ptr, ok.ptr + 4, None))
    _invalid(eng, L.sdcas_dev_hash_messages(ctx, blob.ptr, offs.ptr, lens.ptr, n, None, ok.ptr + 4, None))
    _invalid(eng, L.sdcas_dev_identify(ctx, blob.ptr, offs.ptr, lens.ptr, n, ok.ptr + 4, o32.ptr, oh.ptr, None))
    eng.dev_stream_begin([2 * MiB])
    for d in (8, 4):
        _invalid(eng, L.sdcas_dev_stream_finish(ctx, o32.ptr + d, None))
    eng.dev_stream_finish(o32.ptr)  # the session was left open: an aligned finish closes it (no update: no content)
    eng.dev_sync()
    led.verify("misaligned calls")
    assert ok.untouched() and oh.untouched() and o32.untouched(32), "a rejected call wrote an output"
    # NULL outputs stay legal, and 8 bytes off is a legal d_out_keys
    run(eng, L.sdcas_dev_hash_messages, blob.ptr, offs.ptr, lens.ptr, n, None, ok.ptr + 8, what="keys + 8")
    led.verify("keys at + 8")
    assert ok.untouched(0, 8) and not ok.untouched(8)


# ---- sdcas_dev_confirm_duplicates ---------------------------------------------------------

def confirm_corpus(n):
    """keys from a small pool, one digest per key except one key that carries
    two, some files masked out"""
    rng = np.random.default_rng(n)
    kid = rng.integers(0, max(1, n // 3), n)
    did = kid * 8
    if n > 1:
        kid[-1] = kid[0]
        did[-1] = kid[0] * 8 + 1  # the same key, another digest
    keys = (kid.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    valid = (rng.random(n) > 0.2).astype(np.uint8)
    valid[[0, -1]] = 1
    if n > 2:
        valid[1] = 0
    return keys, digests_of(did), valid


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_confirm_duplicates(eng, n, masked):
    keys, dig, valid = confirm_corpus(n)
    want = group_by(keys, dig, valid if masked else None)
    combos = list(itertools.product([True, False], repeat=4)) if (n == 65 and masked) else [(True,) * 4]
    for outs in combos:
        led = Ledger()
        k = led.inp("keys", keys, 8)
        d = led.inp("digests", dig, 16)
        v = led.inp("valid", valid, 1) if masked else None
        rep = led.out("rep", 8 * n, 8)
        krep = led.out("key_rep", 8 * n, 8)
        fl = led.out("flags", n, 1)
        cnt = led.out("counts", 48, 8)
        o = [P(g) if on else None for g, on in zip((rep, krep, fl, cnt), outs)]
        run(eng, eng.L.sdcas_dev_confirm_duplicates, k.ptr, d.ptr, P(v), n, *o, what="dev_confirm_duplicates")
        what = f"dev_confirm_duplicates n={n} masked={masked} outputs={outs}"
        led.verify(what)
        got = (rep.download(np.int64), krep.download(np.int64), fl.download(),
               dict(zip(COUNTS, (int(x) for x in cnt.download(np.uint64)))))
        for g, on, gv, wv, name in zip((rep, krep, fl, cnt), outs, got, want, ("rep", "key_rep", "flags", "counts")):
            if not on:
                assert g.untouched(), f"{what}: {name} was written though it was not passed"
            elif isinstance(wv, dict):
                assert gv == wv, f"{what}: {gv} != {wv}"
            else:
                assert np.array_equal(gv, wv), f"{what}: {name} differs at {np.flatnonzero(gv != wv)[:8]}"


# ---- dedup ----------------------------------------------------------------------------------

DEDUP_N = [1, 63, 65, 2049, 4097]  # around a wave and around the 2048 / 4096-row tiles
DEDUP_CS = [100, 7]
DEDUP_NE = [0, 1, 65]


def dedup_corpus(n, ne):
    """keys from a small pool that holds the tables' empty marker (all ones)
    and 0; a few rows without cas_id and a few errored ones, the last row
    among them; existing Objects from the same pool"""
    rng = np.random.default_rng(1000 * n + ne)
    pool = np.concatenate([np.array([ALL_ONES, 0], np.uint64), rng.integers(0, 2**64, max(2, n // 4), dtype=np.uint64)])
    keys = pool[rng.integers(0, pool.size, n)]
    if n >= 4:
        keys[[0, n // 2]] = ALL_ONES
        keys[[1, n - 3]] = 0
    has = np.ones(n, np.uint8)
    status = np.zeros(n, np.int32)
    pick = np.unique(rng.integers(0, n, max(1, n // 16)))
    has[pick[::2]] = 0
    status[pick[1::2]] = 5
    has[n - 1] = 0
    status[n - 1] = 0
    if n >= 2:
        status[n - 2] = 5
    existing = pool[rng.integers(0, pool.size, ne)]
    if ne:
        existing[0] = ALL_ONES
    return keys, has, status, existing


def rank_inputs(led, r, keys, has, status, lo, hi):
    return (led.inp(f"keys{r}", keys[lo:hi], 8), led.inp(f"has_key{r}", has[lo:hi], 1),
            led.inp(f"status{r}", status[lo:hi], 4), led.inp(f"ids{r}", np.arange(lo, hi, dtype=np.uint64), 8))


@pytest.mark.parametrize("ne", DEDUP_NE)
@pytest.mark.parametrize("chunk_size", DEDUP_CS)
@pytest.mark.parametrize("n", DEDUP_N)
def test_dedup_one_call(eng, oracle, n, chunk_size, ne):
    """sdcas_dev_dedup_local (with and without the plan header) and the
    device dedup Engine.dev_dedup wraps (with and without counts)"""
    keys, has, status, existing = dedup_corpus(n, ne)
    want, wc, wl, ww = oracle.identifier_job(keys, has, status, chunk_size, existing)
    L = eng.L
    for header in (True, False):
        led = Ledger()
        k, h, s, ids = rank_inputs(led, 0, keys, has, status, 0, n)
        ek = led.inp("existing keys", existing, 8)
        ei = led.inp("existing ids", np.arange(ne, dtype=np.uint64), 8)
        link = led.out("link", 8 * n, 8)
        cnt = led.out("counts", 16, 8).upload(np.zeros(2, np.uint64))
        hd = led.out("plan header", 8 * N.SDCAS_PLAN_HEADER_WORDS, 8)
        run(eng, L.sdcas_dev_dedup_local, k.ptr, h.ptr, s.ptr, ids.ptr, n, ek.ptr if ne else None,
            ei.ptr if ne else None, ne, chunk_size, 0, 0, 0, link.ptr, cnt.ptr, hd.ptr if header else None,
            what="dev_dedup_local")
        what = f"dev_dedup_local n={n} cs={chunk_size} ne={ne} header={header}"
        led.verify(what)
        assert np.array_equal(link.download(np.int64), want), what
        assert tuple(int(x) for x in cnt.download(np.uint64)) == (wc, wl), what
        if header:
            w = hd.download(np.uint64)
            assert (int(w[2]), int(w[3]), int(w[8])) == (ww["steps"], ww["rows"], ww["rereads"]), what
        else:
            assert hd.untouched(), f"{what}: the plan header was written though it was not passed"
    if ne:
        return
    for counts in (True, False):
        led = Ledger()
        k, h, s, _ = rank_inputs(led, 0, keys, has, status, 0, n)
        link = led.out("link", 8 * n, 8)
        cnt = led.out("counts", 16, 8)
        run(eng, L.sdcas_dev_dedup, k.ptr, h.ptr, s.ptr, n, chunk_size, link.ptr, cnt.ptr if counts else None,
            what="dev_dedup")
        what = f"dev_dedup n={n} cs={chunk_size} counts={counts}"
        led.verify(what)
        assert np.array_equal(link.download(np.int64), want), what
        if counts:
            assert tuple(int(x) for x in cnt.download(np.uint64)) == (wc, wl), what
        else:
            assert cnt.untouched(), f"{what}: counts were written though they were not passed"


def stays_and_plan(eng, led, ranks, keys, has, status, cuts, chunk_size, window):
    """stays of every rank (d_stays[cap], the padding checked up to cap
    exactly), gathered on the host, one plan of SDCAS_PLAN_WORDS(n_stays)"""
    L = eng.L
    n = keys.size
    gathered = []
    for r, (k, h, s, ids) in enumerate(ranks):
        lo, hi = cuts[r], cuts[r + 1]
        stay = np.arange(lo, hi, dtype=np.uint64)[(has[lo:hi] == 0) | (status[lo:hi] != 0)]
        cap = stay.size + 3
        out = led.out(f"stays{r}", 8 * cap, 8)
        cnt = led.out(f"stays count{r}", 8, 8)
        run(eng, L.sdcas_dev_dedup_stays, h.ptr, s.ptr, ids.ptr, hi - lo, cap, out.ptr, cnt.ptr, what="dedup_stays")
        got = out.download(np.uint64)
        assert np.array_equal(got[:stay.size], stay), f"stays of rank {r}"
        assert (got[stay.size:] == ALL_ONES).all(), f"stays padding of rank {r}: {got[stay.size:]}"
        assert int(cnt.download(np.int64)[0]) == stay.size
        gathered.append(got)
    gathered = np.concatenate(gathered)
    ds = led.inp("gathered stays", gathered, 8)
    plan = led.out("plan", 8 * (N.SDCAS_PLAN_HEADER_WORDS + gathered.size), 8)
    run(eng, L.sdcas_dev_dedup_plan, ds.ptr, gathered.size, n, chunk_size, 0, 0, plan.ptr, what="dedup_plan")
    w = plan.download(np.uint64)
    assert (int(w[2]), int(w[3]), int(w[8])) == (window["steps"], window["rows"], window["rereads"])
    assert (int(w[4]), int(w[5])) == (n, chunk_size)
    led.freeze("plan")
    return plan


def apply_all(eng, led, ranks, slots, results, cuts, chunk_size, plan, want, wc, wl, what):
    links, created, linked = [], 0, 0
    for r, (k, h, s, ids) in enumerate(ranks):
        m = cuts[r + 1] - cuts[r]
        link = led.out(f"link{r}", 8 * m, 8)
        cnt = led.out(f"counts{r}", 16, 8).upload(np.zeros(2, np.uint64))
        run(eng, eng.L.sdcas_dev_dedup_apply, ids.ptr, slots[r].ptr, m, results[r].ptr, chunk_size, plan.ptr, link.ptr,
            cnt.ptr, what="dedup_apply")
        links.append(link.download(np.int64))
        c = cnt.download(np.uint64)
        created += int(c[0])
        linked += int(c[1])
    led.verify(what)
    got = np.concatenate(links)
    assert np.array_equal(got, want), f"{what}: links differ at {np.flatnonzero(got != want)[:8]}"
    assert (created, linked) == (wc, wl), what


def slot_codes(slot, has, status, lo, hi, what):
    s = slot.download(np.uint32)
    ok = status[lo:hi] == 0
    assert (s[~ok] == 0xFFFFFFFE).all(), f"{what}: slot of a dropped file"
    assert (s[ok & (has[lo:hi] == 0)] == 0xFFFFFFFF).all(), f"{what}: slot of a file without cas_id"
    assert (s[ok & (has[lo:hi] != 0)] < 0xFFFFFFFE).all(), f"{what}: slot of a keyed file"


@pytest.mark.parametrize("ne", DEDUP_NE)
@pytest.mark.parametrize("chunk_size", DEDUP_CS)
@pytest.mark.parametrize("n", DEDUP_N)
@pytest.mark.parametrize("world,combine", [(1, "sync"), (1, "async"), (3, "sync"), (3, "async")])
def test_dedup_exact_stages(eng, oracle, world, combine, n, chunk_size, ne):
    """stays -> plan -> combine (or combine_async) -> resolve -> apply over
    `world` virtual ranks, the exchanges done on the host between guarded
    buffers; resolve's received records must come back unchanged"""
    keys, has, status, existing = dedup_corpus(n, ne)
    want, wc, wl, ww = oracle.identifier_job(keys, has, status, chunk_size, existing)
    what = f"exact stages world={world} {combine} n={n} cs={chunk_size} ne={ne}"
    L = eng.L
    led = Ledger()
    cuts = [n * r // world for r in range(world + 1)]
    ranks = [rank_inputs(led, r, keys, has, status, cuts[r], cuts[r + 1]) for r in range(world)]
    plan = stays_and_plan(eng, led, ranks, keys, has, status, cuts, chunk_size, ww)

    def combine_one(tag, k, h, s, ids, m, want_slot):
        """-> (records uint64[U, 2] on the host, the slot buffer, starts)"""
        rec = led.out(f"rec {tag}", 16 * m, 8)
        slot = led.out(f"slot {tag}", 4 * m, 4) if want_slot else None
        if combine == "sync":
            starts = (ctypes.c_uint64 * (world + 1))()
            run(eng, L.sdcas_dev_dedup_combine, P(k), P(h), P(s), P(ids), m, world, rec.ptr, P(slot), starts,
                what="dedup_combine")
            st = [int(x) for x in starts]
        else:
            ds = led.out(f"starts {tag}", 4 * (world + 1), 4)
            run(eng, L.sdcas_dev_dedup_combine_async, P(k), P(h), P(s), P(ids), m, world, rec.ptr, P(slot), ds.ptr,
                what="dedup_combine_async")
            st = [int(x) for x in ds.download(np.uint32)]
        assert st[0] == 0 and all(a <= b for a, b in zip(st, st[1:])) and st[world] <= m, (what, tag, st)
        return rec.download(np.uint64).reshape(m, 2)[:st[world]], slot, st

    recs, slots, starts = [], [], []
    for r, (k, h, s, ids) in enumerate(ranks):
        rec, slot, st = combine_one(f"files{r}", k, h, s, ids, cuts[r + 1] - cuts[r], True)
        slot_codes(slot, has, status, cuts[r], cuts[r + 1], what)
        led.freeze(f"slot files{r}")
        recs.append(rec)
        slots.append(slot)
        starts.append(st)
    erecs, estarts = [], []
    for r in range(world):
        idx = np.arange(r, ne, world, dtype=np.uint64)
        ek = led.inp(f"existing keys{r}", existing[idx.astype(np.int64)], 8)
        ei = led.inp(f"existing ids{r}", idx, 8)
        rec, _, st = combine_one(f"existing{r}", ek, None, None, ei, idx.size, False)
        erecs.append(rec)
        estarts.append(st)
    led.verify(what + " (combine)")
    # the exchange: owner d receives every rank's records of its range, in rank order
    answers = []
    for d in range(world):
        f = np.concatenate([recs[s][starts[s][d]:starts[s][d + 1]] for s in range(world)])
        e = np.concatenate([erecs[s][estarts[s][d]:estarts[s][d + 1]] for s in range(world)])
        assert (owner_of(f[:, 0], world) == d).all(), f"{what}: a record outside owner {d}'s range"
        frec = led.inp(f"received files{d}", f, 8)
        erec = led.inp(f"received existing{d}", e, 8)
        res = led.out(f"result{d}", 8 * f.shape[0], 8)
        run(eng, L.sdcas_dev_dedup_resolve, frec.ptr, f.shape[0], erec.ptr if e.shape[0] else None, e.shape[0],
            res.ptr, what="dedup_resolve")
        answers.append(res.download(np.int64))
    led.verify(what + " (resolve)")
    # and back: rank s's answers in its send order
    results = []
    for s in range(world):
        back = np.zeros(starts[s][world], np.int64)
        for d in range(world):
            off = sum(starts[t][d + 1] - starts[t][d] for t in range(s))
            cnt = starts[s][d + 1] - starts[s][d]
            back[starts[s][d]:starts[s][d + 1]] = answers[d][off:off + cnt]
        results.append(led.inp(f"answers{s}", back, 8))
    apply_all(eng, led, ranks, slots, results, cuts, chunk_size, plan, want, wc, wl, what)


@pytest.mark.parametrize("ne", DEDUP_NE)
@pytest.mark.parametrize("chunk_size", DEDUP_CS)
@pytest.mark.parametrize("n", DEDUP_N)
def test_dedup_bucket_stages(eng, oracle, n, chunk_size, ne):
    """stays -> plan -> combine_buckets -> resolve_buckets -> apply at world 3
    with buckets that do not overflow; resolve_buckets may overwrite the value
    word of a valid received record and nothing else"""
    world = 3
    keys, has, status, existing = dedup_corpus(n, ne)
    want, wc, wl, ww = oracle.identifier_job(keys, has, status, chunk_size, existing)
    what = f"bucket stages n={n} cs={chunk_size} ne={ne}"
    L = eng.L
    led = Ledger()
    cuts = [n * r // world for r in range(world + 1)]
    ranks = [rank_inputs(led, r, keys, has, status, cuts[r], cuts[r + 1]) for r in range(world)]
    plan = stays_and_plan(eng, led, ranks, keys, has, status, cuts, chunk_size, ww)
    fcap = max(cuts[r + 1] - cuts[r] for r in range(world)) + 1
    ecap = -(-ne // world) + 1 if ne else 0

    def combine_one(tag, k, h, s, ids, m, cap, want_slot):
        """-> (send uint64[world * cap, 2] on the host, the slot buffer, counts)"""
        send = led.out(f"send {tag}", 16 * world * cap, 8)
        slot = led.out(f"slot {tag}", 4 * m, 4) if want_slot else None
        cnt = led.out(f"counts {tag}", 8 * world, 8)
        over = led.out(f"overflow {tag}", 4, 4)
        run(eng, L.sdcas_dev_dedup_combine_buckets, P(k), P(h), P(s), P(ids), m, world, cap, send.ptr, P(slot), cnt.ptr,
            over.ptr, what="dedup_combine_buckets")
        assert int(over.download(np.uint32)[0]) == 0, f"{what}: {tag} overflowed"
        c = cnt.download(np.int64)
        assert ((c >= 0) & (c <= cap)).all(), (what, tag, c)
        return send.download(np.uint64).reshape(world * cap, 2), slot, c

    sends, slots, fcnt = [], [], []
    for r, (k, h, s, ids) in enumerate(ranks):
        send, slot, c = combine_one(f"files{r}", k, h, s, ids, cuts[r + 1] - cuts[r], fcap, True)
        slot_codes(slot, has, status, cuts[r], cuts[r + 1], what)
        led.freeze(f"slot files{r}")
        sends.append(send)
        slots.append(slot)
        fcnt.append(c)
    esends, ecnt = [], []
    for r in range(world):
        if not ne:
            break
        idx = np.arange(r, ne, world, dtype=np.uint64)
        ek = led.inp(f"existing keys{r}", existing[idx.astype(np.int64)], 8)
        ei = led.inp(f"existing ids{r}", idx, 8)
        send, _, c = combine_one(f"existing{r}", ek, None, None, ei, idx.size, ecap, False)
        esends.append(send)
        ecnt.append(c)
    # the equal-split exchange: owner d receives bucket d of every rank, in rank order
    answers = []
    for d in range(world):
        f = np.concatenate([sends[s][d * fcap:(d + 1) * fcap] for s in range(world)])
        fc = np.array([fcnt[s][d] for s in range(world)], np.int64)
        frec = led.inp(f"received files{d}", f, 8)
        dfc = led.inp(f"received file counts{d}", fc, 8)
        if ne:
            e = np.concatenate([esends[s][d * ecap:(d + 1) * ecap] for s in range(world)])
            ec = np.array([ecnt[s][d] for s in range(world)], np.int64)
            erec = led.inp(f"received existing{d}", e, 8)
            dec = led.inp(f"received existing counts{d}", ec, 8)
        else:
            erec = dec = None
        res = led.out(f"result{d}", 8 * world * fcap, 8)
        run(eng, L.sdcas_dev_dedup_resolve_buckets, frec.ptr, fcap, dfc.ptr, P(erec), ecap, P(dec), world, res.ptr,
            what="dedup_resolve_buckets")
        # scratch: the value word (bytes 8..15) of a valid record, nothing else
        for g, cap, cnts in ((frec, fcap, fc), (erec, ecap, ec if ne else None)):
            if g is None:
                continue
            for off in g.changed():
                p = off // 16
                assert off % 16 >= 8 and p % cap < cnts[p // cap], \
                    f"{what}: resolve_buckets changed byte {off} of owner {d}'s received records"
        for s in range(world):
            assert res.untouched(8 * (s * fcap + int(fc[s])), 8 * (s + 1) * fcap), f"{what}: result padding written"
        answers.append(res.download(np.int64).reshape(world, fcap))
    scratch = [f"received files{d}" for d in range(world)] + [f"received existing{d}" for d in range(world)]
    led.verify(what + " (resolve)", scratch=scratch)
    results = [led.inp(f"answers{s}", np.concatenate([answers[d][s] for d in range(world)]), 8) for s in range(world)]
    for name in scratch:  # checked above; apply does not see them
        led.inputs.discard(name)
    apply_all(eng, led, ranks, slots, results, cuts, chunk_size, plan, want, wc, wl, what)
