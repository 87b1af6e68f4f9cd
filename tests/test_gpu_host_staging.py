"""Every host-array entry point (sdcas_dedup_window, sdcas_confirm_duplicates,
sdcas_duplicate_sets, sdcas_tree_digests, sdcas_tree_top, sdcas_chunk_messages,
sdcas_chunk_windows, sdcas_chunk_sharing and the index calls) copies its arrays
into ONE device buffer of the context (sdcas_ctx::host_io, laid out by Parts in
csrc/sdcas_api.hip). What that sharing could break is pinned here: a call that
reads an unlike earlier call's stale bytes, a buffer that grows (or does not)
between unlike calls, an optional array that is off while its neighbours are
on, and byte-sized parts that end off a 16-byte boundary.

The inputs and the references' answers are in tests/_host_staging_cases.py;
the CPU test checks that those inputs are not degenerate, by the references
alone, so that the GPU tests cannot pass on empty results. Every output array
and every count is compared in full."""
import ctypes

import numpy as np
import pytest

from spacedrive_amd import _native as N
from tests import _chunk_index_ref as R
from tests import _host_staging_cases as K

FILL = 0xEE


def test_cases_are_not_degenerate(oracle):
    for n in (3, 5000) + K.EDGES:
        keys, dig, valid, (rep, key_rep, flags, counts) = K.confirm_case(n) if n != 5000 else K.big_confirm_case()
        assert keys.size == n and counts["files"] == n - (valid is not None and n > 2)
        if n >= 4 or (n >= 2 and valid is None) or n == 2:
            assert counts["duplicate_files"] >= 1                      # a duplicate class
    assert K.big_confirm_case()[3][3]["collided_keys"] >= 1
    for n in (2,) + K.EDGES:
        rep, sizes, (set_rep, offs, set_bytes, members, counts) = K.sets_case(n)
        assert counts["sets"] == (n // 2 if n <= 2 else (n - 2) // 2) and members.size == counts["members"]
    assert K.sets_case(2)[2][4]["sets"] == 1 and K.sets_case(17)[2][4]["sets"] == 7  # a set; an odd count of sets
    for n in (1000,) + K.EDGES:
        parent, rep, (top, flags, counts) = K.top_case(n)
        assert parent.size == n and (n < 4 or counts["dup_entries"] >= 2)
    assert K.top_case(1000)[2][2]["nested_entries"] >= 1 and K.top_case(1000)[2][2]["dropped_classes"] >= 1
    t = K.tree_case(oracle)
    assert t[7]["counts"]["complete_dirs"] == 3 and t[8]["counts"]["complete_dirs"] == 3
    assert (t[7]["digests"][1] == t[7]["digests"][4]).all() and t[7]["digests"][1].any()  # equal directories
    assert t[7]["valid"].tolist() == [1, 1, 1, 1, 1, 1, 1] and t[8]["valid"] is None
    assert t[7]["tree_bytes"].tolist() == [4200, 2100, 100, 2000, 2100, 100, 2000] and not t[8]["tree_bytes"][0]
    link, created, linked, win = K.dedup_case(oracle)[4]
    assert created >= 1 and linked >= 1 and win["steps"] == 1 and len(set(link.tolist())) > 3
    c = K.chunk_case(oracle)
    ch, sh = c["chunks"], c["sharing"]
    assert ch["counts"]["chunks"] > 8 and ch["counts"]["hash_cuts"] >= 2 and ch["file_chunks"][1] == 0
    assert sh["counts"]["distinct_chunks"] < ch["counts"]["chunks"]    # a shared chunk,
    assert sh["self_bytes"][4] > 0 and sh["peer"][5] == 2 and sh["other_bytes"][5] == 32  # within a file and across files
    x = K.index_case(oracle)
    assert x["add5"][3]["added"] == 5 and 5 <= x["match"][2]["hits"] < x["keys"].size  # index hits and misses
    assert x["held"][3]["batch_duplicates"] >= 1 and x["held_match"][2].max() == 2     # a pair with two holders
    assert x["removed"][1]["removed"] == 1 and x["removed"][1]["entries_new"] >= 1     # a removed holder
    assert R.dir_bits(x["keys"].size) >= 1


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def same(what, got, want):
    if isinstance(want, dict):
        assert got == want, f"{what}: {got} != {want}"
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape}"
    bad = np.flatnonzero((got != want).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:5]}"


def same_index(what, got, entries, bits):
    for name, g, w in zip(("keys", "digests", "values", "dir", "bits"), got, R.arrays(entries, bits)):
        same(f"{what} {name}", g, w)


# ---- 1: unlike calls, large and small, in turn on one Engine --------------------------

def small_calls(eng, oracle, what):
    """every host-array entry point once at a small size, against the references"""
    keys, dig, valid, want = K.confirm_case(3)
    for name, g, w in zip(("rep", "key_rep", "flags", "counts"), eng.confirm_duplicates(keys, dig, valid), want):
        same(f"{what} confirm_duplicates {name}", g, w)
    rep, sizes, want = K.sets_case(2)
    for name, g, w in zip(("set_rep", "set_offsets", "set_bytes", "members", "counts"),
                          eng.duplicate_sets(rep, sizes), want):
        same(f"{what} duplicate_sets {name}", g, w)

    c = K.chunk_case(oracle)
    ch = c["chunks"]
    want = (ch["file_chunks"], ch["chunk_off"], ch["chunk_len"], ch["chunk_file"], c["keys"], c["digests"], ch["counts"])
    names = ("file_chunks", "chunk_off", "chunk_len", "chunk_file", "keys", "digests", "counts")
    got = eng.chunk_messages(c["blob"], c["offsets"], c["lens"])
    for name, g, w in zip(names, got, want):
        same(f"{what} chunk_messages {name}", g, w)
    win = eng.chunk_windows(c["blob"], c["offsets"], c["lens"], np.ones(len(K.FILE_SIZES), np.uint8))
    for name, g, w in zip(names + ("consumed",), win, want + (c["lens"],)):
        same(f"{what} chunk_windows {name}", g, w)
    sh = c["sharing"]
    for name, g in zip(("new_bytes", "self_bytes", "other_bytes", "peer", "peer_bytes", "counts"),
                       eng.chunk_sharing(got[3], got[2], c["rep"], len(K.FILE_SIZES))):
        same(f"{what} chunk_sharing {name}", g, sh[name])

    x = K.index_case(oracle)
    k, d, v = x["keys"], x["digests"], x["values"]
    idx, pos, flags, counts = eng.chunk_index_add(x["empty"], k[:5], d[:5], v[:5])
    same_index(f"{what} chunk_index_add", idx, x["add5"][0], x["bits5"])
    for name, g, w in zip(("pos", "flags", "counts"), (pos, flags, counts), x["add5"][1:]):
        same(f"{what} chunk_index_add {name}", g, w)
    for name, g, w in zip(("pos", "value", "counts"), eng.chunk_index_match(idx, k, d), x["match"]):
        same(f"{what} chunk_index_match {name}", g, w)
    held, pos, flags, counts = eng.chunk_holders_add(x["empty"], k, d, v)
    same_index(f"{what} chunk_holders_add", held, x["held"][0], x["bits_held"])
    for name, g, w in zip(("pos", "flags", "counts"), (pos, flags, counts), x["held"][1:]):
        same(f"{what} chunk_holders_add {name}", g, w)
    for name, g, w in zip(("pos", "value", "holders", "counts"), eng.chunk_holders_match(held, k, d), x["held_match"]):
        same(f"{what} chunk_holders_match {name}", g, w)
    left, counts = eng.chunk_holders_remove(held, K.REMOVED)
    same_index(f"{what} chunk_holders_remove", left, x["removed"][0], x["bits_held"])
    same(f"{what} chunk_holders_remove counts", counts, x["removed"][1])

    parent, is_dir, name32, digests, _, _, _, _, want = K.tree_case(oracle)
    got = eng.tree_digests(parent, is_dir, name32, digests)  # valid, sizes and keys absent
    assert got[2] is None
    for name, g in zip(("keys", "digests", "valid", "tree_bytes", "tree_files", "flags", "counts"), got):
        if name != "valid":
            same(f"{what} tree_digests {name}", g, want[name])
    keys, has, status, existing, want = K.dedup_case(oracle)
    for name, g, w in zip(("link", "created", "linked", "window"),
                          eng.identifier_dedup_window(keys, has, status, 100, existing), want):
        assert (g == w).all() if name == "link" else g == w, f"{what} identifier_dedup_window {name}: {g} != {w}"


def large_top(eng, what):
    parent, rep, want = K.top_case(1000)
    for name, g, w in zip(("top_rep", "flags", "counts"), eng.tree_top(parent, rep), want):
        same(f"{what} tree_top {name}", g, w)


def large_confirm(eng, what):
    keys, dig, valid, want = K.big_confirm_case()
    for name, g, w in zip(("rep", "key_rep", "flags", "counts"), eng.confirm_duplicates(keys, dig, valid), want):
        same(f"{what} confirm_duplicates {name}", g, w)


@pytest.mark.gpu
def test_unlike_calls_in_turn_on_one_engine(oracle):
    from spacedrive_amd import Engine
    eng = Engine()  # its own: the buffer starts empty and grows here
    try:
        large_top(eng, "first")
        small_calls(eng, oracle, "after tree_top(1000)")
        large_confirm(eng, "then")                       # larger than everything before: the buffer grows
        small_calls(eng, oracle, "after confirm_duplicates(5000)")
        large_top(eng, "last")
    finally:
        eng.close()


# ---- 3: sizes at the edges of the layout, back to back -------------------------------------

@pytest.mark.gpu
def test_sizes_at_the_edges_of_the_layout(eng):
    for n in K.EDGES + K.EDGES[::-1]:
        keys, dig, valid, want = K.confirm_case(n)
        for name, g, w in zip(("rep", "key_rep", "flags", "counts"), eng.confirm_duplicates(keys, dig, valid), want):
            same(f"n={n} confirm_duplicates {name}", g, w)
        rep, sizes, want = K.sets_case(n)
        for name, g, w in zip(("set_rep", "set_offsets", "set_bytes", "members", "counts"),
                              eng.duplicate_sets(rep, sizes), want):
            same(f"n={n} duplicate_sets {name}", g, w)
        parent, rep, want = K.top_case(n)
        for name, g, w in zip(("top_rep", "flags", "counts"), eng.tree_top(parent, rep), want):
            same(f"n={n} tree_top {name}", g, w)


# ---- 2: optional arrays off ------------------------------------------------------------
#
# Straight through the library. Already asserted elsewhere and not repeated:
# each output of sdcas_confirm_duplicates, sdcas_duplicate_sets and
# sdcas_tree_digests null ALONE (test_gpu_confirm.py and test_gpu_dupsets.py
# test_null_outputs_one_at_a_time, test_gpu_dirtree.py
# test_each_output_null_in_turn_through_the_host_call), and sdcas_duplicate_sets
# with sizes and every output but the counts null (test_gpu_dupsets.py
# test_null_sizes). Here: every optional output null but the counts, only the
# counts null, and each optional input null, behind a larger unlike call.

class Call:
    """one library call over host arrays. args: the arguments between the
    context and the counts, in order: an array, None, a plain value, or the
    NAME of an output; outs: {name: (shape, dtype)} of the outputs that are
    passed, each filled with FILL before the call (a name that is not in outs
    goes as NULL) -> ({name: array}, the counts as a dict or None)"""

    def __init__(self, eng, fn, counts_type):
        self.eng, self.fn, self.counts_type = eng, fn, counts_type

    def __call__(self, args, outs, counts=True):
        bufs = {name: np.full(shape, FILL, dtype) for name, (shape, dtype) in outs.items()}
        cts = self.counts_type() if counts else None
        p = lambda a: None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else a
        argv = [p(bufs.get(a, None)) if isinstance(a, str) else p(a) for a in args]
        rc = self.fn(self.eng.ctx, *argv, ctypes.byref(cts) if counts else None)
        assert rc == N.SDCAS_OK, self.eng.L.sdcas_last_error(self.eng.ctx)
        return bufs, cts.as_dict() if counts else None


def variants(optional):
    """[(the variant's name, the optional outputs passed, counts passed)]"""
    return [("only the counts", (), True), ("all but the counts", optional, False)]


@pytest.fixture(scope="module")
def filled(eng):
    """the Engine after a larger unlike call: the buffer holds its bytes"""
    large_confirm(eng, "fill")
    return eng


@pytest.mark.gpu
def test_confirm_sets_and_top_with_arrays_off(filled):
    eng, L = filled, filled.L
    n = 17
    keys, dig, valid, (rep, key_rep, flags, counts) = K.confirm_case(n)
    call = Call(eng, L.sdcas_confirm_duplicates, N.ConfirmCounts)
    shapes = {"rep": (n, np.int64), "key_rep": (n, np.int64), "flags": (n, np.uint8)}
    for what, on, with_counts in variants(tuple(shapes)):
        got, cts = call([keys, dig, valid, n, "rep", "key_rep", "flags"], {k: shapes[k] for k in on}, with_counts)
        for name, w in zip(shapes, (rep, key_rep, flags)):
            if name in on:
                same(f"confirm_duplicates, {what}: {name}", got[name], w)
        if with_counts:
            same(f"confirm_duplicates, {what}: counts", cts, counts)
    want = K.group_by(keys, dig)  # valid null: every file takes part
    got, cts = call([keys, dig, None, n, "rep", "key_rep", "flags"], shapes)
    for name, w in zip(shapes, want):
        same(f"confirm_duplicates, valid null: {name}", got[name], w)
    same("confirm_duplicates, valid null: counts", cts, want[3])

    rep, sizes, (set_rep, offs, set_bytes, members, counts) = K.sets_case(n)
    call = Call(eng, L.sdcas_duplicate_sets, N.SetsCounts)
    h = n // 2
    shapes = {"set_rep": (h, np.int64), "set_offsets": (h + 1, np.uint64), "set_bytes": (h, np.uint64),
              "members": (n, np.int64)}
    s, m = counts["sets"], counts["members"]
    for what, on, with_counts in variants(tuple(shapes)):
        got, cts = call([rep, sizes, n, N.SDCAS_SETS_BY_REP, *shapes], {k: shapes[k] for k in on}, with_counts)
        for name, w, k in zip(shapes, (set_rep, offs, set_bytes, members), (s, s + 1, s, m)):
            if name in on:
                same(f"duplicate_sets, {what}: {name}", got[name][:k], w)
                assert (got[name][k:] == FILL).all(), f"duplicate_sets, {what}: {name} written past the sets"
        if with_counts:
            same(f"duplicate_sets, {what}: counts", cts, counts)
    got, cts = call([rep, None, n, N.SDCAS_SETS_BY_REP, *shapes], shapes)  # sizes null: set_bytes 0
    for name, w, k in zip(shapes, (set_rep, offs, np.zeros(s, np.uint64), members), (s, s + 1, s, m)):
        same(f"duplicate_sets, sizes null: {name}", got[name][:k], w)
    same("duplicate_sets, sizes null: counts", cts, dict(counts, reclaimable_bytes=0))

    parent, rep, (top, flags, counts) = K.top_case(n)
    call = Call(eng, L.sdcas_tree_top, N.TopCounts)
    shapes = {"top_rep": (n, np.int64), "flags": (n, np.uint8)}
    for what, on, with_counts in variants(tuple(shapes)):
        got, cts = call([parent, rep, n, "top_rep", "flags"], {k: shapes[k] for k in on}, with_counts)
        for name, w in zip(shapes, (top, flags)):
            if name in on:
                same(f"tree_top, {what}: {name}", got[name], w)
        if with_counts:
            same(f"tree_top, {what}: counts", cts, counts)


@pytest.mark.gpu
def test_tree_digests_and_dedup_with_arrays_off(filled, oracle):
    eng, L = filled, filled.L
    parent, is_dir, name32, digests, valid, sizes, keys, full, bare = K.tree_case(oracle)
    n = parent.size
    call = Call(eng, L.sdcas_tree_digests, N.TreeCounts)
    shapes = {"tree_bytes": (n, np.uint64), "tree_files": (n, np.uint64), "flags": (n, np.uint8)}

    def run(what, want, sz, ks, va, on, with_counts):
        io = {"digests": digests.copy(), "keys": None if ks is None else ks.copy(),
              "valid": None if va is None else va.copy()}
        got, cts = call([parent, is_dir, name32, sz, n, io["keys"], io["digests"], io["valid"], *shapes],
                        {k: shapes[k] for k in on}, with_counts)
        same(f"tree_digests, {what}: digests", io["digests"], want["digests"])
        for name in ("keys", "valid"):
            if io[name] is not None:
                same(f"tree_digests, {what}: {name}", io[name], want[name])
        for name in on:
            same(f"tree_digests, {what}: {name}", got[name], want[name])
        if with_counts:
            same(f"tree_digests, {what}: counts", cts, want["counts"])

    for what, on, with_counts in variants(tuple(shapes)):
        run(what, full, sizes, keys, valid, on, with_counts)
    # each optional input null in turn (all three: small_calls)
    nosize = dict(full, tree_bytes=np.zeros(n, np.uint64))
    run("sizes null", nosize, None, keys, valid, tuple(shapes), True)
    run("keys null", full, sizes, None, valid, tuple(shapes), True)
    novalid = dict(full, valid=None)
    run("valid null", novalid, sizes, keys, None, tuple(shapes), True)

    keys, has, status, existing, (link, created, linked, window) = K.dedup_case(oracle)
    n = keys.size

    def dedup(st, with_counts, with_window):
        out = np.full(n, FILL, np.int64)
        c, l = ctypes.c_int64(-7), ctypes.c_int64(-7)
        win = N.JobWindow(0, 0, 0, 0, 0, 0)
        rc = L.sdcas_dedup_window(eng.ctx, keys.ctypes.data, has.ctypes.data, None if st is None else st.ctypes.data, n,
                                  100, existing.ctypes.data, existing.size, ctypes.byref(win) if with_window else None,
                                  out.ctypes.data, ctypes.byref(c) if with_counts else None,
                                  ctypes.byref(l) if with_counts else None)
        assert rc == N.SDCAS_OK, L.sdcas_last_error(eng.ctx)
        return out, (c.value, l.value), {"steps": win.steps, "rows": win.rows, "rereads": win.rereads}

    out, _, _ = dedup(status, False, False)
    same("dedup_window, only the links", out, link)
    out, cl, win = dedup(status, True, True)
    same("dedup_window, all on", out, link)
    assert cl == (created, linked) and win == window
    want = oracle.identifier_job(keys, has, None, 100, existing)
    out, cl, win = dedup(None, True, True)
    same("dedup_window, status null", out, want[0])
    assert cl == want[1:3] and win == want[3]


@pytest.mark.gpu
def test_chunk_calls_with_arrays_off(filled, oracle):
    eng, L = filled, filled.L
    c = K.chunk_case(oracle)
    ch, blob, offs, lens = c["chunks"], c["blob"], c["offsets"], c["lens"]
    n, m = lens.size, ch["counts"]["chunks"]
    mc = eng.chunk_plan(lens)[0]
    cp = eng._chunk_params(None)
    shapes = {"file_chunks": (n + 1, np.uint64), "chunk_off": (mc, np.uint64), "chunk_len": (mc, np.uint64),
              "chunk_file": (mc, np.uint32), "keys": (mc, np.uint64), "digests": ((mc, 32), np.uint8),
              "consumed": (n, np.uint64)}
    want = dict(ch, keys=c["keys"], digests=c["digests"], consumed=lens)
    final = np.ones(n, np.uint8)

    def check(who, what, got, cts, on, with_counts):
        for name in on:
            k = m if name not in ("file_chunks", "consumed") else shapes[name][0]
            same(f"{who}, {what}: {name}", got[name][:k], want[name])
            assert (got[name][k:] == FILL).all(), f"{who}, {what}: {name} written past the chunks"
        if with_counts:
            same(f"{who}, {what}: counts", cts, ch["counts"])

    names = tuple(shapes)[:6]
    call = Call(eng, L.sdcas_chunk_messages, N.ChunkCounts)
    for what, on, with_counts in variants(names) + [("chunk_off without chunk_file", ("chunk_off",), True)]:
        got, cts = call([blob, offs, lens, n, ctypes.byref(cp), *names], {k: shapes[k] for k in on}, with_counts)
        check("chunk_messages", what, got, cts, on, with_counts)
    call = Call(eng, L.sdcas_chunk_windows, N.ChunkCounts)
    for fin in (final, None):  # final null: every window is final
        for what, on, with_counts in variants(tuple(shapes)):
            got, cts = call([blob, offs, lens, fin, n, ctypes.byref(cp), *shapes], {k: shapes[k] for k in on},
                            with_counts)
            check("chunk_windows", what + ("" if fin is not None else ", final null"), got, cts, on, with_counts)

    sh = c["sharing"]
    fl, ln, rep = ch["chunk_file"], ch["chunk_len"], c["rep"]
    shapes = {k: (n, np.int64 if k == "peer" else np.uint64)
              for k in ("new_bytes", "self_bytes", "other_bytes", "peer", "peer_bytes")}
    call = Call(eng, L.sdcas_chunk_sharing, N.SharingCounts)
    for what, on, with_counts in variants(tuple(shapes)):
        got, cts = call([fl, ln, rep, m, n, *shapes], {k: shapes[k] for k in on}, with_counts)
        for name in on:
            same(f"chunk_sharing, {what}: {name}", got[name], sh[name])
        if with_counts:
            same(f"chunk_sharing, {what}: counts", cts, sh["counts"])


@pytest.mark.gpu
def test_index_calls_with_arrays_off(filled, oracle):
    eng, L = filled, filled.L
    x = K.index_case(oracle)
    k, d, v = x["keys"], x["digests"], x["values"]
    m = k.size
    valid = np.ones(m, np.uint8)
    valid[1] = 0
    for kind, fn_match, fn_add, ref, entries, bits in (
            ("index", L.sdcas_chunk_index_match, L.sdcas_chunk_index_add, R, x["add5"][0], x["bits5"]),
            ("holders", L.sdcas_chunk_holders_match, L.sdcas_chunk_holders_add, K.H, x["held"][0], x["bits_held"])):
        ik, idg, iv, idir, _ = R.arrays(entries, bits)
        shapes = {"pos": (m, np.int64), "value": (m, np.uint64)}
        if kind == "holders":
            shapes["holders"] = (m, np.uint32)
        call = Call(eng, fn_match, N.IndexMatchCounts)
        cases = [(what, on, wc, None) for what, on, wc in variants(tuple(shapes))]
        cases += [("with valid", tuple(shapes), True, valid)]
        for what, on, with_counts, va in cases:
            want = dict(zip(tuple(shapes) + ("counts",), ref.match(entries, k, d, va)))
            got, cts = call([ik, idg, iv, idir, ik.size, bits, k, d, va, m, *shapes], {s: shapes[s] for s in on},
                            with_counts)
            for name in on:
                same(f"{kind} match, {what}: {name}", got[name], want[name])
            if with_counts:
                same(f"{kind} match, {what}: counts", cts, want["counts"])

        # the add: the new index is required; pos, flags and the counts are optional
        cap = ik.size + m
        bits_new = R.dir_bits(cap)
        new = {"new_keys": (cap, np.uint64), "new_digests": ((cap, 32), np.uint8), "new_values": (cap, np.uint64),
               "new_dir": ((1 << bits_new) + 1, np.uint32)}
        opt = {"pos": (m, np.int64), "flags": (m, np.uint8)}
        call = Call(eng, fn_add, N.IndexAddCounts)
        cases = [(what, on, wc, v, None) for what, on, wc in variants(tuple(opt))]
        cases += [("values null", tuple(opt), True, None, None), ("with valid", tuple(opt), True, v, valid)]
        for what, on, with_counts, values, va in cases:
            wnew, wpos, wflags, wcounts = ref.add(entries, k, d, values, va)
            got, cts = call([ik, idg, iv, idir, ik.size, bits, k, d, values, va, m, *new, bits_new, *opt],
                            {**new, **{s: opt[s] for s in on}}, with_counts)
            e = len(wnew)
            same_index(f"{kind} add, {what}", (got["new_keys"][:e], got["new_digests"][:e], got["new_values"][:e],
                                              got["new_dir"], bits_new), wnew, bits_new)
            for name in ("new_keys", "new_digests", "new_values"):
                assert (got[name][e:] == FILL).all(), f"{kind} add, {what}: {name} written past entries_new"
            for name, w in (("pos", wpos), ("flags", wflags)):
                if name in on:
                    same(f"{kind} add, {what}: {name}", got[name], w)
            if with_counts:
                same(f"{kind} add, {what}: counts", cts, wcounts)

    # the remove: only the counts are optional
    entries, bits = x["held"][0], x["bits_held"]
    ik, idg, iv, idir, _ = R.arrays(entries, bits)
    n = ik.size
    new = {"new_keys": (n, np.uint64), "new_digests": ((n, 32), np.uint8), "new_values": (n, np.uint64),
           "new_dir": ((1 << bits) + 1, np.uint32)}
    call = Call(eng, L.sdcas_chunk_holders_remove, N.HoldersRemoveCounts)
    wnew, wcounts = x["removed"]
    for with_counts in (True, False):
        got, cts = call([ik, idg, iv, idir, n, bits, K.REMOVED, K.REMOVED.size, *new, bits], new, with_counts)
        e = len(wnew)
        same_index(f"holders remove, counts {with_counts}", (got["new_keys"][:e], got["new_digests"][:e],
                                                             got["new_values"][:e], got["new_dir"], bits), wnew, bits)
        if with_counts:
            same("holders remove: counts", cts, wcounts)
