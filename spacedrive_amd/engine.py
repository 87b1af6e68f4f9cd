"""Host-side mirror of sd-core's content-identification interface over the
libsdcas.so C ABI.

The reference functions keep their names, argument meaning and error
behaviour:

* ``generate_cas_id(path, size) -> str`` — core/src/object/cas.rs:23-62
  (16 lowercase hex chars; io errors raise ``OSError``; a file shorter than
  the windows ``size`` implies raises ``OSError(UnexpectedEof, "failed to
  fill whole buffer")`` like tokio's read_exact);
* ``file_checksum(path) -> str`` — core/src/object/validation/hash.rs:11-25
  (64 lowercase hex chars);
* ``identifier_dedup(...)`` — the cas_id -> Object link of
  core/src/object/file_identifier/mod.rs:98-350 in canonical form.

The batch forms (``generate_cas_ids``, ``file_checksums``,
``hash_messages``) are what the identifier/validator jobs would call once per
chunk instead of per file. Everything runs on the GPU; there is no CPU path.
"""
import ctypes
import itertools
import os
import sys

import numpy as np

from . import _native as N



_STREAM_TOKENS = itertools.count(1)  # sdcas_dev_bind_stream tokens: unique per process

def _cpaths(paths):
    """(buffer, pointers) for a `const char* const*` argument: the paths
    NUL-terminated in ONE bytes buffer and a uint64 array of their addresses
    (one numpy pass instead of a ctypes object per path — the per-path form
    cost more than the library's reads of 200 K files). Keep `buffer` alive
    for the call."""
    n = len(paths)
    if n == 0:
        return None, np.zeros(1, np.uint64)
    try:  # the common case, a list of str: one join, one encode
        enc = ("\0".join(paths) + "\0").encode(sys.getfilesystemencoding(), "surrogateescape")
    except TypeError:  # bytes or os.PathLike items
        enc = b"\0".join(os.fsencode(p) for p in paths) + b"\0"
    buf = np.frombuffer(enc, np.uint8)
    ends = np.flatnonzero(buf == 0)
    if len(ends) != n:
        raise ValueError("a path contains a NUL byte")
    ptrs = np.empty(n, np.uint64)
    ptrs[0] = 0
    ptrs[1:] = ends[:-1] + 1
    ptrs += np.uint64(buf.ctypes.data)
    return buf, ptrs


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def key_to_hex(key: int) -> str:
    return f"{int(key):016x}"


def digest_to_hex(d) -> str:
    return bytes(np.asarray(d, dtype=np.uint8)).hex()


def io_error(status: int, path=None) -> OSError:
    if status == N.SDCAS_STATUS_UNEXPECTED_EOF:
        e = OSError(status, "failed to fill whole buffer")
    else:
        e = OSError(status, os.strerror(status) if status < 4096 else f"status {status}")
    if path is not None:
        e.filename = str(path)
    return e


class Engine:
    """One libsdcas context bound to one GPU.

    progress: optional callable(done_bytes, total_bytes), called on the
    calling thread after every staging slot of a path call (the job's
    progress report, job/worker.rs:458-480). cancel: optional
    ``ctypes.c_int32`` the caller may set nonzero from any thread to stop a
    path call (job/mod.rs:862-960); the call then raises ``Cancelled`` whose
    ``partial`` holds the completed items. direct_io: the path calls
    (generate_cas_ids, file_checksums) read with O_DIRECT (cold storage).
    """

    def __init__(self, device: int = 0, io_threads: int = 0, staging_bytes: int = 0, progress=None, cancel=None,
                 direct_io=False):
        self.L = N.load()
        self.device_ordinal = int(device)
        self._cb = self._progress_fn(progress)
        self._cancel = cancel
        opts = N.Options(device, io_threads, N.SDCAS_OPT_DIRECT_IO if direct_io else 0, staging_bytes, self._cb,
                         None, ctypes.pointer(cancel) if cancel is not None else None)
        ctx = ctypes.c_void_p()
        rc = self.L.sdcas_init(ctypes.byref(opts), ctypes.byref(ctx))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, "sdcas_init failed (no HIP device?)")
        self.ctx = ctx

    @staticmethod
    def _progress_fn(progress):
        if progress is None:
            return N.PROGRESS_FN()
        return N.PROGRESS_FN(lambda _user, done, total: progress(int(done), int(total)))

    def set_progress(self, progress=None, cancel=None):
        """re-bind the progress callable and cancel flag (sdcas_set_progress)"""
        cb = self._progress_fn(progress)
        self._check(self.L.sdcas_set_progress(self.ctx, cb, None,
                                              ctypes.pointer(cancel) if cancel is not None else None),
                    "sdcas_set_progress")
        self._cb, self._cancel = cb, cancel

    # -- lifetime -------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            self.L.sdcas_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what, partial=None):
        if rc != N.SDCAS_OK:
            msg = self.L.sdcas_last_error(self.ctx).decode(errors="replace")
            if rc == N.SDCAS_E_CANCELLED:
                raise N.Cancelled(f"{what}: {msg}", partial)
            raise N.SdcasError(rc, f"{what}: {msg}")

    # -- reference functions, batched ------------------------------------------
    def generate_cas_ids(self, paths, sizes):
        """cas.rs:23-62 for many files -> (keys uint64[n], status int32[n])"""
        n = len(paths)
        buf, parr = _cpaths(paths)
        sizes = _arr(sizes, np.uint64)
        keys = np.zeros(n, np.uint64)
        st = np.zeros(n, np.int32)
        self._check(self.L.sdcas_cas_ids(self.ctx, _ptr(parr), _ptr(sizes), n, _ptr(keys), _ptr(st)),
                    "sdcas_cas_ids", (keys, st))
        del buf
        return keys, st

    def file_metadata(self, paths, size_hints=None):
        """FileMetadata::new's fs::metadata + generate_cas_id (mod.rs:48-96) for
        many files, the length from fstat of the read descriptor
        (sdcas_file_metadata; size_hints: the indexer's sizes, which only plan
        the staging) -> (sizes uint64[n], keys uint64[n], status int32[n],
        flags uint8[n]: SDCAS_META_HAS_CAS_ID | SDCAS_META_DIR)"""
        n = len(paths)
        buf, parr = _cpaths(paths)
        hints = _arr(size_hints, np.uint64) if size_hints is not None else None
        sizes = np.zeros(n, np.uint64)
        keys = np.zeros(n, np.uint64)
        st = np.zeros(n, np.int32)
        fl = np.zeros(n, np.uint8)
        self._check(self.L.sdcas_file_metadata(self.ctx, _ptr(parr), _ptr(hints) if hints is not None else None, n,
                                               _ptr(sizes), _ptr(keys), _ptr(st), _ptr(fl)),
                    "sdcas_file_metadata", (sizes, keys, st, fl))
        del buf
        return sizes, keys, st, fl

    def identify_checksums(self, paths, size_hints=None):
        """file_metadata followed by file_checksums from ONE open and ONE read
        of each file (sdcas_identify_checksums) -> (sizes uint64[n], keys
        uint64[n], digests uint8[n, 32], status int32[n], flags uint8[n]:
        SDCAS_META_HAS_CAS_ID | SDCAS_META_DIR | SDCAS_META_HAS_CHECKSUM)"""
        n = len(paths)
        buf, parr = _cpaths(paths)
        hints = _arr(size_hints, np.uint64) if size_hints is not None else None
        sizes = np.zeros(n, np.uint64)
        keys = np.zeros(n, np.uint64)
        out = np.zeros((n, 32), np.uint8)
        st = np.zeros(n, np.int32)
        fl = np.zeros(n, np.uint8)
        self._check(self.L.sdcas_identify_checksums(self.ctx, _ptr(parr),
                                                    _ptr(hints) if hints is not None else None, n, _ptr(sizes),
                                                    _ptr(keys), _ptr(out), _ptr(st), _ptr(fl)),
                    "sdcas_identify_checksums", (sizes, keys, out, st, fl))
        del buf
        return sizes, keys, out, st, fl

    def file_checksums(self, paths):
        """hash.rs:11-25 for many files -> (digests uint8[n, 32], status int32[n])"""
        n = len(paths)
        buf, parr = _cpaths(paths)
        out = np.zeros((n, 32), np.uint8)
        st = np.zeros(n, np.int32)
        self._check(self.L.sdcas_checksums(self.ctx, _ptr(parr), n, _ptr(out), _ptr(st)), "sdcas_checksums",
                    (out, st))
        del buf
        return out, st

    def generate_cas_id(self, path, size) -> str:
        keys, st = self.generate_cas_ids([path], [size])
        if st[0]:
            raise io_error(int(st[0]), path)
        return key_to_hex(keys[0])

    def file_checksum(self, path) -> str:
        out, st = self.file_checksums([path])
        if st[0]:
            raise io_error(int(st[0]), path)
        return digest_to_hex(out[0])

    # -- pre-assembled messages ---------------------------------------------------
    @staticmethod
    def pack(messages):
        """list of bytes-like -> (blob, offsets, lens)"""
        lens = np.array([len(m) for m in messages], np.uint64)
        offs = np.zeros(len(messages), np.uint64)
        if len(messages):
            offs[1:] = np.cumsum(lens[:-1])
        blob = np.frombuffer(b"".join(bytes(m) for m in messages), np.uint8) if len(messages) else \
            np.zeros(0, np.uint8)
        return blob, offs, lens

    def hash_messages(self, blob, offsets, lens):
        blob = _arr(blob, np.uint8)
        offsets, lens = _arr(offsets, np.uint64), _arr(lens, np.uint64)
        n = lens.size
        out = np.zeros((n, 32), np.uint8)
        self._check(self.L.sdcas_hash_messages(self.ctx, _ptr(blob) or 1, _ptr(offsets), _ptr(lens), n,
                                               _ptr(out)), "sdcas_hash_messages")
        return out

    def cas_ids_from_messages(self, blob, offsets, lens):
        blob = _arr(blob, np.uint8)
        offsets, lens = _arr(offsets, np.uint64), _arr(lens, np.uint64)
        n = lens.size
        keys = np.zeros(n, np.uint64)
        self._check(self.L.sdcas_cas_ids_from_messages(self.ctx, _ptr(blob) or 1, _ptr(offsets),
                                                       _ptr(lens), n, _ptr(keys)),
                    "sdcas_cas_ids_from_messages")
        return keys

    # -- dedup ------------------------------------------------------------------------
    def identifier_dedup(self, keys, has_key, status=None, chunk_size=100, existing_keys=()):
        """the file identifier job's group-by over these orphans (sdcas_dedup)
        -> (link int64[n], created, linked)"""
        link, created, linked, _ = self.identifier_dedup_window(keys, has_key, status, chunk_size, existing_keys)
        return link, created, linked

    def identifier_dedup_window(self, keys, has_key, status=None, chunk_size=100, existing_keys=(), max_steps=0,
                                more=False):
        """sdcas_dedup_window: the job's steps over one batch of its orphans
        -> (link, created, linked, {"steps", "rows", "rereads"})"""
        keys = _arr(keys, np.uint64)
        n = keys.size
        has_key = _arr(has_key, np.uint8)
        st = None if status is None else _arr(status, np.int32)
        ex = _arr(existing_keys, np.uint64)
        out = np.zeros(n, np.int64)
        created, linked = ctypes.c_int64(0), ctypes.c_int64(0)
        win = N.JobWindow(int(max_steps), int(bool(more)), 0, 0, 0, 0)
        self._check(self.L.sdcas_dedup_window(self.ctx, _ptr(keys), _ptr(has_key), _ptr(st), n, chunk_size,
                                              _ptr(ex), ex.size, ctypes.byref(win), _ptr(out), ctypes.byref(created),
                                              ctypes.byref(linked)), "sdcas_dedup_window")
        return out, created.value, linked.value, {"steps": win.steps, "rows": win.rows, "rereads": win.rereads}

    # -- duplicates confirmed by checksum -----------------------------------------------
    def confirm_duplicates(self, keys, digests, valid=None):
        """the group-by over (cas key, 32-byte checksum) (sdcas_confirm_duplicates):
        files with one key and one digest are a class, a key with two classes
        collides -> (rep int64[n]: the class's lowest valid file, key_rep
        int64[n]: the key's, both -1 for a file with valid == 0, flags uint8[n]:
        SDCAS_CONFIRM_DUPLICATE | SDCAS_CONFIRM_COLLISION | SDCAS_CONFIRM_SKIPPED,
        counts: dict of sdcas_confirm_counts' six fields)"""
        keys = _arr(keys, np.uint64)
        n = keys.size
        digests = _arr(digests, np.uint8)
        if digests.size != 32 * n:
            raise ValueError(f"confirm_duplicates: {n} keys, {digests.size} digest bytes")
        va = None if valid is None else _arr(valid, np.uint8)
        if va is not None and va.size != n:
            raise ValueError(f"confirm_duplicates: {n} keys, {va.size} valid flags")
        rep = np.zeros(n, np.int64)
        key_rep = np.zeros(n, np.int64)
        flags = np.zeros(n, np.uint8)
        counts = N.ConfirmCounts()
        self._check(self.L.sdcas_confirm_duplicates(self.ctx, _ptr(keys), _ptr(digests), _ptr(va), n, _ptr(rep),
                                                    _ptr(key_rep), _ptr(flags), ctypes.byref(counts)),
                    "sdcas_confirm_duplicates")
        return rep, key_rep, flags, counts.as_dict()

    def identify_confirmed(self, paths, size_hints=None):
        """scan these files and say which are really duplicates:
        identify_checksums, then confirm_duplicates over the files that have a
        cas_id and a checksum and were read without error -> (identify_checksums'
        tuple, confirm_duplicates' tuple)"""
        ident = self.identify_checksums(paths, size_hints)
        _, keys, digests, st, fl = ident
        both = N.SDCAS_META_HAS_CAS_ID | N.SDCAS_META_HAS_CHECKSUM
        valid = (((fl & both) == both) & (st == 0)).astype(np.uint8)
        return ident, self.confirm_duplicates(keys, digests, valid)

    # -- duplicate sets ---------------------------------------------------------------
    def duplicate_sets(self, rep, sizes=None, order=N.SDCAS_SETS_BY_REP):
        """the files grouped by the value rep[i] (confirm_duplicates' rep;
        values outside [0, n) take no part) into sets of two or more
        (sdcas_duplicate_sets) -> (set_rep int64[S]: each set's lowest member,
        set_offsets uint64[S + 1], set_bytes uint64[S]: sizes[set_rep],
        members int64[M]: set s is members[set_offsets[s]:set_offsets[s + 1]],
        ascending, counts: dict of sdcas_sets_counts' six fields). order:
        SDCAS_SETS_BY_REP, or SDCAS_SETS_BY_RECLAIMABLE (needs sizes): most
        reclaimable bytes first, ties by set_rep"""
        rep = _arr(rep, np.int64)
        n = rep.size
        sz = None if sizes is None else _arr(sizes, np.uint64)
        if sz is not None and sz.size != n:
            raise ValueError(f"duplicate_sets: {n} reps, {sz.size} sizes")
        set_rep = np.zeros(n // 2, np.int64)
        set_offsets = np.zeros(n // 2 + 1, np.uint64)
        set_bytes = np.zeros(n // 2, np.uint64)
        members = np.zeros(n, np.int64)
        counts = N.SetsCounts()
        # (an empty sizes array is still "sizes given": never dereferenced with n == 0)
        self._check(self.L.sdcas_duplicate_sets(self.ctx, _ptr(rep), None if sz is None else _ptr(sz) or 8, n,
                                                int(order), _ptr(set_rep),
                                                _ptr(set_offsets), _ptr(set_bytes), _ptr(members),
                                                ctypes.byref(counts)), "sdcas_duplicate_sets")
        s, m = int(counts.sets), int(counts.members)
        return set_rep[:s].copy(), set_offsets[:s + 1].copy(), set_bytes[:s].copy(), members[:m].copy(), \
            counts.as_dict()

    def identify_duplicate_sets(self, paths, size_hints=None, order=N.SDCAS_SETS_BY_RECLAIMABLE):
        """scan these files and list the sets of equal ones, the biggest win
        first: identify_confirmed, then duplicate_sets over its rep and the
        sizes identify_checksums returned -> (identify_checksums' tuple,
        confirm_duplicates' tuple, duplicate_sets' tuple)"""
        ident, confirm = self.identify_confirmed(paths, size_hints)
        return ident, confirm, self.duplicate_sets(confirm[0], ident[0], order)

    # -- duplicate directories ---------------------------------------------------------
    @staticmethod
    def tree_plan(parent, is_dir):
        """sdcas_tree_plan (no GPU): checks the shape (SdcasError with
        SDCAS_E_INVALID / SDCAS_E_CAPACITY) -> (depth uint32[n], children
        uint64[n], levels)"""
        parent, is_dir = _arr(parent, np.int64), _arr(is_dir, np.uint8)
        n = parent.size
        if is_dir.size != n:
            raise ValueError(f"tree_plan: {n} parents, {is_dir.size} is_dir flags")
        depth = np.zeros(n, np.uint32)
        children = np.zeros(n, np.uint64)
        levels = ctypes.c_uint64(0)
        rc = N.load().sdcas_tree_plan(_ptr(parent), _ptr(is_dir), n, _ptr(depth), _ptr(children),
                                      ctypes.byref(levels))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, "sdcas_tree_plan: the shape is refused")
        return depth, children, int(levels.value)

    def tree_digests(self, parent, is_dir, name32, digests, valid=None, sizes=None, keys=None):
        """a digest per directory (sdcas_tree_digests; the definitions are in
        include/sdcas.h). digests / valid / keys hold the FILE entries' values;
        copies of them come back with the directory entries' slots filled ->
        (keys uint64[n], digests uint8[n, 32], valid uint8[n] or None when none
        was given, tree_bytes uint64[n], tree_files uint64[n], flags uint8[n]:
        SDCAS_TREE_DIR | SDCAS_TREE_INCOMPLETE | SDCAS_TREE_EMPTY, counts: dict
        of sdcas_tree_counts' six fields)"""
        parent, is_dir = _arr(parent, np.int64), _arr(is_dir, np.uint8)
        n = parent.size
        name32 = _arr(name32, np.uint8)
        digests = np.array(digests, dtype=np.uint8, order="C").reshape(n, 32)
        va = None if valid is None else np.array(valid, dtype=np.uint8, order="C")
        sz = None if sizes is None else _arr(sizes, np.uint64)
        ks = np.zeros(n, np.uint64) if keys is None else np.array(keys, dtype=np.uint64, order="C")
        for nm, a, want in (("is_dir", is_dir, n), ("name32", name32, 32 * n), ("valid", va, n), ("sizes", sz, n),
                            ("keys", ks, n)):
            if a is not None and a.size != want:
                raise ValueError(f"tree_digests: {n} entries, {a.size} bytes or entries of {nm}")
        tree_bytes = np.zeros(n, np.uint64)
        tree_files = np.zeros(n, np.uint64)
        flags = np.zeros(n, np.uint8)
        counts = N.TreeCounts()
        self._check(self.L.sdcas_tree_digests(self.ctx, _ptr(parent), _ptr(is_dir), _ptr(name32),
                                              None if sz is None else _ptr(sz), n, _ptr(ks), _ptr(digests),
                                              None if va is None else _ptr(va), _ptr(tree_bytes), _ptr(tree_files),
                                              _ptr(flags), ctypes.byref(counts)), "sdcas_tree_digests")
        return ks, digests, va, tree_bytes, tree_files, flags, counts.as_dict()

    def tree_top(self, parent, rep):
        """the top-most duplicates (sdcas_tree_top): rep is a label per entry,
        e.g. confirm_duplicates' rep over ALL entries -> (top_rep int64[n]:
        rep[i] when i's class is kept, else -1, flags uint8[n]: SDCAS_TOP_DUP |
        SDCAS_TOP_NESTED, counts: dict of sdcas_top_counts' six fields)"""
        parent, rep = _arr(parent, np.int64), _arr(rep, np.int64)
        n = parent.size
        if rep.size != n:
            raise ValueError(f"tree_top: {n} parents, {rep.size} reps")
        top = np.zeros(n, np.int64)
        flags = np.zeros(n, np.uint8)
        counts = N.TopCounts()
        self._check(self.L.sdcas_tree_top(self.ctx, _ptr(parent), _ptr(rep), n, _ptr(top), _ptr(flags),
                                          ctypes.byref(counts)), "sdcas_tree_top")
        return top, flags, counts.as_dict()

    @staticmethod
    def walk_tree(root):
        """the entries below root (root itself is none), a directory's entries
        in name order, symlinks skipped and not followed -> (relative paths,
        is_dir uint8[n], parent int64[n]: -1 directly under root)"""
        rel, kinds, parents = [], [], []
        stack = [(os.fspath(root), "", -1)]
        while stack:
            path, prefix, at = stack.pop()
            with os.scandir(path) as it:
                found = sorted(it, key=lambda e: os.fsencode(e.name))
            for e in found:
                if e.is_symlink():
                    continue
                d = e.is_dir(follow_symlinks=False)
                if not d and not e.is_file(follow_symlinks=False):
                    continue
                rel.append(prefix + e.name)
                kinds.append(1 if d else 0)
                parents.append(at)
                if d:
                    stack.append((e.path, prefix + e.name + os.sep, len(rel) - 1))
        return rel, np.array(kinds, np.uint8), np.array(parents, np.int64)

    def identify_duplicate_trees(self, root, order=N.SDCAS_SETS_BY_RECLAIMABLE):
        """scan a directory and list its top-most duplicates, directories and
        files mixed, the biggest win first: walk_tree, identify_checksums over
        the files, the names hashed by hash_messages, tree_digests, the file
        entries keyed by their digests' first 8 bytes (one key rule for both
        kinds), ONE confirm_duplicates over all entries, tree_top, then
        duplicate_sets over top_rep and tree_bytes -> dict with "entries"
        (relative path, is_dir), the per-entry arrays "parent", "is_dir",
        "sizes", "status", "keys", "digests", "valid", "tree_bytes",
        "tree_files", "tree_flags", "rep", "top_rep", "top_flags", the sets
        "set_rep", "set_offsets", "set_bytes", "members" (duplicate_sets'
        layout) and "tree_counts", "top_counts", "sets_counts"."""
        root = os.fspath(root)
        rel, is_dir, parent = self.walk_tree(root)
        n = len(rel)
        files = np.flatnonzero(is_dir == 0)
        sizes = np.zeros(n, np.uint64)
        status = np.zeros(n, np.int32)
        digests = np.zeros((n, 32), np.uint8)
        valid = np.zeros(n, np.uint8)
        if files.size:
            fs, _, fd, fst, ffl = self.identify_checksums([os.path.join(root, rel[i]) for i in files])
            sizes[files], status[files], digests[files] = fs, fst, fd
            valid[files] = ((ffl & N.SDCAS_META_HAS_CHECKSUM) != 0) & (fst == 0)
        names = [os.fsencode(os.path.basename(r)) for r in rel]
        name32 = self.hash_messages(*self.pack(names)) if n else np.zeros((0, 32), np.uint8)
        keys = np.zeros(n, np.uint64)
        keys[files] = digests[files, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
        keys, digests, valid, tree_bytes, tree_files, tflags, tcounts = self.tree_digests(
            parent, is_dir, name32, digests, valid, sizes, keys)
        rep, _, _, _ = self.confirm_duplicates(keys, digests, valid)
        top_rep, top_flags, top_counts = self.tree_top(parent, rep)
        set_rep, set_offsets, set_bytes, members, scounts = self.duplicate_sets(top_rep, tree_bytes, order)
        return {"entries": list(zip(rel, (bool(d) for d in is_dir))), "parent": parent, "is_dir": is_dir,
                "sizes": sizes, "status": status, "name32": name32, "keys": keys, "digests": digests, "valid": valid,
                "tree_bytes": tree_bytes, "tree_files": tree_files, "tree_flags": tflags, "rep": rep,
                "top_rep": top_rep, "top_flags": top_flags, "set_rep": set_rep, "set_offsets": set_offsets,
                "set_bytes": set_bytes, "members": members, "tree_counts": tcounts, "top_counts": top_counts,
                "sets_counts": scounts}

    # -- content-defined chunks: files that share most of their bytes ---------------
    @staticmethod
    def _chunk_params(params):
        mn, bits, mx = N.SDCAS_CHUNK_PARAMS_DEFAULT if params is None else (int(v) for v in params)
        return N.ChunkParams(mn, bits, mx, 0)

    @staticmethod
    def chunk_plan(lens, params=None):
        """sdcas_chunk_plan (no GPU): SdcasError with SDCAS_E_INVALID for
        invalid parameters (min_len, avg_bits, max_len), SDCAS_E_CAPACITY above
        2^30 chunks -> (max_chunks: the entries of every per-chunk array,
        max_slots: what sizes dev_chunk's workspace)"""
        lens = _arr(lens, np.uint64)
        mc, ms = ctypes.c_uint64(0), ctypes.c_uint64(0)
        cp = Engine._chunk_params(params)
        rc = N.load().sdcas_chunk_plan(_ptr(lens), lens.size, ctypes.byref(cp), ctypes.byref(mc), ctypes.byref(ms))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, "sdcas_chunk_plan: the parameters or the lengths are refused")
        return int(mc.value), int(ms.value)

    def chunk_messages(self, blob, offsets, lens, params=None, hashes=True):
        """the files blob[offsets[i] : offsets[i] + lens[i]] cut into
        content-defined chunks (sdcas_chunk_messages; the definition is in
        include/sdcas.h) -> (file_chunks uint64[n + 1], chunk_off uint64[m]:
        offsets in the blob, chunk_len uint64[m], chunk_file uint32[m], keys
        uint64[m], digests uint8[m, 32], counts: dict of sdcas_chunk_counts'
        six fields). hashes False: no keys and digests (None)"""
        blob = _arr(blob, np.uint8)
        offsets, lens = _arr(offsets, np.uint64), _arr(lens, np.uint64)
        n = lens.size
        if offsets.size != n:
            raise ValueError(f"chunk_messages: {n} lens, {offsets.size} offsets")
        if n and int((offsets + lens).max()) > blob.size:
            raise ValueError("chunk_messages: a file ends past the blob")
        mc, _ = self.chunk_plan(lens, params)
        fc = np.zeros(n + 1, np.uint64)
        off, ln = np.zeros(mc, np.uint64), np.zeros(mc, np.uint64)
        fl = np.zeros(mc, np.uint32)
        keys = np.zeros(mc, np.uint64) if hashes else None
        dig = np.zeros((mc, 32), np.uint8) if hashes else None
        counts = N.ChunkCounts()
        cp = self._chunk_params(params)
        self._check(self.L.sdcas_chunk_messages(self.ctx, _ptr(blob), _ptr(offsets), _ptr(lens), n, ctypes.byref(cp),
                                                _ptr(fc), _ptr(off), _ptr(ln), _ptr(fl),
                                                _ptr(keys) if hashes else None, _ptr(dig) if hashes else None,
                                                ctypes.byref(counts)), "sdcas_chunk_messages")
        m = int(counts.chunks)
        return fc, off[:m].copy(), ln[:m].copy(), fl[:m].copy(), keys[:m].copy() if hashes else None, \
            dig[:m].copy() if hashes else None, counts.as_dict()

    def chunk_sharing(self, chunk_file, chunk_len, rep, n_files):
        """per file, the bytes of its chunks seen first in it, earlier in it
        and in other files, and the other file that holds most of them
        (sdcas_chunk_sharing; rep: confirm_duplicates' rep over the chunks) ->
        (new_bytes, self_bytes, other_bytes uint64[n_files], peer
        int64[n_files]: -1 for none, peer_bytes uint64[n_files], counts: dict
        of sdcas_sharing_counts' six fields)"""
        chunk_file, chunk_len, rep = _arr(chunk_file, np.uint32), _arr(chunk_len, np.uint64), _arr(rep, np.int64)
        m, nf = chunk_file.size, int(n_files)
        if chunk_len.size != m or rep.size != m:
            raise ValueError(f"chunk_sharing: {m} chunk files, {chunk_len.size} lengths, {rep.size} reps")
        new, own, other = (np.zeros(nf, np.uint64) for _ in range(3))
        peer, peer_bytes = np.zeros(nf, np.int64), np.zeros(nf, np.uint64)
        counts = N.SharingCounts()
        self._check(self.L.sdcas_chunk_sharing(self.ctx, _ptr(chunk_file), _ptr(chunk_len), _ptr(rep), m, nf,
                                               _ptr(new), _ptr(own), _ptr(other), _ptr(peer), _ptr(peer_bytes),
                                               ctypes.byref(counts)), "sdcas_chunk_sharing")
        return new, own, other, peer, peer_bytes, counts.as_dict()

    def similar_files(self, paths, params=None, max_bytes=1 << 30):
        """which of these files share most of their bytes: the files are read
        whole (ValueError when they hold more than max_bytes in total: the
        contents must be resident at once), cut into content-defined chunks,
        the chunks grouped by (key, digest) and the sharing pass run over them
        -> dict with the per-file arrays "sizes", "new_bytes", "self_bytes",
        "other_bytes", "peer", "peer_bytes", the chunk arrays "file_chunks",
        "chunk_off" (offsets in the file), "chunk_len", "chunk_file", "keys",
        "digests", "rep", and "chunk_counts", "sharing_counts"."""
        paths = [os.fspath(p) for p in paths]
        total = sum(os.path.getsize(p) for p in paths)
        if total > int(max_bytes):
            raise ValueError(f"similar_files: {total} bytes in {len(paths)} files exceed max_bytes = {int(max_bytes)}")
        data = []
        for p in paths:
            with open(p, "rb") as f:
                data.append(f.read())
        if sum(len(d) for d in data) > int(max_bytes):
            raise ValueError(f"similar_files: the files grew past max_bytes = {int(max_bytes)}")
        blob, offs, lens = self.pack(data)
        fc, off, ln, fl, keys, dig, ccounts = self.chunk_messages(blob, offs, lens, params)
        rep = self.confirm_duplicates(keys, dig)[0]
        new, own, other, peer, peer_bytes, scounts = self.chunk_sharing(fl, ln, rep, len(paths))
        return {"sizes": lens, "new_bytes": new, "self_bytes": own, "other_bytes": other, "peer": peer,
                "peer_bytes": peer_bytes, "file_chunks": fc, "chunk_off": off - offs[fl], "chunk_len": ln,
                "chunk_file": fl, "keys": keys, "digests": dig, "rep": rep, "chunk_counts": ccounts,
                "sharing_counts": scounts}

    # -- chunk windows: files larger than device memory, piece by piece --------------
    @staticmethod
    def chunk_seg_bytes(params=None):
        """sdcas_chunk_seg_bytes (no GPU): the segment length the cut pass of
        chunk_windows uses for these parameters (SDCAS_CHUNK_SEG_BYTES, default
        1 MiB, not below 2 * max_len, a multiple of 64); 0 for invalid ones"""
        cp = Engine._chunk_params(params)
        return int(N.load().sdcas_chunk_seg_bytes(ctypes.byref(cp)))

    def chunk_windows(self, blob, offsets, lens, final=None, params=None, hashes=True):
        """chunk_messages over windows (sdcas_chunk_windows; the definition is
        in include/sdcas.h): window i is blob[offsets[i] : offsets[i] +
        lens[i]], bytes of a file from one of its cuts on; final[i] says that
        it ends where the file ends (None: all do). -> chunk_messages' seven
        results and consumed uint64[n]: where the next window of that file
        begins, relative to this one"""
        blob = _arr(blob, np.uint8)
        offsets, lens = _arr(offsets, np.uint64), _arr(lens, np.uint64)
        n = lens.size
        if offsets.size != n:
            raise ValueError(f"chunk_windows: {n} lens, {offsets.size} offsets")
        if final is not None:
            final = _arr(np.asarray(final).astype(np.uint8), np.uint8)
            if final.size != n:
                raise ValueError(f"chunk_windows: {n} lens, {final.size} final flags")
        if n and int((offsets + lens).max()) > blob.size:
            raise ValueError("chunk_windows: a window ends past the blob")
        mc, _ = self.chunk_plan(lens, params)
        fc = np.zeros(n + 1, np.uint64)
        off, ln = np.zeros(mc, np.uint64), np.zeros(mc, np.uint64)
        fl = np.zeros(mc, np.uint32)
        keys = np.zeros(mc, np.uint64) if hashes else None
        dig = np.zeros((mc, 32), np.uint8) if hashes else None
        consumed = np.zeros(n, np.uint64)
        counts = N.ChunkCounts()
        cp = self._chunk_params(params)
        self._check(self.L.sdcas_chunk_windows(self.ctx, _ptr(blob), _ptr(offsets), _ptr(lens),
                                               None if final is None else _ptr(final), n, ctypes.byref(cp),
                                               _ptr(fc), _ptr(off), _ptr(ln), _ptr(fl),
                                               _ptr(keys) if hashes else None, _ptr(dig) if hashes else None,
                                               _ptr(consumed), ctypes.byref(counts)), "sdcas_chunk_windows")
        m = int(counts.chunks)
        return fc, off[:m].copy(), ln[:m].copy(), fl[:m].copy(), keys[:m].copy() if hashes else None, \
            dig[:m].copy() if hashes else None, counts.as_dict(), consumed

    @staticmethod
    def plan_windows(lens, window_bytes):
        """the windows chunk_stream makes of files of these lengths, taken in
        order (no GPU) -> list of (first_file, n_files, streamed): consecutive
        whole files while they fit in window_bytes together (streamed False),
        a file larger than window_bytes alone, over consecutive windows
        (streamed True, n_files 1)"""
        window_bytes = int(window_bytes)
        if window_bytes <= 0:
            raise ValueError("plan_windows: window_bytes must be positive")
        plan, first, held = [], 0, 0
        for i, n in enumerate(int(v) for v in lens):
            if n > window_bytes:
                if i > first:
                    plan.append((first, i - first, False))
                plan.append((i, 1, True))
                first, held = i + 1, 0
            elif held + n > window_bytes:
                plan.append((first, i - first, False))
                first, held = i, n
            else:
                held += n
        if len(lens) > first:
            plan.append((first, len(lens) - first, False))
        return plan

    def chunk_stream(self, paths, window_bytes=256 << 20, params=None):
        """the chunks of these files without their contents being resident at
        once: a generator over windows of at most window_bytes (plan_windows).
        Whole files share a window, all final; a file larger than window_bytes
        is streamed alone, each window starting at the `consumed` of the one
        before and grown when one consumed nothing, so chunks stay numbered
        file by file. Yields dicts of "chunk_off" (offsets in the file),
        "chunk_len", "chunk_file" (indices into paths), "keys", "digests",
        "counts" (sdcas_chunk_counts of this window), "first_file", "n_files",
        "file_pos" (where a streamed window begins), "final" and "sizes" (the
        bytes read of each of the window's files)."""
        paths = [os.fspath(p) for p in paths]
        lens = [os.path.getsize(p) for p in paths]
        for first, nf, streamed in self.plan_windows(lens, window_bytes):
            if not streamed:
                data = []
                for p in paths[first:first + nf]:
                    with open(p, "rb") as f:
                        data.append(f.read())
                blob, offs, ln_ = self.pack(data)
                fc, off, ln, fl, keys, dig, counts, _ = self.chunk_windows(blob, offs, ln_, None, params)
                yield {"chunk_off": off - offs[fl], "chunk_len": ln, "chunk_file": fl + np.uint32(first), "keys": keys,
                       "digests": dig, "counts": counts, "first_file": first, "n_files": nf, "file_pos": 0,
                       "final": True, "sizes": ln_}
                continue
            pos, want, size = 0, int(window_bytes), lens[first]
            with open(paths[first], "rb") as f:
                while True:
                    f.seek(pos)
                    data = f.read(want)
                    final = pos + len(data) >= size or len(data) < want
                    blob, offs, ln_ = self.pack([data])
                    fc, off, ln, fl, keys, dig, counts, consumed = self.chunk_windows(blob, offs, ln_, [final], params)
                    used = int(consumed[0])
                    if not final and used == 0:
                        want *= 2  # shorter than max_len: nothing could be decided
                        continue
                    yield {"chunk_off": off - offs[fl] + np.uint64(pos), "chunk_len": ln,
                           "chunk_file": fl + np.uint32(first), "keys": keys, "digests": dig, "counts": counts,
                           "first_file": first, "n_files": 1, "file_pos": pos, "final": bool(final),
                           "sizes": np.array([used], np.uint64)}
                    if final:
                        break
                    pos, want = pos + used, int(window_bytes)

    def similar_files_streamed(self, paths, window_bytes=256 << 20, params=None):
        """similar_files for files that need not fit in device memory: the
        chunks come from chunk_stream, window by window; the chunk arrays, keys
        and digests are kept and one confirm and one sharing pass run over all
        of them. The same dict as similar_files, equal to it entry for entry"""
        paths = [os.fspath(p) for p in paths]
        n = len(paths)
        parts = {k: [] for k in ("chunk_off", "chunk_len", "chunk_file", "keys", "digests")}
        sizes = np.zeros(n, np.uint64)
        ccounts = dict.fromkeys((name for name, _ in N.ChunkCounts._fields_), 0)
        for w in self.chunk_stream(paths, window_bytes, params):
            for k in parts:
                parts[k].append(w[k])
            sizes[w["first_file"]:w["first_file"] + w["n_files"]] += w["sizes"]
            for k, v in w["counts"].items():
                ccounts[k] += v
        off = np.concatenate(parts["chunk_off"] or [np.zeros(0, np.uint64)]).astype(np.uint64)
        ln = np.concatenate(parts["chunk_len"] or [np.zeros(0, np.uint64)]).astype(np.uint64)
        fl = np.concatenate(parts["chunk_file"] or [np.zeros(0, np.uint32)]).astype(np.uint32)
        keys = np.concatenate(parts["keys"] or [np.zeros(0, np.uint64)]).astype(np.uint64)
        dig = np.concatenate(parts["digests"] or [np.zeros((0, 32), np.uint8)]).astype(np.uint8)
        fc = np.zeros(n + 1, np.uint64)
        fc[1:] = np.cumsum(np.bincount(fl, minlength=n)[:n])
        rep = self.confirm_duplicates(keys, dig)[0]
        new, own, other, peer, peer_bytes, scounts = self.chunk_sharing(fl, ln, rep, n)
        return {"sizes": sizes, "new_bytes": new, "self_bytes": own, "other_bytes": other, "peer": peer,
                "peer_bytes": peer_bytes, "file_chunks": fc, "chunk_off": off, "chunk_len": ln,
                "chunk_file": fl, "keys": keys, "digests": dig, "rep": rep, "chunk_counts": ccounts,
                "sharing_counts": scounts}

    # -- the chunk index: a batch's chunks against the chunks stored before ------------
    @staticmethod
    def chunk_index_dir_bits(n):
        """sdcas_chunk_index_dir_bits (no GPU): the recommended directory width
        for an index of n entries"""
        return int(N.load().sdcas_chunk_index_dir_bits(int(n)))

    @staticmethod
    def chunk_index_check(keys, digests, dir, bits):
        """sdcas_chunk_index_check (no GPU) over host arrays -> (rc, first_bad):
        (SDCAS_OK, None) for an index as include/sdcas.h defines it,
        (SDCAS_E_INVALID, the first entry or directory slot that is wrong),
        (SDCAS_E_CAPACITY, None) beyond the limits"""
        return Engine._index_check(N.load().sdcas_chunk_index_check, "chunk_index_check", keys, digests, dir, bits)

    @staticmethod
    def _index_check(fn, who, keys, digests, dir, bits, *values):
        """the two checks' body: library function `fn`, named `who` in
        messages; `values` is the holders check's one extra array (or None)"""
        keys, digests, dir = _arr(keys, np.uint64), _arr(digests, np.uint8), _arr(dir, np.uint32)
        values = [None if v is None else _arr(v, np.uint64) for v in values]
        n = keys.size
        if digests.size != 32 * n or any(v is not None and v.size != n for v in values):
            raise ValueError(f"{who}: {n} keys, {digests.size} digest bytes")
        if int(bits) <= N.SDCAS_INDEX_MAX_BITS and dir.size != (1 << int(bits)) + 1:
            raise ValueError(f"{who}: {dir.size} directory slots for {int(bits)} bits")
        bad = ctypes.c_uint64(0)
        rc = fn(_ptr(keys), _ptr(digests), *map(_ptr, values), _ptr(dir), n, int(bits), ctypes.byref(bad))
        return rc, int(bad.value) if rc == N.SDCAS_E_INVALID else None

    @staticmethod
    def _index_arrays(index, who):
        keys, digests, values, dir, bits = index
        keys, digests, dir = _arr(keys, np.uint64), _arr(digests, np.uint8), _arr(dir, np.uint32)
        values = None if values is None else _arr(values, np.uint64)
        n = keys.size
        if digests.size != 32 * n or (values is not None and values.size != n):
            raise ValueError(f"{who}: {n} index keys, {digests.size} digest bytes")
        if n and dir.size != (1 << int(bits)) + 1:
            raise ValueError(f"{who}: {dir.size} directory slots for {int(bits)} bits")
        return keys, digests, values, dir, int(bits)

    @staticmethod
    def _index_batch(keys, digests, valid, who):
        keys, digests = _arr(keys, np.uint64), _arr(digests, np.uint8)
        m = keys.size
        if digests.size != 32 * m:
            raise ValueError(f"{who}: {m} keys, {digests.size} digest bytes")
        va = None if valid is None else _arr(valid, np.uint8)
        if va is not None and va.size != m:
            raise ValueError(f"{who}: {m} keys, {va.size} valid flags")
        return keys, digests, va

    def chunk_index_match(self, index, keys, digests, valid=None):
        """sdcas_chunk_index_match over host arrays. index: (keys uint64[n],
        digests uint8[n, 32], values uint64[n] or None, dir uint32[2^bits + 1],
        bits) -> (pos int64[m]: the entry with the query's key and digest or
        -1, value uint64[m]: its value or 0, counts: dict of
        sdcas_index_match_counts' four fields)"""
        ik, idg, iv, idir, bits = self._index_arrays(index, "chunk_index_match")
        keys, digests, va = self._index_batch(keys, digests, valid, "chunk_index_match")
        m = keys.size
        pos, value = np.zeros(m, np.int64), np.zeros(m, np.uint64)
        counts = N.IndexMatchCounts()
        self._check(self.L.sdcas_chunk_index_match(self.ctx, _ptr(ik), _ptr(idg), _ptr(iv), _ptr(idir), ik.size, bits,
                                                   _ptr(keys), _ptr(digests), _ptr(va), m, _ptr(pos), _ptr(value),
                                                   ctypes.byref(counts)), "sdcas_chunk_index_match")
        return pos, value, counts.as_dict()

    def chunk_index_add(self, index, keys, digests, values, valid=None, bits_new=None):
        """sdcas_chunk_index_add over host arrays: the sorted distinct union
        of the index (chunk_index_match's tuple) and the batch's valid pairs,
        with its directory at bits_new (None: the recommended width for n + m)
        -> (new index tuple, trimmed to entries_new, pos int64[m], flags
        uint8[m]: SDCAS_INDEX_HIT / ADDED / SKIPPED or 0, counts: dict of
        sdcas_index_add_counts' six fields)"""
        return self._index_add(self.L.sdcas_chunk_index_add, "chunk_index_add", index, keys, digests, values, valid,
                               bits_new)

    def _index_add(self, fn, who, index, keys, digests, values, valid, bits_new):
        """the two host adds' body: library function `fn`, named `who` in messages"""
        ik, idg, iv, idir, bits = self._index_arrays(index, who)
        keys, digests, va = self._index_batch(keys, digests, valid, who)
        m, n = keys.size, ik.size
        values = None if values is None else _arr(values, np.uint64)
        if values is not None and values.size != m:
            raise ValueError(f"{who}: {m} keys, {values.size} values")
        if bits_new is None:
            bits_new = self.chunk_index_dir_bits(n + m)
        bits_new = int(bits_new)
        if not 0 <= bits_new <= N.SDCAS_INDEX_MAX_BITS:
            raise N.SdcasError(N.SDCAS_E_CAPACITY, f"{who}: a directory of {bits_new} bits")
        nk, nd, nv = np.zeros(n + m, np.uint64), np.zeros((n + m, 32), np.uint8), np.zeros(n + m, np.uint64)
        ndir = np.zeros((1 << bits_new) + 1, np.uint32)
        pos, flags = np.zeros(m, np.int64), np.zeros(m, np.uint8)
        counts = N.IndexAddCounts()
        self._check(fn(self.ctx, _ptr(ik), _ptr(idg), _ptr(iv), _ptr(idir), n, bits, _ptr(keys), _ptr(digests),
                       _ptr(values), _ptr(va), m, nk.ctypes.data, nd.ctypes.data, nv.ctypes.data, ndir.ctypes.data,
                       bits_new, _ptr(pos), _ptr(flags), ctypes.byref(counts)), "sdcas_" + who)
        e = int(counts.entries_new)
        return (nk[:e].copy(), nd[:e].copy(), nv[:e].copy(), ndir, bits_new), pos, flags, counts.as_dict()

    # -- the holders index: a chunk index that keeps every holder and can forget files --
    @staticmethod
    def chunk_holders_check(keys, digests, values, dir, bits):
        """sdcas_chunk_holders_check (no GPU) over host arrays -> (rc,
        first_bad) as chunk_index_check, in the order of the triple (key,
        digest, value); values None: all 0"""
        return Engine._index_check(N.load().sdcas_chunk_holders_check, "chunk_holders_check", keys, digests, dir, bits,
                                   values)

    def chunk_holders_match(self, index, keys, digests, valid=None):
        """sdcas_chunk_holders_match over host arrays; index as for
        chunk_index_match -> (pos int64[m]: the FIRST entry with the query's
        pair or -1, value uint64[m]: its value (the lowest holder) or 0,
        holders uint32[m]: the entries with the pair, counts)"""
        ik, idg, iv, idir, bits = self._index_arrays(index, "chunk_holders_match")
        keys, digests, va = self._index_batch(keys, digests, valid, "chunk_holders_match")
        m = keys.size
        pos, value, holders = np.zeros(m, np.int64), np.zeros(m, np.uint64), np.zeros(m, np.uint32)
        counts = N.IndexMatchCounts()
        self._check(self.L.sdcas_chunk_holders_match(self.ctx, _ptr(ik), _ptr(idg), _ptr(iv), _ptr(idir), ik.size,
                                                     bits, _ptr(keys), _ptr(digests), _ptr(va), m, _ptr(pos),
                                                     _ptr(value), _ptr(holders), ctypes.byref(counts)),
                    "sdcas_chunk_holders_match")
        return pos, value, holders, counts.as_dict()

    def chunk_holders_add(self, index, keys, digests, values, valid=None, bits_new=None):
        """sdcas_chunk_holders_add over host arrays: the sorted distinct union
        of the index's triples and the batch's valid (key, digest, value)
        triples -> (new index tuple, trimmed to entries_new, pos int64[m],
        flags uint8[m], counts), as chunk_index_add but read per triple"""
        return self._index_add(self.L.sdcas_chunk_holders_add, "chunk_holders_add", index, keys, digests, values, valid,
                               bits_new)

    def chunk_holders_remove(self, index, removed, bits_new=None):
        """sdcas_chunk_holders_remove over host arrays: the index's entries
        whose value is not in `removed` (uint64, strictly ascending), in their
        order, with the directory at bits_new (None: the index's width) ->
        (new index tuple, trimmed to entries_new, counts: dict of
        sdcas_holders_remove_counts' four fields)"""
        ik, idg, iv, idir, bits = self._index_arrays(index, "chunk_holders_remove")
        removed = _arr(removed, np.uint64)
        n = ik.size
        bits_new = bits if bits_new is None else int(bits_new)
        if not 0 <= bits_new <= N.SDCAS_INDEX_MAX_BITS:
            raise N.SdcasError(N.SDCAS_E_CAPACITY, f"chunk_holders_remove: a directory of {bits_new} bits")
        nk, nd, nv = np.zeros(n, np.uint64), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint64)
        ndir = np.zeros((1 << bits_new) + 1, np.uint32)
        counts = N.HoldersRemoveCounts()
        self._check(self.L.sdcas_chunk_holders_remove(self.ctx, _ptr(ik), _ptr(idg), _ptr(iv), _ptr(idir), n, bits,
                                                      _ptr(removed), removed.size, nk.ctypes.data, nd.ctypes.data,
                                                      nv.ctypes.data, ndir.ctypes.data, bits_new,
                                                      ctypes.byref(counts)), "sdcas_chunk_holders_remove")
        e = int(counts.entries_new)
        return (nk[:e].copy(), nd[:e].copy(), nv[:e].copy(), ndir, bits_new), counts.as_dict()

    # -- chunk peers: per file, the top-k files by shared bytes over every holder ------
    @staticmethod
    def _peers_mode(mode):
        try:
            return {"earlier": N.SDCAS_PEERS_EARLIER, "all": N.SDCAS_PEERS_ALL}[mode]
        except (KeyError, TypeError):
            return int(mode)

    @staticmethod
    def chunk_peers_plan(m, n_files, k, max_holders):
        """sdcas_chunk_peers_plan (no GPU) -> (max_pairs: min(m * max_holders,
        2^30), the bound that cannot overflow, workspace_bytes: what the device
        call takes for that many pairs); SdcasError beyond the ranges"""
        pairs, ws = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = N.load().sdcas_chunk_peers_plan(int(m), int(n_files), int(k), int(max_holders), ctypes.byref(pairs),
                                             ctypes.byref(ws))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, f"chunk_peers_plan({m}, {n_files}, k={k}, max_holders={max_holders})")
        return int(pairs.value), int(ws.value)

    def chunk_peers(self, index, keys, digests, chunk_file, chunk_len, file_ids, k=4, max_holders=64, mode="earlier",
                    valid=None, max_pairs=0):
        """sdcas_chunk_peers over host arrays; index as for chunk_holders_match,
        the batch as for chunk_sharing plus its keys and digests, file_ids
        uint64[n_files]: the id each batch file has in the index. mode
        "earlier": a chunk's counted holders are the index's entries below the
        file's own id, "all": every entry but the file's own; a chunk with more
        than max_holders of them is common and scores for nobody. max_pairs 0:
        the plan's bound. -> dict: "peer_count" uint32[n], "peers" uint64[n, k]
        (by bytes descending, then id ascending; unused slots 0), "peers_bytes"
        uint64[n, k], "shared_bytes", "unique_bytes", "common_bytes" uint64[n],
        "counts": sdcas_peers_counts' seven fields. SdcasError
        (SDCAS_E_CAPACITY) when the pairs exceed max_pairs."""
        ik, idg, iv, idir, bits = self._index_arrays(index, "chunk_peers")
        keys, digests, va = self._index_batch(keys, digests, valid, "chunk_peers")
        m = keys.size
        fl, ln, ids = _arr(chunk_file, np.uint32), _arr(chunk_len, np.uint64), _arr(file_ids, np.uint64)
        if fl.size != m or ln.size != m:
            raise ValueError(f"chunk_peers: {m} keys, {fl.size} chunk files, {ln.size} chunk lengths")
        n, k = ids.size, int(k)
        if not 1 <= k <= N.SDCAS_PEERS_MAX_K:
            raise N.SdcasError(N.SDCAS_E_INVALID, f"chunk_peers: k = {k}")
        cnt, peers, pb = np.zeros(n, np.uint32), np.zeros((n, k), np.uint64), np.zeros((n, k), np.uint64)
        shared, unique, common = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        counts = N.PeersCounts()
        self._check(self.L.sdcas_chunk_peers(self.ctx, _ptr(ik), _ptr(idg), _ptr(iv), _ptr(idir), ik.size, bits,
                                             _ptr(keys), _ptr(digests), _ptr(va), _ptr(fl), _ptr(ln), m, _ptr(ids), n,
                                             k, int(max_holders), self._peers_mode(mode), int(max_pairs),
                                             cnt.ctypes.data, peers.ctypes.data, pb.ctypes.data, shared.ctypes.data,
                                             unique.ctypes.data, common.ctypes.data, ctypes.byref(counts)),
                    "sdcas_chunk_peers")
        return {"peer_count": cnt, "peers": peers, "peers_bytes": pb, "shared_bytes": shared, "unique_bytes": unique,
                "common_bytes": common, "counts": counts.as_dict()}

    def similar_files_indexed(self, paths, file_ids, index, params=None, window_bytes=256 << 20, peers=0,
                              max_holders=64, chunks=False):
        """similar_files_streamed against what earlier calls stored: the files
        are chunked through chunk_stream, their chunks confirmed within the
        batch, matched against `index` (a ChunkIndex or a ChunkHolders) and
        then added to it with the value file_ids[chunk_file]. The origin of a
        chunk is the stored value when the index holds it (a ChunkIndex: the
        first owner; a ChunkHolders: the lowest holder that was not removed),
        else the id of the file of its lowest copy in the batch; `peer` is a FILE ID (from file_ids or a
        stored value; ties go to the lowest id), -1 for none. Every listed
        file has its own id, also a path listed twice. -> dict with the per-file
        arrays "sizes", "new_bytes", "self_bytes", "other_bytes",
        "indexed_bytes" (the bytes of chunks the index held before the call),
        "peer", "peer_bytes", and "chunk_counts", "match_counts", "add_counts".
        For ids ascending in scan order and any split of the files into
        consecutive calls on one index that started empty, the per-file
        results are similar_files_streamed's over all the files at once, with
        its peer mapped through the ids.

        peers=k > 0 (a ChunkHolders only; ValueError with a ChunkIndex) adds,
        after the add and still on the index's stream, ChunkHolders.peers in
        "earlier" mode over the batch's device arrays: "peers" uint64[n, k]
        (the k files below the file's own id that hold most of its bytes,
        counting EVERY holder of a chunk, not only its origin; by bytes
        descending, then id ascending; unused slots 0), "peers_bytes"
        uint64[n, k], "peer_count" uint32[n], "shared_bytes", "common_bytes"
        (chunks with more than max_holders counted holders score for nobody)
        and "peers_counts". `peer` answers "the lowest holder of most of my
        chunks", peers[:, 0] "the file that holds most of my bytes": of three
        versions of a growing log the third's peer is the first, its first
        peer the second. The same law holds for these keys (but
        "peers_counts", which is per call): for ids ascending in scan order
        and any split of the files into consecutive calls on a holders index
        that started empty, every file's rows equal those of one call over all
        the files — in "earlier" mode a file's result does not depend on which
        later files the index holds — and after remove(R) the rows of the later
        batches equal those of one run over the survivors and those batches.
        With peers=0 the calls and the dict are what they were.

        chunks=True adds the batch's chunk arrays, which the call holds anyway:
        "chunk_file" uint32[m] (rows of this call), "chunk_len" uint64[m],
        "chunk_keys" uint64[m] and "chunk_digests" uint8[m, 32]; the index
        keeps no lengths, so a caller that wants family_bytes_of keeps these.
        With the default the dict is what it was."""
        import torch

        if peers and not isinstance(index, ChunkHolders):
            raise ValueError("similar_files_indexed: peers needs a ChunkHolders (ChunkHolders.from_index converts)")

        paths = [os.fspath(p) for p in paths]
        n = len(paths)
        ids = _arr(file_ids, np.uint64)
        if ids.size != n:
            raise ValueError(f"similar_files_indexed: {n} paths, {ids.size} file ids")
        if np.unique(ids).size != n:
            raise ValueError("similar_files_indexed: file ids must be distinct")
        parts = {k: [] for k in ("chunk_len", "chunk_file", "keys", "digests")}
        sizes = np.zeros(n, np.uint64)
        ccounts = dict.fromkeys((name for name, _ in N.ChunkCounts._fields_), 0)
        for w in self.chunk_stream(paths, window_bytes, params):
            for k in parts:
                parts[k].append(w[k])
            sizes[w["first_file"]:w["first_file"] + w["n_files"]] += w["sizes"]
            for k, v in w["counts"].items():
                ccounts[k] += v
        ln = np.concatenate(parts["chunk_len"] or [np.zeros(0, np.uint64)]).astype(np.uint64)
        fl = np.concatenate(parts["chunk_file"] or [np.zeros(0, np.uint32)]).astype(np.uint32)
        keys = np.concatenate(parts["keys"] or [np.zeros(0, np.uint64)]).astype(np.uint64)
        dig = np.concatenate(parts["digests"] or [np.zeros((0, 32), np.uint8)]).astype(np.uint8)
        m = keys.size
        if index.engine is not self:
            raise ValueError("similar_files_indexed: the index belongs to another engine")
        with torch.cuda.stream(index.stream):  # the batch goes up once; confirm, match and add run on the index's stream
            d_keys, d_dig = index._upload(keys, np.int64), index._upload(dig, np.uint8)
            d_rep = torch.empty(m, dtype=torch.int64, device=index.device)
            self.dev_confirm_duplicates(d_keys.data_ptr(), d_dig.data_ptr(), 0, m, rep=d_rep.data_ptr(),
                                        stream=index.stream.cuda_stream)
            d_pos, d_val, mcounts = index._match_dev(d_keys, d_dig, None)
            rep, hit, val = d_rep.cpu().numpy(), d_pos.cpu().numpy() >= 0, d_val.cpu().numpy().view(np.uint64)
            acounts = index._add_dev(d_keys, d_dig, index._upload(ids[fl], np.int64), None)[2]
            near = index._peers_dev(d_keys, d_dig, None, index._upload(fl, np.int32), index._upload(ln, np.int64),
                                    index._upload(ids, np.int64), n, int(peers), int(max_holders),
                                    N.SDCAS_PEERS_EARLIER) if peers else None
        # One pseudo-chunk of length 0 per chunk that is its pair's lowest in
        # the batch and hits the index, in front of the batch's chunks, owned
        # by a pseudo file that stands for the stored owner: a batch chunk with
        # a hit then has its lowest copy there. Files get ordinals by the rank
        # of their id over the stored owners and the batch's ids, so that the
        # sharing pass's tie rule (the lowest ordinal) is the lowest id.
        heads = np.flatnonzero(hit & (rep == np.arange(m)))
        all_ids = np.union1d(val[heads], ids)
        ordinal = np.searchsorted(all_ids, ids).astype(np.uint32)
        nh = heads.size
        s_file = np.concatenate([np.searchsorted(all_ids, val[heads]).astype(np.uint32), ordinal[fl]])
        s_len = np.concatenate([np.zeros(nh, np.uint64), ln])
        slot = np.full(m, -1, np.int64)
        slot[heads] = np.arange(nh)
        s_rep = np.concatenate([np.arange(nh, dtype=np.int64), np.where(hit, slot[rep], rep + nh)])
        new, own, other, peer, peer_bytes, _ = self.chunk_sharing(s_file, s_len, s_rep, all_ids.size)
        indexed = np.zeros(n, np.uint64)
        np.add.at(indexed, fl[hit], ln[hit])
        peer = peer[ordinal]
        out = {"sizes": sizes, "new_bytes": new[ordinal], "self_bytes": own[ordinal], "other_bytes": other[ordinal],
               "indexed_bytes": indexed, "peer": np.where(peer >= 0, all_ids[np.maximum(peer, 0)].astype(np.int64), -1),
               "peer_bytes": peer_bytes[ordinal], "chunk_counts": ccounts, "match_counts": mcounts,
               "add_counts": acounts}
        if near is not None:
            out.update({"peers": near["peers"], "peers_bytes": near["peers_bytes"], "peer_count": near["peer_count"],
                        "shared_bytes": near["shared_bytes"], "common_bytes": near["common_bytes"],
                        "peers_counts": near["counts"]})
        if chunks:
            out.update({"chunk_file": fl, "chunk_len": ln, "chunk_keys": keys, "chunk_digests": dig.reshape(-1, 32)})
        return out

    # -- file families: the connected components of the peer rows ---------------------
    @staticmethod
    def file_families_plan(n, k):
        """sdcas_file_families_plan (no GPU) -> workspace_bytes: what the device
        call takes for n rows; SdcasError beyond the ranges"""
        ws = ctypes.c_uint64(0)
        rc = N.load().sdcas_file_families_plan(int(n), int(k), ctypes.byref(ws))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, f"file_families_plan({n}, k={k})")
        return int(ws.value)

    def file_families(self, ids, sizes, peer_count, peers, peer_bytes, num=1, den=2, sets=False):
        """sdcas_file_families over host arrays: ids uint64[n] strictly
        ascending, sizes uint64[n], and chunk_peers' "peer_count" uint32[n],
        "peers" and "peers_bytes" uint64[n, k] as they are. A slot links row i
        and the row j of its peer when it shares b > 0 bytes with b * den >=
        num * max(sizes[i], sizes[j]); the default 1/2, "half of the larger
        file", is a documented choice, not a measurement. -> dict: "family"
        int64[n] (the lowest row of the row's component), "family_size"
        uint32[n], "counts": sdcas_families_counts' ten fields. sets=True adds
        duplicate_sets(family, None, SDCAS_SETS_BY_REP): "set_rep",
        "set_offsets" and "members", one set per family of two rows or more.
        SdcasError (SDCAS_E_INVALID) when ids is not strictly ascending."""
        ids, sz, pc = _arr(ids, np.uint64), _arr(sizes, np.uint64), _arr(peer_count, np.uint32)
        pe, pb = np.ascontiguousarray(peers, np.uint64), np.ascontiguousarray(peer_bytes, np.uint64)
        n = ids.size
        if sz.size != n or pc.size != n:
            raise ValueError(f"file_families: {n} ids, {sz.size} sizes, {pc.size} peer counts")
        if pe.shape != pb.shape or pe.ndim != 2 or pe.shape[0] != n:
            raise ValueError(f"file_families: peers {pe.shape} and peer bytes {pb.shape} are not both [{n}, k]")
        k = int(pe.shape[1])
        if not 1 <= k <= N.SDCAS_PEERS_MAX_K:
            raise N.SdcasError(N.SDCAS_E_INVALID, f"file_families: k = {k}")
        family, fsize = np.zeros(n, np.int64), np.zeros(n, np.uint32)
        counts = N.FamiliesCounts()
        self._check(self.L.sdcas_file_families(self.ctx, _ptr(ids), _ptr(sz), _ptr(pc), _ptr(pe.reshape(-1)),
                                               _ptr(pb.reshape(-1)), n, k, int(num), int(den), family.ctypes.data,
                                               fsize.ctypes.data, ctypes.byref(counts)), "sdcas_file_families")
        out = {"family": family, "family_size": fsize, "counts": counts.as_dict()}
        if sets:
            set_rep, set_offsets, _, members, _ = self.duplicate_sets(family, None, N.SDCAS_SETS_BY_REP)
            out.update({"set_rep": set_rep, "set_offsets": set_offsets, "members": members})
        return out

    def families_of(self, results, file_ids, num=1, den=2):
        """the families over consecutive similar_files_indexed(..., peers=k)
        calls: `results` their dicts and `file_ids` their id arrays, in call
        order (ids ascending throughout, one k throughout; a removed file's
        row dropped from both). Concatenates "sizes", "peer_count", "peers" and
        "peers_bytes" and calls file_families(..., sets=True); rows are numbered
        in that order. A peer id that is no longer listed is a missing slot."""
        results, file_ids = list(results), [_arr(x, np.uint64) for x in file_ids]
        if len(results) != len(file_ids):
            raise ValueError(f"families_of: {len(results)} results, {len(file_ids)} id arrays")
        for r in results:
            if "peers" not in r:
                raise ValueError("families_of: a result has no peers (similar_files_indexed(..., peers=k))")
        ks = {int(np.asarray(r["peers"]).shape[1]) for r in results}
        if len(ks) > 1:
            raise ValueError(f"families_of: the results have different k: {sorted(ks)}")
        k = ks.pop() if ks else 1

        def cat(key, dtype, *tail):
            return np.concatenate([np.zeros((0,) + tail, dtype)] +
                                  [np.asarray(r[key], dtype).reshape((-1,) + tail) for r in results])
        ids = np.concatenate([np.zeros(0, np.uint64)] + file_ids)
        return self.file_families(ids, cat("sizes", np.uint64), cat("peer_count", np.uint32), cat("peers", np.uint64, k),
                                  cat("peers_bytes", np.uint64, k), num, den, sets=True)

    # -- family bytes: what a family's versions store and give back ---------------------
    @staticmethod
    def family_bytes_plan(m, n_files):
        """sdcas_family_bytes_plan (no GPU) -> workspace_bytes: what the device
        call takes for m chunks of n_files rows; SdcasError beyond the ranges"""
        ws = ctypes.c_uint64(0)
        rc = N.load().sdcas_family_bytes_plan(int(m), int(n_files), ctypes.byref(ws))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, f"family_bytes_plan({m}, {n_files})")
        return int(ws.value)

    def family_bytes(self, chunk_file, chunk_len, rep, family, sets=False):
        """sdcas_family_bytes over host arrays: chunk_sharing's chunk_file
        uint32[m], chunk_len uint64[m] and rep int64[m], and a label per row,
        family int64[n] (file_families' "family" as it is; values outside
        [0, n) take no part). A chunk's class is (label of its row, class
        number); its bytes are the row's delta when it is the class's first
        occurrence, self when that lies earlier in the row itself, inherited
        when it lies in another row of the family. -> dict: "file_bytes",
        "delta_bytes", "self_bytes", "inherited_bytes" uint64[n]; per label
        with two rows or more, most reclaimable first (ties by lowest row):
        "set_rep" int64[S], "set_files" uint32[S], "set_total", "set_stored"
        and "set_reclaimable" (total - stored) uint64[S]; "counts":
        sdcas_family_bytes_counts' nine fields. sets=True adds "set_offsets"
        uint64[S + 1] and "members" int64[M] in the same set order: they come
        from duplicate_sets(family, None, SDCAS_SETS_BY_REP), permuted on the
        host through its set_rep; that host step follows the number of sets
        and members, not the chunks."""
        fl, ln, rp = _arr(chunk_file, np.uint32), _arr(chunk_len, np.uint64), _arr(rep, np.int64)
        fam = _arr(family, np.int64)
        m, n = fl.size, fam.size
        if ln.size != m or rp.size != m:
            raise ValueError(f"family_bytes: {m} chunk files, {ln.size} lengths, {rp.size} reps")
        h = n // 2
        rows = [np.zeros(n, np.uint64) for _ in range(4)]
        set_rep, set_files = np.zeros(h, np.int64), np.zeros(h, np.uint32)
        set_total, set_stored = np.zeros(h, np.uint64), np.zeros(h, np.uint64)
        counts = N.FamilyBytesCounts()
        self._check(self.L.sdcas_family_bytes(self.ctx, _ptr(fl), _ptr(ln), _ptr(rp), m, _ptr(fam), n,
                                              *(a.ctypes.data for a in rows), set_rep.ctypes.data,
                                              set_files.ctypes.data, set_total.ctypes.data, set_stored.ctypes.data,
                                              ctypes.byref(counts)), "sdcas_family_bytes")
        s = int(counts.sets)
        out = {"file_bytes": rows[0], "delta_bytes": rows[1], "self_bytes": rows[2], "inherited_bytes": rows[3],
               "set_rep": set_rep[:s].copy(), "set_files": set_files[:s].copy(), "set_total": set_total[:s].copy(),
               "set_stored": set_stored[:s].copy(), "set_reclaimable": set_total[:s] - set_stored[:s],
               "counts": counts.as_dict()}
        if sets:
            by_rep, offs, _, members, _ = self.duplicate_sets(fam, None, N.SDCAS_SETS_BY_REP)
            pos = np.searchsorted(by_rep, out["set_rep"])  # by_rep ascends; both list the same sets
            if pos.size and (pos.max(initial=0) >= by_rep.size or not np.array_equal(by_rep[pos], out["set_rep"])):
                raise RuntimeError("family_bytes: the sets of duplicate_sets and of family_bytes differ")
            lens = (offs[1:] - offs[:-1])[pos].astype(np.int64)
            new_offs = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])
            take = np.repeat(offs[:-1][pos].astype(np.int64) - new_offs[:-1], lens) + np.arange(new_offs[-1])
            out.update({"set_offsets": new_offs.astype(np.uint64), "members": members[take]})
        return out

    def family_bytes_of(self, results, file_ids, num=1, den=2):
        """families_of plus the bytes: over consecutive
        similar_files_indexed(..., peers=k, chunks=True) calls, `results` their
        dicts and `file_ids` their id arrays in call order. The families are
        families_of's; the chunk arrays are concatenated ("chunk_file" shifted
        by the rows before), confirm_duplicates over the concatenated (key,
        digest) pairs gives rep, and family_bytes(..., sets=True) runs over
        them. -> families_of's dict merged with family_bytes': where both have
        a key ("set_rep", "set_offsets", "members", "counts") families_of's
        goes under "families_" + key and the reclaimable-ordered form keeps the
        plain name. ValueError when a result lacks the chunk arrays or its rows
        do not match its ids: dropped rows are not supported here."""
        fam, fl, ln, rep = self._family_inputs(results, file_ids, num, den, "family_bytes_of")
        return self._family_bytes_merged(fam, fl, ln, rep)

    def _family_inputs(self, results, file_ids, num, den, who):
        """family_bytes_of's and family_recipes_of's common start -> (families_of's
        dict, chunk_file, chunk_len, rep) over the concatenated rows"""
        results, file_ids = list(results), [_arr(x, np.uint64) for x in file_ids]
        if len(results) != len(file_ids):
            raise ValueError(f"{who}: {len(results)} results, {len(file_ids)} id arrays")
        for r in results:
            for key in ("chunk_file", "chunk_len", "chunk_keys", "chunk_digests"):
                if key not in r:
                    raise ValueError(f"{who}: a result has no {key} (similar_files_indexed(..., chunks=True))")
        fl, ln, keys, dig, row0 = [], [], [], [], 0
        for r, ids in zip(results, file_ids):
            cf = _arr(r["chunk_file"], np.uint32)
            if np.asarray(r["sizes"]).size != ids.size or (cf.size and int(cf.max()) >= ids.size):
                raise ValueError(f"{who}: a result's rows do not match its ids (dropped rows are not supported)")
            fl.append((cf.astype(np.uint64) + row0).astype(np.uint32))
            ln.append(_arr(r["chunk_len"], np.uint64))
            keys.append(_arr(r["chunk_keys"], np.uint64))
            dig.append(_arr(r["chunk_digests"], np.uint8).reshape(-1, 32))
            row0 += ids.size
        fl = np.concatenate([np.zeros(0, np.uint32)] + fl)
        ln = np.concatenate([np.zeros(0, np.uint64)] + ln)
        keys = np.concatenate([np.zeros(0, np.uint64)] + keys)
        dig = np.concatenate([np.zeros((0, 32), np.uint8)] + dig)
        fam = self.families_of(results, file_ids, num, den)
        rep = self.confirm_duplicates(keys, dig)[0]
        return fam, fl, ln, rep

    def _family_bytes_merged(self, fam, fl, ln, rep):
        out = dict(fam)
        for key in ("set_rep", "set_offsets", "members", "counts"):
            out["families_" + key] = out.pop(key)
        out.update(self.family_bytes(fl, ln, rep, fam["family"], sets=True))
        return out

    def similar_families(self, paths, k=4, max_holders=64, num=1, den=2, params=None, window_bytes=256 << 20):
        """the families of these files and their bytes in one call, with no
        index for the caller to keep: family_bytes_of over one
        similar_files_indexed(paths, arange(n), ChunkHolders(self), ...,
        peers=k, chunks=True). Rows are the paths in order. -> that dict plus
        "sizes". The steps go through the host forms."""
        paths = [os.fspath(p) for p in paths]
        ids = np.arange(len(paths), dtype=np.uint64)
        r = self.similar_files_indexed(paths, ids, ChunkHolders(self), params, window_bytes, peers=int(k),
                                       max_holders=max_holders, chunks=True)
        out = self.family_bytes_of([r], [ids], num, den)
        out["sizes"] = r["sizes"]
        return out

    # -- family recipes: the byte ranges that rebuild every file from its family's stored bytes
    @staticmethod
    def family_recipes_plan(m, n_files):
        """sdcas_family_recipes_plan (no GPU) -> workspace_bytes: what the device
        call takes for m chunks of n_files rows; SdcasError beyond the ranges"""
        ws = ctypes.c_uint64(0)
        rc = N.load().sdcas_family_recipes_plan(int(m), int(n_files), ctypes.byref(ws))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, f"family_recipes_plan({m}, {n_files})")
        return int(ws.value)

    @staticmethod
    def running_offsets(chunk_file, chunk_len):
        """the per-file running sums of chunk_len in position order, uint64[m]
        (modulo 2^64): a chunk's offset in its file when the chunks of a file
        cover it in order, as every chunker here writes them"""
        fl, ln = _arr(chunk_file, np.uint32), _arr(chunk_len, np.uint64)
        if fl.size != ln.size:
            raise ValueError(f"running_offsets: {fl.size} chunk files, {ln.size} lengths")
        order = np.argsort(fl, kind="stable")
        sf, sl = fl[order], ln[order]
        before = np.cumsum(sl, dtype=np.uint64) - sl
        start = np.flatnonzero(np.concatenate([np.ones(min(sf.size, 1), bool), sf[1:] != sf[:-1]]))
        runs = np.diff(np.concatenate([start, [sf.size]]))
        off = np.zeros(fl.size, np.uint64)
        off[order] = before - np.repeat(before[start], runs)
        return off

    def family_recipes(self, chunk_file, chunk_len, rep, family, chunk_off=None):
        """sdcas_family_recipes over host arrays: family_bytes' inputs and
        chunk_off uint64[m], a chunk's offset in its file (None: the per-file
        running sums of chunk_len in position order, computed on the host). ->
        dict: per op, in order of the head chunks, "op_chunk", "op_src_chunk",
        "op_row", "op_src_row" uint32[ops], "op_dst_off", "op_src_off", "op_len"
        uint64[ops] and "op_literal" bool[ops] (the row keeps these bytes; else
        the op copies op_len bytes from op_src_off of op_src_row); "chunk_op"
        uint32[m] (0xFFFFFFFF: the chunk takes no part); "row_ops" and
        "row_first_op" uint32[n] (a row of adjacent chunks has the ops
        [row_first_op, row_first_op + row_ops)); "chunk_off" as used; "counts":
        sdcas_family_recipes_counts' eight fields. rebuild_files applies them."""
        fl, ln, rp = _arr(chunk_file, np.uint32), _arr(chunk_len, np.uint64), _arr(rep, np.int64)
        fam = _arr(family, np.int64)
        m, n = fl.size, fam.size
        if ln.size != m or rp.size != m:
            raise ValueError(f"family_recipes: {m} chunk files, {ln.size} lengths, {rp.size} reps")
        off = self.running_offsets(fl, ln) if chunk_off is None else _arr(chunk_off, np.uint64)
        if off.size != m:
            raise ValueError(f"family_recipes: {m} chunk files, {off.size} offsets")
        op32 = [np.zeros(m, np.uint32) for _ in range(4)]
        op64 = [np.zeros(m, np.uint64) for _ in range(3)]
        chunk_op, row_ops, row_first = np.zeros(m, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        counts = N.FamilyRecipesCounts()
        self._check(self.L.sdcas_family_recipes(self.ctx, _ptr(fl), _ptr(off), _ptr(ln), _ptr(rp), m, _ptr(fam), n,
                                                *(a.ctypes.data for a in op32 + op64), chunk_op.ctypes.data,
                                                row_ops.ctypes.data, row_first.ctypes.data, ctypes.byref(counts)),
                    "sdcas_family_recipes")
        k = int(counts.ops)
        names = ("op_chunk", "op_src_chunk", "op_row", "op_src_row", "op_dst_off", "op_src_off", "op_len")
        out = {name: a[:k].copy() for name, a in zip(names, op32 + op64)}
        out.update({"op_literal": out["op_chunk"] == out["op_src_chunk"], "chunk_op": chunk_op, "row_ops": row_ops,
                    "row_first_op": row_first, "chunk_off": off, "counts": counts.as_dict()})
        return out

    def family_recipes_of(self, results, file_ids, num=1, den=2):
        """family_bytes_of plus the recipes: its inputs, its dict, and under
        "recipes" family_recipes' dict over the same concatenated chunk arrays,
        rep and families, with chunk_off the per-file running sums (the chunks
        of a file cover it in order). Rows are numbered as in families_of.
        ValueError as family_bytes_of: dropped rows are not supported here."""
        fam, fl, ln, rep = self._family_inputs(results, file_ids, num, den, "family_recipes_of")
        out = self._family_bytes_merged(fam, fl, ln, rep)
        out["recipes"] = self.family_recipes(fl, ln, rep, fam["family"])
        return out

    def similar_recipes(self, paths, k=4, max_holders=64, num=1, den=2, params=None, window_bytes=256 << 20):
        """similar_families plus the recipes: family_recipes_of over one
        similar_files_indexed(paths, arange(n), ChunkHolders(self), ...,
        peers=k, chunks=True). Rows are the paths in order. -> similar_families'
        dict plus "recipes"; rebuild_files(out["recipes"], read) gives every
        file back from the literal ranges alone."""
        paths = [os.fspath(p) for p in paths]
        ids = np.arange(len(paths), dtype=np.uint64)
        r = self.similar_files_indexed(paths, ids, ChunkHolders(self), params, window_bytes, peers=int(k),
                                       max_holders=max_holders, chunks=True)
        out = self.family_recipes_of([r], [ids], num, den)
        out["sizes"] = r["sizes"]
        return out

    # -- family store: the literal bytes packed into one store, files restored from it
    @staticmethod
    def family_store_tile_bytes():
        """sdcas_family_store_tile_bytes (no GPU): the mover's tile in destination bytes"""
        return int(N.load().sdcas_family_store_tile_bytes())

    @staticmethod
    def family_store_plan(max_ops, n_files):
        """sdcas_family_store_plan (no GPU) -> workspace_bytes: what the layout,
        pack and restore device calls share for max_ops ops; SdcasError beyond
        the ranges"""
        ws = ctypes.c_uint64(0)
        rc = N.load().sdcas_family_store_plan(int(max_ops), int(n_files), ctypes.byref(ws))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, f"family_store_plan({max_ops}, {n_files})")
        return int(ws.value)

    @staticmethod
    def _store_ops(recipes, who):
        u32 = [_arr(recipes[k], np.uint32) for k in ("op_chunk", "op_src_chunk", "op_row", "op_src_row")]
        u64 = [_arr(recipes[k], np.uint64) for k in ("op_dst_off", "op_src_off", "op_len")]
        k = u32[0].size
        if not all(a.size == k for a in u32 + u64):
            raise ValueError(f"{who}: the op arrays differ in length")
        return u32 + u64, k

    def family_store_layout(self, recipes):
        """sdcas_family_store_layout over family_recipes' dict -> {"op_store_off":
        uint64[ops], 2^64 - 1 for an uncovered copy op; "counts":
        sdcas_family_store_counts' six fields}"""
        ops, k = self._store_ops(recipes, "family_store_layout")
        chunk_op = _arr(recipes["chunk_op"], np.uint32)
        off = np.zeros(k, np.uint64)
        counts = N.FamilyStoreCounts()
        self._check(self.L.sdcas_family_store_layout(self.ctx, *(_ptr(a) for a in ops), k, _ptr(chunk_op),
                                                     chunk_op.size, _ptr(off), ctypes.byref(counts)),
                    "sdcas_family_store_layout")
        return {"op_store_off": off, "counts": counts.as_dict()}

    @staticmethod
    def _store_rows(row_at, row_len, row_base, who):
        at, ln = _arr(row_at, np.uint64), _arr(row_len, np.uint64)
        base = None if row_base is None else _arr(row_base, np.uint64)
        if ln.size != at.size or (base is not None and base.size != at.size):
            raise ValueError(f"{who}: row_at, row_len and row_base differ in length")
        return at, base, ln

    def family_pack(self, recipes, layout, blob, row_at, row_len, row_base=None, store=None, counts=None):
        """sdcas_family_pack over host arrays: the literal ops' bytes from the
        rows' windows in `blob` (row i's bytes [row_base[i], row_base[i] +
        row_len[i]) at blob[row_at[i]:]; row_len 0: the row is not there) into
        the store. `store`: an earlier call's store to pack further windows
        into (None: store_bytes zeros). -> the store, uint8. `counts`, a dict,
        receives sdcas_family_move_counts' four fields."""
        ops, k = self._store_ops(recipes, "family_pack")
        off = _arr(layout["op_store_off"], np.uint64)
        if off.size != k:
            raise ValueError(f"family_pack: {k} ops, {off.size} store offsets")
        at, base, ln = self._store_rows(row_at, row_len, row_base, "family_pack")
        blob = _arr(blob, np.uint8)
        store = np.zeros(int(layout["counts"]["store_bytes"]), np.uint8) if store is None else \
            np.array(store, np.uint8, copy=True).reshape(-1)
        c = N.FamilyMoveCounts()
        self._check(self.L.sdcas_family_pack(self.ctx, _ptr(ops[0]), _ptr(ops[1]), _ptr(ops[2]), _ptr(ops[4]),
                                             _ptr(ops[6]), _ptr(off), k, _ptr(at), _ptr(base), _ptr(ln), at.size,
                                             _ptr(blob), blob.size, _ptr(store), store.size, ctypes.byref(c)),
                    "sdcas_family_pack")
        if counts is not None:
            counts.update(c.as_dict())
        return store

    def family_restore(self, recipes, layout, store, row_at, row_len, row_base=None, blob_bytes=None, blob=None,
                       counts=None):
        """sdcas_family_restore over host arrays: every op with a store offset
        written into its row's window. The blob is `blob` (copied; the bytes no
        op covers stay) or blob_bytes zeros (None: up to the last window's
        end). -> the blob, uint8."""
        ops, k = self._store_ops(recipes, "family_restore")
        off = _arr(layout["op_store_off"], np.uint64)
        if off.size != k:
            raise ValueError(f"family_restore: {k} ops, {off.size} store offsets")
        at, base, ln = self._store_rows(row_at, row_len, row_base, "family_restore")
        store = _arr(store, np.uint8).reshape(-1)
        if blob is not None:
            blob = np.array(blob, np.uint8, copy=True).reshape(-1)
        else:
            if blob_bytes is None:
                blob_bytes = int((at[ln != 0] + ln[ln != 0]).max()) if (ln != 0).any() else 0
            blob = np.zeros(int(blob_bytes), np.uint8)
        c = N.FamilyMoveCounts()
        self._check(self.L.sdcas_family_restore(self.ctx, _ptr(ops[2]), _ptr(ops[4]), _ptr(ops[6]), _ptr(off), k,
                                                _ptr(at), _ptr(base), _ptr(ln), at.size, _ptr(store), store.size,
                                                _ptr(blob), blob.size, ctypes.byref(c)), "sdcas_family_restore")
        if counts is not None:
            counts.update(c.as_dict())
        return blob

    def store_files(self, paths, k=4, max_holders=64, num=1, den=2, params=None, window_bytes=256 << 20):
        """The family store of these files -> FamilyStore (spacedrive_amd/store.py):
        similar_recipes, the layout, the store allocated on the device
        (SdcasError SDCAS_E_CAPACITY when store_bytes does not fit there), the
        files read again window by window (plan_windows) and packed, the store
        brought down, and the files' checksums (file_checksums) to verify
        against. The files are read three times in all; rows are the paths in
        order."""
        from .store import FamilyStore
        return FamilyStore.of_files(self, paths, k=k, max_holders=max_holders, num=num, den=den, params=params,
                                    window_bytes=window_bytes)

    # -- family store: forget rows (keep on the chunk arrays, moves from the old store to the new)
    @staticmethod
    def family_forget_plan(m, n_files):
        """sdcas_family_forget_plan (no GPU) -> workspace_bytes: what keep and
        moves share for m chunks of n_files rows; SdcasError beyond the ranges"""
        ws = ctypes.c_uint64(0)
        rc = N.load().sdcas_family_forget_plan(int(m), int(n_files), ctypes.byref(ws))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, f"family_forget_plan({m}, {n_files})")
        return int(ws.value)

    def family_chunks_keep(self, chunk_file, chunk_off, chunk_len, rep, family, keep):
        """sdcas_family_chunks_keep over host arrays -> recipes.keep_chunks'
        dict: "row_new" uint32[n], "row_from" uint32[n'], "family" int64[n'],
        "chunk_from", "chunk_file" uint32[m'], "chunk_off", "chunk_len"
        uint64[m'], "rep" int64[m'], "counts": sdcas_family_keep_counts' six
        fields"""
        fl, off = _arr(chunk_file, np.uint32), _arr(chunk_off, np.uint64)
        ln, rp = _arr(chunk_len, np.uint64), _arr(rep, np.int64)
        fam = _arr(family, np.int64)
        kp = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, np.uint8)
        m, n = fl.size, fam.size
        if off.size != m or ln.size != m or rp.size != m:
            raise ValueError(f"family_chunks_keep: {m} chunk files, {off.size} offsets, {ln.size} lengths, "
                             f"{rp.size} reps")
        if kp.size != n:
            raise ValueError(f"family_chunks_keep: {n} labels, {kp.size} keep flags")
        row_new, row_from, out_family = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int64)
        c_from, c_file = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        c_off, c_len, c_rep = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.int64)
        counts = N.FamilyKeepCounts()
        self._check(self.L.sdcas_family_chunks_keep(self.ctx, _ptr(fl), _ptr(off), _ptr(ln), _ptr(rp), m, _ptr(fam),
                                                    _ptr(kp), n, _ptr(row_new), _ptr(row_from), _ptr(out_family),
                                                    _ptr(c_from), _ptr(c_file), _ptr(c_off), _ptr(c_len), _ptr(c_rep),
                                                    ctypes.byref(counts)), "sdcas_family_chunks_keep")
        n2, m2 = int(counts.rows_kept), int(counts.chunks_kept)
        return {"row_new": row_new, "row_from": row_from[:n2].copy(), "family": out_family[:n2].copy(),
                "chunk_from": c_from[:m2].copy(), "chunk_file": c_file[:m2].copy(), "chunk_off": c_off[:m2].copy(),
                "chunk_len": c_len[:m2].copy(), "rep": c_rep[:m2].copy(), "counts": counts.as_dict()}

    def family_store_moves(self, old_recipes, old_layout, new_recipes, new_layout, chunk_from, chunk_len):
        """sdcas_family_store_moves over host arrays, with recipes.store_moves'
        arguments -> its dict: "move_dst", "move_src", "move_len" uint64[moves],
        "counts": sdcas_family_moves_counts' six fields"""
        coff, cop = _arr(old_recipes["chunk_off"], np.uint64), _arr(old_recipes["chunk_op"], np.uint32)
        odst, ooff = _arr(old_recipes["op_dst_off"], np.uint64), _arr(old_layout["op_store_off"], np.uint64)
        nfrom, nlen = _arr(chunk_from, np.uint32), _arr(chunk_len, np.uint64)
        noff, nop = _arr(new_recipes["chunk_off"], np.uint64), _arr(new_recipes["chunk_op"], np.uint32)
        noc, nosc = _arr(new_recipes["op_chunk"], np.uint32), _arr(new_recipes["op_src_chunk"], np.uint32)
        ndst, nso = _arr(new_recipes["op_dst_off"], np.uint64), _arr(new_layout["op_store_off"], np.uint64)
        m, k, m2, k2 = coff.size, odst.size, nfrom.size, noc.size
        if cop.size != m or ooff.size != k:
            raise ValueError("family_store_moves: the old layout is of other recipes")
        if nlen.size != m2 or noff.size != m2 or nop.size != m2 or nosc.size != k2 or ndst.size != k2 or \
                nso.size != k2:
            raise ValueError("family_store_moves: the new arrays differ in length")
        dst, src, ln = np.zeros(m2, np.uint64), np.zeros(m2, np.uint64), np.zeros(m2, np.uint64)
        counts = N.FamilyMovesCounts()
        self._check(self.L.sdcas_family_store_moves(self.ctx, _ptr(coff), _ptr(cop), m, _ptr(odst), _ptr(ooff), k,
                                                    _ptr(nfrom), _ptr(noff), _ptr(nlen), _ptr(nop), m2, _ptr(noc),
                                                    _ptr(nosc), _ptr(ndst), _ptr(nso), k2, _ptr(dst), _ptr(src),
                                                    _ptr(ln), ctypes.byref(counts)), "sdcas_family_store_moves")
        j = int(counts.moves)
        return {"move_dst": dst[:j].copy(), "move_src": src[:j].copy(), "move_len": ln[:j].copy(),
                "counts": counts.as_dict()}

    # -- device-resident (pointers are ints: device addresses, e.g. tensor.data_ptr())
    def dev_family_chunks_keep(self, chunk_file, chunk_off, chunk_len, rep, m, family, keep, n_files, row_new=0,
                               row_from=0, family_out=0, chunk_from=0, chunk_file_out=0, chunk_off_out=0,
                               chunk_len_out=0, rep_out=0, counts=0, stream=0):
        """family_chunks_keep over device arrays (sdcas_dev_family_chunks_keep):
        keep uint8[n_files]; the row outputs hold n_files entries and the chunk
        outputs m, counts six uint64; any output may be 0. The outputs are
        dev_family_recipes' inputs as they are, with counts + 2 words the new
        number of chunks"""
        self._check(self.L.sdcas_dev_family_chunks_keep(self.ctx, chunk_file or None, chunk_off or None,
                                                        chunk_len or None, rep or None, int(m), family or None,
                                                        keep or None, int(n_files), row_new or None, row_from or None,
                                                        family_out or None, chunk_from or None, chunk_file_out or None,
                                                        chunk_off_out or None, chunk_len_out or None, rep_out or None,
                                                        counts or None, stream or None), "dev_family_chunks_keep")

    def dev_family_store_moves(self, chunk_off, chunk_op, m, op_dst_off, op_store_off, ops, max_ops, new_chunk_from,
                               new_chunk_off, new_chunk_len, new_chunk_op, new_chunks, max_chunks, new_op_chunk,
                               new_op_src_chunk, new_op_dst_off, new_op_store_off, new_ops, max_new_ops, move_dst=0,
                               move_src=0, move_len=0, counts=0, stream=0):
        """family_store_moves over device arrays (sdcas_dev_family_store_moves):
        ops, new_chunks and new_ops are device uint64 (the old recipes' counts +
        2 words, keep's counts + 2, the new recipes' counts + 2); the move arrays
        hold max_chunks entries, counts six uint64, whose first word is the
        number of moves: dev_family_restore's `ops` when the moves are carried"""
        self._check(self.L.sdcas_dev_family_store_moves(self.ctx, chunk_off or None, chunk_op or None, int(m),
                                                        op_dst_off or None, op_store_off or None, ops or None,
                                                        int(max_ops), new_chunk_from or None, new_chunk_off or None,
                                                        new_chunk_len or None, new_chunk_op or None,
                                                        new_chunks or None, int(max_chunks), new_op_chunk or None,
                                                        new_op_src_chunk or None, new_op_dst_off or None,
                                                        new_op_store_off or None, new_ops or None, int(max_new_ops),
                                                        move_dst or None, move_src or None, move_len or None,
                                                        counts or None, stream or None), "dev_family_store_moves")

    def dev_chunk_index_match(self, idx_keys, idx_digests, idx_values, idx_dir, n, bits, keys, digests, valid, m,
                              pos=0, value=0, counts=0, stream=0):
        """chunk_index_match over device arrays (sdcas_dev_chunk_index_match);
        idx_values, valid and any output may be 0; counts four uint64; nothing
        waits for the device and no workspace is used"""
        self._check(self.L.sdcas_dev_chunk_index_match(self.ctx, idx_keys or None, idx_digests or None,
                                                       idx_values or None, idx_dir or None, int(n), int(bits),
                                                       keys or None, digests or None, valid or None, int(m),
                                                       pos or None, value or None, counts or None, stream or None),
                    "dev_chunk_index_match")

    def dev_chunk_index_add(self, old_keys, old_digests, old_values, old_dir, n_old, bits_old, keys, digests, values,
                            valid, m, new_keys, new_digests, new_values, new_dir, bits_new, pos=0, flags=0, counts=0,
                            stream=0):
        """chunk_index_add over device arrays (sdcas_dev_chunk_index_add): the
        new arrays hold n_old + m entries (the directory 2^bits_new + 1) and
        must not overlap the old ones; counts six uint64, entries_new among
        them; nothing waits for the device once the workspace for m exists"""
        self._check(self.L.sdcas_dev_chunk_index_add(self.ctx, old_keys or None, old_digests or None,
                                                     old_values or None, old_dir or None, int(n_old), int(bits_old),
                                                     keys or None, digests or None, values or None, valid or None,
                                                     int(m), new_keys or None, new_digests or None,
                                                     new_values or None, new_dir or None, int(bits_new), pos or None,
                                                     flags or None, counts or None, stream or None),
                    "dev_chunk_index_add")

    def dev_chunk_holders_match(self, idx_keys, idx_digests, idx_values, idx_dir, n, bits, keys, digests, valid, m,
                                pos=0, value=0, holders=0, counts=0, stream=0):
        """chunk_holders_match over device arrays (sdcas_dev_chunk_holders_match);
        idx_values, valid and any output may be 0; holders uint32[m], counts
        four uint64; nothing waits for the device and no workspace is used"""
        self._check(self.L.sdcas_dev_chunk_holders_match(self.ctx, idx_keys or None, idx_digests or None,
                                                         idx_values or None, idx_dir or None, int(n), int(bits),
                                                         keys or None, digests or None, valid or None, int(m),
                                                         pos or None, value or None, holders or None, counts or None,
                                                         stream or None), "dev_chunk_holders_match")

    def dev_chunk_holders_add(self, old_keys, old_digests, old_values, old_dir, n_old, bits_old, keys, digests, values,
                              valid, m, new_keys, new_digests, new_values, new_dir, bits_new, pos=0, flags=0,
                              counts=0, stream=0):
        """chunk_holders_add over device arrays (sdcas_dev_chunk_holders_add),
        with dev_chunk_index_add's arguments and rules"""
        self._check(self.L.sdcas_dev_chunk_holders_add(self.ctx, old_keys or None, old_digests or None,
                                                       old_values or None, old_dir or None, int(n_old), int(bits_old),
                                                       keys or None, digests or None, values or None, valid or None,
                                                       int(m), new_keys or None, new_digests or None,
                                                       new_values or None, new_dir or None, int(bits_new),
                                                       pos or None, flags or None, counts or None, stream or None),
                    "dev_chunk_holders_add")

    def dev_chunk_holders_remove(self, old_keys, old_digests, old_values, old_dir, n_old, bits_old, removed, r,
                                 new_keys, new_digests, new_values, new_dir, bits_new, counts=0, stream=0):
        """chunk_holders_remove over device arrays (sdcas_dev_chunk_holders_remove):
        the new arrays hold n_old entries (the directory 2^bits_new + 1) and
        must overlap neither the old ones nor `removed` (uint64[r], strictly
        ascending); counts four uint64, entries_new among them; nothing waits
        for the device once the workspace for n_old exists"""
        self._check(self.L.sdcas_dev_chunk_holders_remove(self.ctx, old_keys or None, old_digests or None,
                                                          old_values or None, old_dir or None, int(n_old),
                                                          int(bits_old), removed or None, int(r), new_keys or None,
                                                          new_digests or None, new_values or None, new_dir or None,
                                                          int(bits_new), counts or None, stream or None),
                    "dev_chunk_holders_remove")

    def dev_chunk_peers(self, idx_keys, idx_digests, idx_values, idx_dir, n, bits, keys, digests, valid, chunk_file,
                        chunk_len, m, file_ids, n_files, k, max_holders, mode, max_pairs, peer_count=0, peers=0,
                        peer_bytes=0, shared_bytes=0, unique_bytes=0, common_bytes=0, counts=0, stream=0):
        """chunk_peers over device arrays (sdcas_dev_chunk_peers); idx_values,
        valid and any output may be 0; chunk_file uint32[m], peer_count
        uint32[n_files], peers and peer_bytes uint64[n_files * k], counts seven
        uint64. max_pairs is taken as given: beyond it the counts' overflow is
        1 and the peer rows are zero. Nothing waits for the device once the
        workspace for (m, max_pairs) exists"""
        self._check(self.L.sdcas_dev_chunk_peers(self.ctx, idx_keys or None, idx_digests or None, idx_values or None,
                                                 idx_dir or None, int(n), int(bits), keys or None, digests or None,
                                                 valid or None, chunk_file or None, chunk_len or None, int(m),
                                                 file_ids or None, int(n_files), int(k), int(max_holders),
                                                 self._peers_mode(mode), int(max_pairs), peer_count or None,
                                                 peers or None, peer_bytes or None, shared_bytes or None,
                                                 unique_bytes or None, common_bytes or None, counts or None,
                                                 stream or None), "dev_chunk_peers")

    def dev_file_families(self, ids, sizes, peer_count, peers, peer_bytes, n, k, num=1, den=2, family=0, family_size=0,
                          counts=0, stream=0):
        """file_families over device arrays (sdcas_dev_file_families), e.g.
        dev_chunk_peers' peer_count / peers / peer_bytes as they are; family
        int64[n] (a rep for dev_duplicate_sets), family_size uint32[n], counts
        ten uint64; any output may be 0. ids that are not strictly ascending
        give the trivial rows and the counts' unsorted = 1. Nothing waits for
        the device once the workspace for n exists"""
        self._check(self.L.sdcas_dev_file_families(self.ctx, ids or None, sizes or None, peer_count or None,
                                                   peers or None, peer_bytes or None, int(n), int(k), int(num),
                                                   int(den), family or None, family_size or None, counts or None,
                                                   stream or None), "dev_file_families")

    def dev_family_bytes(self, chunk_file, chunk_len, rep, m, family, n_files, file_bytes=0, delta_bytes=0,
                         self_bytes=0, inherited_bytes=0, set_rep=0, set_files=0, set_total=0, set_stored=0,
                         counts=0, stream=0):
        """family_bytes over device arrays (sdcas_dev_family_bytes), e.g.
        dev_chunk's chunk_file / chunk_len, dev_confirm_duplicates' rep and
        dev_file_families' family as they are; the four per-row outputs
        uint64[n_files], set_rep int64, set_files uint32, set_total and
        set_stored uint64 of n_files // 2 entries each (the first `sets` are
        written), counts nine uint64; any output may be 0. Nothing waits for
        the device once the workspace for (m, n_files) exists"""
        self._check(self.L.sdcas_dev_family_bytes(self.ctx, chunk_file or None, chunk_len or None, rep or None,
                                                  int(m), family or None, int(n_files), file_bytes or None,
                                                  delta_bytes or None, self_bytes or None, inherited_bytes or None,
                                                  set_rep or None, set_files or None, set_total or None,
                                                  set_stored or None, counts or None, stream or None),
                    "dev_family_bytes")

    def dev_family_recipes(self, chunk_file, chunk_off, chunk_len, rep, m, family, n_files, op_chunk=0, op_src_chunk=0,
                           op_row=0, op_src_row=0, op_dst_off=0, op_src_off=0, op_len=0, chunk_op=0, row_ops=0,
                           row_first_op=0, counts=0, stream=0):
        """family_recipes over device arrays (sdcas_dev_family_recipes), e.g.
        dev_chunk's chunk_file / chunk_off / chunk_len, dev_confirm_duplicates'
        rep and dev_file_families' family as they are; the four uint32 and
        three uint64 op arrays of m entries each (the first `ops` are written),
        chunk_op uint32[m], row_ops and row_first_op uint32[n_files], counts
        eight uint64; any output may be 0. Nothing waits for the device once
        the workspace for (m, n_files) exists"""
        self._check(self.L.sdcas_dev_family_recipes(self.ctx, chunk_file or None, chunk_off or None, chunk_len or None,
                                                    rep or None, int(m), family or None, int(n_files),
                                                    op_chunk or None, op_src_chunk or None, op_row or None,
                                                    op_src_row or None, op_dst_off or None, op_src_off or None,
                                                    op_len or None, chunk_op or None, row_ops or None,
                                                    row_first_op or None, counts or None, stream or None),
                    "dev_family_recipes")

    def dev_family_store_layout(self, op_chunk, op_src_chunk, op_row, op_src_row, op_dst_off, op_src_off, op_len,
                                chunk_op, m, ops, max_ops, op_store_off=0, counts=0, stream=0):
        """family_store_layout over dev_family_recipes' outputs as they are
        (sdcas_dev_family_store_layout): ops is a device uint64, the recipes'
        counts + 2 words; op_store_off uint64[max_ops], counts six uint64.
        Nothing waits for the device once the workspace for max_ops exists"""
        self._check(self.L.sdcas_dev_family_store_layout(self.ctx, op_chunk or None, op_src_chunk or None,
                                                         op_row or None, op_src_row or None, op_dst_off or None,
                                                         op_src_off or None, op_len or None, chunk_op or None, int(m),
                                                         ops or None, int(max_ops), op_store_off or None,
                                                         counts or None, stream or None), "dev_family_store_layout")

    def dev_family_pack(self, op_chunk, op_src_chunk, op_row, op_dst_off, op_len, op_store_off, ops, max_ops, row_at,
                        row_base, row_len, n_files, blob, blob_bytes, store, store_capacity, counts=0, stream=0):
        """family_pack over device arrays (sdcas_dev_family_pack): blob and store
        16-byte aligned and readable to the next multiple of 16; row_base may
        be 0; counts four uint64"""
        self._check(self.L.sdcas_dev_family_pack(self.ctx, op_chunk or None, op_src_chunk or None, op_row or None,
                                                 op_dst_off or None, op_len or None, op_store_off or None,
                                                 ops or None, int(max_ops), row_at or None, row_base or None,
                                                 row_len or None, int(n_files), blob or None, int(blob_bytes),
                                                 store or None, int(store_capacity), counts or None, stream or None),
                    "dev_family_pack")

    def dev_family_restore(self, op_row, op_dst_off, op_len, op_store_off, ops, max_ops, row_at, row_base, row_len,
                           n_files, store, store_bytes, blob, blob_bytes, counts=0, stream=0):
        """family_restore over device arrays (sdcas_dev_family_restore), under
        dev_family_pack's contract"""
        self._check(self.L.sdcas_dev_family_restore(self.ctx, op_row or None, op_dst_off or None, op_len or None,
                                                    op_store_off or None, ops or None, int(max_ops), row_at or None,
                                                    row_base or None, row_len or None, int(n_files), store or None,
                                                    int(store_bytes), blob or None, int(blob_bytes), counts or None,
                                                    stream or None), "dev_family_restore")

    def dev_chunk_windows(self, blob, offs, lens, final, n, max_chunks, max_slots, params=None, file_chunks=0,
                          chunk_off=0, chunk_len=0, chunk_file=0, keys=0, digests=0, consumed=0, counts=0, stream=0):
        """chunk_windows over device arrays (sdcas_dev_chunk_windows):
        dev_chunk's contracts; final uint8[n] or 0 (all final), consumed
        uint64[n] or 0. Waits for the device once when keys or digests are
        asked for, never otherwise"""
        cp = self._chunk_params(params)
        self._check(self.L.sdcas_dev_chunk_windows(self.ctx, blob or None, offs or None, lens or None, final or None,
                                                   int(n), ctypes.byref(cp), int(max_chunks), int(max_slots),
                                                   file_chunks or None, chunk_off or None, chunk_len or None,
                                                   chunk_file or None, keys or None, digests or None,
                                                   consumed or None, counts or None, stream or None),
                    "dev_chunk_windows")

    def dev_chunk(self, blob, offs, lens, n, max_chunks, max_slots, params=None, file_chunks=0, chunk_off=0,
                  chunk_len=0, chunk_file=0, keys=0, digests=0, counts=0, stream=0):
        """chunk_messages over device arrays (sdcas_dev_chunk): the blob and
        every offset 16-byte aligned, the blob readable 64 B past every file's
        end; max_chunks / max_slots: chunk_plan's of the lengths; any output
        may be 0; counts six uint64. Waits for the device once when keys or
        digests are asked for, never otherwise"""
        cp = self._chunk_params(params)
        self._check(self.L.sdcas_dev_chunk(self.ctx, blob or None, offs or None, lens or None, int(n),
                                           ctypes.byref(cp), int(max_chunks), int(max_slots), file_chunks or None,
                                           chunk_off or None, chunk_len or None, chunk_file or None, keys or None,
                                           digests or None, counts or None, stream or None), "dev_chunk")

    def dev_chunk_sharing(self, chunk_file, chunk_len, rep, m, n_files, new_bytes=0, self_bytes=0, other_bytes=0,
                          peer=0, peer_bytes=0, counts=0, stream=0):
        """chunk_sharing over device arrays (sdcas_dev_chunk_sharing), e.g.
        dev_chunk's chunk_file / chunk_len and dev_confirm_duplicates' rep as
        they are; any output may be 0; counts six uint64; nothing waits for
        the device"""
        self._check(self.L.sdcas_dev_chunk_sharing(self.ctx, chunk_file or None, chunk_len or None, rep or None,
                                                   int(m), int(n_files), new_bytes or None, self_bytes or None,
                                                   other_bytes or None, peer or None, peer_bytes or None,
                                                   counts or None, stream or None), "dev_chunk_sharing")

    def dev_tree_digests(self, parent, is_dir, name32, sizes, n, keys=0, digests=0, valid=0, tree_bytes=0,
                         tree_files=0, flags=0, counts=0, stream=0):
        """tree_digests over device arrays (sdcas_dev_tree_digests): parent
        (int64) and is_dir (uint8) are HOST numpy arrays, everything else a
        device address; digests / keys / valid are read for the file entries
        and written for the directory entries in place; sizes, keys, valid and
        any output may be 0; counts six uint64"""
        parent, is_dir = _arr(parent, np.int64), _arr(is_dir, np.uint8)
        if parent.size != int(n) or is_dir.size != int(n):
            raise ValueError(f"dev_tree_digests: {n} entries, {parent.size} parents, {is_dir.size} is_dir flags")
        self._check(self.L.sdcas_dev_tree_digests(self.ctx, _ptr(parent), _ptr(is_dir), name32 or None,
                                                  sizes or None, int(n), keys or None, digests or None,
                                                  valid or None, tree_bytes or None, tree_files or None,
                                                  flags or None, counts or None, stream or None),
                    "dev_tree_digests")

    def dev_tree_top(self, parent, rep, n, top_rep=0, flags=0, counts=0, stream=0):
        """tree_top over device arrays (sdcas_dev_tree_top; parent too: a
        parent outside [-1, n) counts as -1); any output may be 0; counts six
        uint64; nothing waits for the device"""
        self._check(self.L.sdcas_dev_tree_top(self.ctx, parent or None, rep or None, int(n), top_rep or None,
                                              flags or None, counts or None, stream or None), "dev_tree_top")

    def dev_reserve(self, max_msgs, max_chunks):
        self._check(self.L.sdcas_dev_reserve(self.ctx, int(max_msgs), int(max_chunks)), "dev_reserve")

    def dev_hash_messages(self, blob, offs, lens, n, out32=0, keys=0, stream=0):
        self._check(self.L.sdcas_dev_hash_messages(self.ctx, blob, offs, lens, int(n), out32 or None,
                                                   keys or None, stream or None), "dev_hash_messages")

    def dev_identify(self, blob, offs, lens, n, keys=0, out32=0, has_key=0, stream=0):
        """cas keys and content digests of n content-resident files from one
        pass over their bytes (sdcas_dev_identify); any output may be 0"""
        self._check(self.L.sdcas_dev_identify(self.ctx, blob, offs, lens, int(n), keys or None, out32 or None,
                                              has_key or None, stream or None), "dev_identify")

    def dev_confirm_duplicates(self, keys, digests, valid, n, rep=0, key_rep=0, flags=0, counts=0, stream=0):
        """confirm_duplicates over device arrays (sdcas_dev_confirm_duplicates),
        e.g. dev_identify's keys / out32 / has_key as they are; valid and any
        output may be 0; counts: six uint64"""
        self._check(self.L.sdcas_dev_confirm_duplicates(self.ctx, keys or None, digests or None, valid or None,
                                                        int(n), rep or None, key_rep or None, flags or None,
                                                        counts or None, stream or None), "dev_confirm_duplicates")

    def dev_duplicate_sets(self, rep, sizes, n, set_rep=0, set_offsets=0, set_bytes=0, members=0, counts=0, order=0,
                           stream=0):
        """duplicate_sets over device arrays (sdcas_dev_duplicate_sets), e.g.
        dev_confirm_duplicates' rep as it is; sizes and any output may be 0;
        set_rep / set_bytes hold n // 2 entries, set_offsets n // 2 + 1,
        members n, counts six uint64; nothing waits for the device"""
        self._check(self.L.sdcas_dev_duplicate_sets(self.ctx, rep or None, sizes or None, int(n), int(order),
                                                    set_rep or None, set_offsets or None, set_bytes or None,
                                                    members or None, counts or None, stream or None),
                    "dev_duplicate_sets")

    def dev_sync(self, stream=0):
        self._check(self.L.sdcas_dev_sync(self.ctx, stream or None), "dev_sync")

    def dev_bind_stream(self, stream, token=None):
        """name `stream`'s identity (sdcas_dev_bind_stream): consecutive
        device calls on it skip the scratch fence's event wait. token None:
        a fresh one (never reused in this process); 0: unbind"""
        if token is None:
            token = next(_STREAM_TOKENS)
        self._check(self.L.sdcas_dev_bind_stream(self.ctx, stream or None, int(token)), "dev_bind_stream")
        return token

    def dev_synth_cas_messages(self, keys, sizes, offs, n, blob, stream=0):
        self._check(self.L.sdcas_dev_synth_cas_messages(self.ctx, keys, sizes, offs, int(n), blob,
                                                        stream or None), "synth")

    def dev_synth_content(self, keys, starts, lens, offs, n, blob, stream=0):
        self._check(self.L.sdcas_dev_synth_content(self.ctx, keys, starts, lens, offs, int(n), blob,
                                                   stream or None), "synth")

    def dev_dedup(self, keys, has_key, status, n, chunk_size, out_link, counts, stream=0):
        self._check(self.L.sdcas_dev_dedup(self.ctx, keys, has_key, status or None, int(n), chunk_size,
                                           out_link, counts or None, stream or None), "dev_dedup")

    def dev_stream_begin(self, lens):
        """device-resident big-message session (sdcas_dev_stream_*): lens > 1 MiB each"""
        lens = _arr(lens, np.uint64)
        self._check(self.L.sdcas_dev_stream_begin(self.ctx, _ptr(lens), lens.size), "dev_stream_begin")

    def dev_stream_update(self, files, msg_offs, lens, dev_addrs, stream=0):
        f, o, l, a = (_arr(x, np.uint64) for x in (files, msg_offs, lens, dev_addrs))
        self._check(self.L.sdcas_dev_stream_update(self.ctx, f.size, _ptr(f), _ptr(o), _ptr(l), _ptr(a),
                                                   stream or None), "dev_stream_update")

    def dev_stream_node_bytes(self):
        return int(self.L.sdcas_dev_stream_node_bytes(self.ctx))

    def dev_stream_export(self, dst, nbytes, stream=0):
        self._check(self.L.sdcas_dev_stream_export(self.ctx, dst, int(nbytes), stream or None), "dev_stream_export")

    def dev_stream_import(self, src, nbytes, stream=0):
        self._check(self.L.sdcas_dev_stream_import(self.ctx, src, int(nbytes), stream or None), "dev_stream_import")

    def dev_stream_finish(self, out32, stream=0):
        self._check(self.L.sdcas_dev_stream_finish(self.ctx, out32, stream or None), "dev_stream_finish")

    def dev_profile(self, enable=True):
        self._check(self.L.sdcas_dev_profile(self.ctx, 1 if enable else 0), "dev_profile")

    def dev_set_leaf_variant(self, v):
        """tuning knob: leaf/tree kernel variant (-1 = default); False (and the
        selection unchanged) for a variant this build does not hold"""
        return self.L.sdcas_dev_set_leaf_variant(self.ctx, int(v)) == N.SDCAS_OK

    def dev_set_piece_variant(self, v):
        """tuning knob: 1 MiB-piece kernel variant of the checksum path (-1 = default)"""
        return self.L.sdcas_dev_set_piece_variant(self.ctx, int(v)) == N.SDCAS_OK

    def dev_set_sort(self, enable):
        """tuning knob: length-sorted slot order (default on); results identical"""
        self._check(self.L.sdcas_dev_set_sort(self.ctx, 1 if enable else 0), "dev_set_sort")

    def dev_kernel_ms(self):
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        self._check(self.L.sdcas_dev_last_kernel_ms(self.ctx, ctypes.byref(a), ctypes.byref(b)), "ms")
        return a.value, b.value


_default = None


class ChunkIndex:
    """A chunk index (include/sdcas.h) kept on the device: the (key, digest)
    pairs of the chunks stored so far, sorted, each with the id of the file
    that held it first. `match` costs what the batch costs, not what the index
    holds; `add` merges the batch's unseen pairs in one pass over the index.

    The four arrays are torch tensors on the engine's GPU (keys and values as
    int64 bit patterns of the uint64 words, the directory as int32); every
    device call runs on the index's own stream, and a tensor handed to the
    `_dev` forms must have been made under ``torch.cuda.stream(index.stream)``.
    """

    def __init__(self, engine, device=None):
        import torch
        self.engine = engine
        self.device = torch.device(device if device is not None else f"cuda:{engine.device_ordinal}")
        self.stream = torch.cuda.Stream(self.device)
        self.n, self.bits = 0, 0
        with torch.cuda.stream(self.stream):
            self.keys = torch.zeros(0, dtype=torch.int64, device=self.device)
            self.digests = torch.zeros(0, dtype=torch.uint8, device=self.device)
            self.values = torch.zeros(0, dtype=torch.int64, device=self.device)
            self.dir = torch.zeros(2, dtype=torch.int32, device=self.device)

    def _upload(self, a, dtype):
        """a host array's bytes as a device tensor of `dtype` (a numpy dtype of
        the same width: uint64 words travel as int64)"""
        import torch
        a = np.ascontiguousarray(a).reshape(-1)
        return torch.from_numpy(a.view(dtype).copy()).to(self.device)

    def _batch(self, keys, digests, valid, who):
        keys, digests, va = Engine._index_batch(keys, digests, valid, who)
        return (self._upload(keys, np.int64), self._upload(digests, np.uint8),
                None if va is None else self._upload(va, np.uint8))

    # what a subclass names: the kind in `load`'s messages, its check (no GPU)
    # and the engine's device add
    _noun = "chunk index"

    @staticmethod
    def _checker(keys, digests, values, dir, bits):
        return Engine.chunk_index_check(keys, digests, dir, bits)

    def _dev_add(self, *args, **kw):
        return self.engine.dev_chunk_index_add(*args, **kw)

    # -- match ----------------------------------------------------------------------
    def _match_call(self, d_keys, d_digests, d_valid, with_holders):
        """the outputs allocated, the engine's device match for the kind of
        index, the counts read -> (pos, value, holders int32[m] or None, counts)"""
        import torch
        m = d_keys.numel()
        p = lambda t: t.data_ptr() if t is not None and t.numel() else 0
        with torch.cuda.stream(self.stream):
            pos = torch.empty(m, dtype=torch.int64, device=self.device)
            value = torch.empty(m, dtype=torch.int64, device=self.device)
            holders = torch.empty(m, dtype=torch.int32, device=self.device) if with_holders else None
            counts = torch.zeros(4, dtype=torch.int64, device=self.device)
            args = (p(self.keys), p(self.digests), p(self.values), p(self.dir), self.n, self.bits, p(d_keys),
                    p(d_digests), p(d_valid), m, p(pos), p(value))
            if with_holders:
                self.engine.dev_chunk_holders_match(*args, p(holders), counts.data_ptr(), stream=self.stream.cuda_stream)
            else:
                self.engine.dev_chunk_index_match(*args, counts.data_ptr(), stream=self.stream.cuda_stream)
            c = [int(v) for v in counts.cpu()]
        return pos, value, holders, dict(zip((name for name, _ in N.IndexMatchCounts._fields_), c))

    def _match_dev(self, d_keys, d_digests, d_valid):
        """device tensors in, device tensors out: (pos int64[m], value
        int64[m]: the uint64's bits, counts dict — reading them is the wait)"""
        pos, value, _, counts = self._match_call(d_keys, d_digests, d_valid, False)
        return pos, value, counts

    def match(self, keys, digests, valid=None):
        """only the batch goes up -> (pos int64[m], value uint64[m], counts),
        as Engine.chunk_index_match"""
        import torch
        with torch.cuda.stream(self.stream):
            d_keys, d_dig, d_valid = self._batch(keys, digests, valid, "ChunkIndex.match")
            pos, value, counts = self._match_dev(d_keys, d_dig, d_valid)
            return pos.cpu().numpy(), value.cpu().numpy().view(np.uint64), counts

    # -- add ------------------------------------------------------------------------
    def _add_dev(self, d_keys, d_digests, d_values, d_valid):
        """the batch merged in: new arrays of n + m entries, the device add at
        the recommended width for n + m, entries_new read (the one wait), the
        arrays swapped -> (pos int64[m], flags uint8[m] device tensors, counts)"""
        import torch
        m = d_keys.numel()
        p = lambda t: t.data_ptr() if t is not None and t.numel() else 0
        bits_new = self.engine.chunk_index_dir_bits(self.n + m)
        with torch.cuda.stream(self.stream):
            if m == 0:  # nothing to merge: the index stays as it is
                return (torch.empty(0, dtype=torch.int64, device=self.device),
                        torch.empty(0, dtype=torch.uint8, device=self.device),
                        dict(zip((name for name, _ in N.IndexAddCounts._fields_), (0, 0, 0, 0, self.n, self.n))))
            cap = self.n + m
            keys = torch.empty(cap, dtype=torch.int64, device=self.device)
            digests = torch.empty(32 * cap, dtype=torch.uint8, device=self.device)
            values = torch.empty(cap, dtype=torch.int64, device=self.device)
            dir = torch.empty((1 << bits_new) + 1, dtype=torch.int32, device=self.device)
            pos = torch.empty(m, dtype=torch.int64, device=self.device)
            flags = torch.empty(m, dtype=torch.uint8, device=self.device)
            counts = torch.zeros(6, dtype=torch.int64, device=self.device)
            self._dev_add(p(self.keys), p(self.digests), p(self.values), p(self.dir), self.n, self.bits, p(d_keys),
                          p(d_digests), p(d_values), p(d_valid), m, p(keys), p(digests), p(values), dir.data_ptr(),
                          bits_new, p(pos), p(flags), counts.data_ptr(), stream=self.stream.cuda_stream)
            c = [int(v) for v in counts.cpu()]
            n_new = c[5]
            if not self.n <= n_new <= cap:
                raise N.SdcasError(N.SDCAS_E_HIP,
                                   f"{type(self).__name__}.add: {n_new} entries from {self.n} and a batch of {m}")
            self.keys, self.digests, self.values, self.dir = keys[:n_new], digests[:32 * n_new], values[:n_new], dir
            self.n, self.bits = n_new, bits_new
        return pos, flags, dict(zip((name for name, _ in N.IndexAddCounts._fields_), c))

    def add(self, keys, digests, values, valid=None):
        """-> (pos int64[m]: the pair's entry in the index as it is now, flags
        uint8[m], counts), as Engine.chunk_index_add"""
        import torch
        with torch.cuda.stream(self.stream):
            d_keys, d_dig, d_valid = self._batch(keys, digests, valid, "ChunkIndex.add")
            values = _arr(values, np.uint64)
            if values.size != d_keys.numel():
                raise ValueError(f"ChunkIndex.add: {d_keys.numel()} keys, {values.size} values")
            pos, flags, counts = self._add_dev(d_keys, d_dig, self._upload(values, np.int64), d_valid)
            return pos.cpu().numpy(), flags.cpu().numpy(), counts

    # -- host copies ----------------------------------------------------------------
    def arrays(self):
        """-> (keys uint64[n], digests uint8[n, 32], values uint64[n], dir
        uint32[2^bits + 1], bits) on the host: Engine.chunk_index_match's tuple"""
        import torch
        with torch.cuda.stream(self.stream):
            return (self.keys.cpu().numpy().view(np.uint64), self.digests.cpu().numpy().reshape(-1, 32),
                    self.values.cpu().numpy().view(np.uint64), self.dir.cpu().numpy().view(np.uint32), self.bits)

    def save(self, path):
        """the index as one .npz"""
        keys, digests, values, dir, bits = self.arrays()
        with open(path, "wb") as f:
            np.savez(f, keys=keys, digests=digests, values=values, dir=dir, bits=np.uint32(bits))

    @classmethod
    def load(cls, engine, path, device=None):
        """an index saved by `save`: checked (the class's check:
        sdcas_chunk_index_check, for ChunkHolders sdcas_chunk_holders_check)
        before anything goes to the device; ValueError when it is not an index
        of the class's kind"""
        import torch
        import zipfile
        try:  # the archive's own checksums catch a byte that changed on disk
            with np.load(path) as z:
                keys, digests, values, dir, bits = (z["keys"].astype(np.uint64), z["digests"].astype(np.uint8),
                                                    z["values"].astype(np.uint64), z["dir"].astype(np.uint32),
                                                    int(z["bits"]))
        except (zipfile.BadZipFile, KeyError, EOFError, OSError, ValueError) as e:
            raise ValueError(f"{path}: not a saved {cls._noun} ({e})") from e
        n = keys.size
        if digests.size != 32 * n or values.size != n or not 0 <= bits <= N.SDCAS_INDEX_MAX_BITS or \
                dir.size != (1 << bits) + 1:
            raise ValueError(f"{path}: the arrays' sizes do not make an index")
        rc, bad = cls._checker(keys, digests, values, dir, bits)
        if rc != N.SDCAS_OK:
            raise ValueError(f"{path}: not a {cls._noun} (sdcas error {rc}" +
                             (f", first at entry or slot {bad})" if bad is not None else ")"))
        ix = cls(engine, device)
        with torch.cuda.stream(ix.stream):
            ix.keys, ix.digests = ix._upload(keys, np.int64), ix._upload(digests, np.uint8)
            ix.values, ix.dir = ix._upload(values, np.int64), ix._upload(dir, np.int32)
        ix.n, ix.bits = n, bits
        return ix


class ChunkHolders(ChunkIndex):
    """A holders index (include/sdcas.h) kept on the device: a ChunkIndex that
    stores EVERY file that holds a pair, one entry per (key, digest, file id),
    sorted by that triple, and so can forget files again. `match` gives a
    pair's lowest holder and the number of its holders; `add` merges the
    batch's unseen triples; `remove(file_ids)` streams the index through once
    and leaves, byte for byte, the index built from the files that remain;
    `peers` reads the holders between a run's two ends: per batch file, the k
    files that hold most of its bytes.

    The tensors, the stream, `load` and the `_upload` / `_match_dev` /
    `_add_dev` contract are ChunkIndex's (here `_add_dev` merges the batch's
    unseen (key, digest, value) triples), so Engine.similar_files_indexed takes
    either kind; with this one the origin of a stored chunk is its lowest
    holder."""

    _noun = "holders index"
    _checker = staticmethod(Engine.chunk_holders_check)

    def _dev_add(self, *args, **kw):
        return self.engine.dev_chunk_holders_add(*args, **kw)

    # -- match ----------------------------------------------------------------------
    def _match_holders_dev(self, d_keys, d_digests, d_valid):
        """device tensors in, device tensors out: (pos int64[m], value
        int64[m]: the uint64's bits, holders int32[m], counts dict — reading
        them is the wait)"""
        return self._match_call(d_keys, d_digests, d_valid, True)

    def _match_dev(self, d_keys, d_digests, d_valid):
        """ChunkIndex._match_dev's triple: pos is the pair's first entry, value
        its lowest holder"""
        pos, value, _, counts = self._match_holders_dev(d_keys, d_digests, d_valid)
        return pos, value, counts

    def match(self, keys, digests, valid=None):
        """only the batch goes up -> (pos int64[m], value uint64[m], holders
        uint32[m], counts), as Engine.chunk_holders_match"""
        import torch
        with torch.cuda.stream(self.stream):
            d_keys, d_dig, d_valid = self._batch(keys, digests, valid, "ChunkHolders.match")
            pos, value, holders, counts = self._match_holders_dev(d_keys, d_dig, d_valid)
            return (pos.cpu().numpy(), value.cpu().numpy().view(np.uint64), holders.cpu().numpy().view(np.uint32),
                    counts)

    # -- peers ----------------------------------------------------------------------
    def _peers_dev(self, d_keys, d_digests, d_valid, d_file, d_len, d_ids, n_files, k, max_holders, mode,
                   max_pairs=None):
        """device tensors in (d_file int32[m]: the uint32's bits, d_len and
        d_ids int64), the outputs on the host -> Engine.chunk_peers' dict.
        max_pairs None: a first call without outputs and without room counts
        the pairs (its `pairs` is exact whatever the room), the second takes
        exactly that many, so the workspace follows the batch's pairs and not
        m * max_holders; reading the counts is the wait, once per call"""
        import torch
        m, n, k = d_keys.numel(), int(n_files), int(k)
        p = lambda t: t.data_ptr() if t is not None and t.numel() else 0
        with torch.cuda.stream(self.stream):
            counts = torch.zeros(7, dtype=torch.int64, device=self.device)
            args = (p(self.keys), p(self.digests), p(self.values), p(self.dir), self.n, self.bits, p(d_keys),
                    p(d_digests), p(d_valid), p(d_file), p(d_len), m, p(d_ids), n, k, int(max_holders), mode)
            if max_pairs is None:
                self.engine.dev_chunk_peers(*args, 0, counts=counts.data_ptr(), stream=self.stream.cuda_stream)
                max_pairs = int(counts.cpu()[3])
                if max_pairs > N.SDCAS_PEERS_MAX_PAIRS:
                    raise N.SdcasError(N.SDCAS_E_CAPACITY, f"ChunkHolders.peers: {max_pairs} (chunk, holder) pairs")
            cnt = torch.empty(n, dtype=torch.int32, device=self.device)
            peers = torch.empty(n * k, dtype=torch.int64, device=self.device)
            pb = torch.empty(n * k, dtype=torch.int64, device=self.device)
            shared, unique, common = (torch.empty(n, dtype=torch.int64, device=self.device) for _ in range(3))
            self.engine.dev_chunk_peers(*args, max_pairs, p(cnt), p(peers), p(pb), p(shared), p(unique), p(common),
                                        counts.data_ptr(), stream=self.stream.cuda_stream)
            c = dict(zip((name for name, _ in N.PeersCounts._fields_), (int(v) for v in counts.cpu())))
            u64 = lambda t: t.cpu().numpy().view(np.uint64)
            out = {"peer_count": cnt.cpu().numpy().view(np.uint32), "peers": u64(peers).reshape(n, k),
                   "peers_bytes": u64(pb).reshape(n, k), "shared_bytes": u64(shared), "unique_bytes": u64(unique),
                   "common_bytes": u64(common), "counts": c}
        if c["overflow"]:
            raise N.SdcasError(N.SDCAS_E_CAPACITY,
                               f"ChunkHolders.peers: {c['pairs']} (chunk, holder) pairs exceed max_pairs {max_pairs}")
        return out

    def peers(self, keys, digests, chunk_file, chunk_len, file_ids, k=4, max_holders=64, mode="earlier", valid=None,
              max_pairs=None):
        """only the batch goes up; on the index's stream -> Engine.chunk_peers'
        dict: per batch file the k files of the index that hold most of its
        bytes, over EVERY holder of its chunks. file_ids[i] is the id file i
        has (or would have) in the index; mode "earlier" counts the holders
        below it, "all" every holder but itself. The index is not changed."""
        import torch
        fl, ln, ids = _arr(chunk_file, np.uint32), _arr(chunk_len, np.uint64), _arr(file_ids, np.uint64)
        with torch.cuda.stream(self.stream):
            d_keys, d_dig, d_valid = self._batch(keys, digests, valid, "ChunkHolders.peers")
            if fl.size != d_keys.numel() or ln.size != d_keys.numel():
                raise ValueError(f"ChunkHolders.peers: {d_keys.numel()} keys, {fl.size} chunk files, {ln.size} lengths")
            return self._peers_dev(d_keys, d_dig, d_valid, self._upload(fl, np.int32), self._upload(ln, np.int64),
                                   self._upload(ids, np.int64), ids.size, k, max_holders,
                                   Engine._peers_mode(mode), max_pairs)

    # -- remove ---------------------------------------------------------------------
    def remove(self, file_ids, bits_new=None):
        """every entry whose value is one of file_ids taken out (the ids are
        sorted and made distinct here): new arrays of n entries, the directory
        at bits_new (None: the width the index has; a wide directory is legal
        and only costs memory), entries_new read (the one wait), the arrays
        swapped -> counts: dict of sdcas_holders_remove_counts' four fields"""
        import torch
        ids = np.unique(_arr(file_ids, np.uint64).reshape(-1))
        bits_new = self.bits if bits_new is None else int(bits_new)
        if not 0 <= bits_new <= N.SDCAS_INDEX_MAX_BITS:
            raise N.SdcasError(N.SDCAS_E_CAPACITY, f"ChunkHolders.remove: a directory of {bits_new} bits")
        p = lambda t: t.data_ptr() if t is not None and t.numel() else 0
        n = self.n
        with torch.cuda.stream(self.stream):
            d_ids = self._upload(ids, np.int64)
            keys = torch.empty(n, dtype=torch.int64, device=self.device)
            digests = torch.empty(32 * n, dtype=torch.uint8, device=self.device)
            values = torch.empty(n, dtype=torch.int64, device=self.device)
            dir = torch.empty((1 << bits_new) + 1, dtype=torch.int32, device=self.device)
            counts = torch.zeros(4, dtype=torch.int64, device=self.device)
            self.engine.dev_chunk_holders_remove(p(self.keys), p(self.digests), p(self.values), p(self.dir), n,
                                                 self.bits, p(d_ids), ids.size, p(keys), p(digests), p(values),
                                                 dir.data_ptr(), bits_new, counts.data_ptr(),
                                                 stream=self.stream.cuda_stream)
            c = [int(v) for v in counts.cpu()]
            n_new = c[2]
            if not 0 <= n_new <= n:
                raise N.SdcasError(N.SDCAS_E_HIP, f"ChunkHolders.remove: {n_new} entries left of {n}")
            self.keys, self.digests, self.values, self.dir = keys[:n_new], digests[:32 * n_new], values[:n_new], dir
            self.n, self.bits = n_new, bits_new
        return dict(zip((name for name, _ in N.HoldersRemoveCounts._fields_), c))

    # -- other sources ----------------------------------------------------------------
    @classmethod
    def from_index(cls, chunk_index):
        """a ChunkIndex's arrays adopted by device copy: every chunk index is a
        holders index, in which each pair has the one holder that came first"""
        import torch
        ix = cls(chunk_index.engine, chunk_index.device)
        ready = torch.cuda.Event()
        ready.record(chunk_index.stream)
        ix.stream.wait_event(ready)
        with torch.cuda.stream(ix.stream):  # the copies are this index's own; the source may change once they are made
            ix.keys, ix.digests, ix.values, ix.dir = (t.clone() for t in (chunk_index.keys, chunk_index.digests,
                                                                          chunk_index.values, chunk_index.dir))
        ix.stream.synchronize()
        ix.n, ix.bits = chunk_index.n, chunk_index.bits
        return ix


def default_engine() -> Engine:
    global _default
    if _default is None:
        _default = Engine()
    return _default


def generate_cas_id(path, size) -> str:
    """core/src/object/cas.rs:23 — `pub async fn generate_cas_id(path, size) -> Result<String>`"""
    return default_engine().generate_cas_id(path, size)


def file_checksum(path) -> str:
    """core/src/object/validation/hash.rs:11 — `pub async fn file_checksum(path) -> Result<String>`"""
    return default_engine().file_checksum(path)


__all__ = ["Engine", "generate_cas_id", "file_checksum", "key_to_hex", "digest_to_hex", "io_error",
           "default_engine"]


class Node:
    """sdcas_node: one process driving several GPUs (one context per entry of
    `devices`; a device may repeat). The batch calls shard over the contexts
    and the dedup's exchange runs in this process (RCCL between distinct
    devices, device copies otherwise)."""

    def __init__(self, devices=(0,), io_threads: int = 0, staging_bytes: int = 0, direct_io=False, progress=None,
                 cancel=None):
        self.L = N.load()
        self._cb = Engine._progress_fn(progress)
        self._cancel = cancel
        opts = N.Options(-1, io_threads, N.SDCAS_OPT_DIRECT_IO if direct_io else 0, staging_bytes, self._cb,
                         None, ctypes.pointer(cancel) if cancel is not None else None)
        devs = (ctypes.c_int32 * len(devices))(*devices)
        node = ctypes.c_void_p()
        rc = self.L.sdcas_node_init(devs, len(devices), ctypes.byref(opts), ctypes.byref(node))
        if rc != N.SDCAS_OK:
            raise N.SdcasError(rc, "sdcas_node_init failed")
        self.node = node

    @property
    def size(self):
        return int(self.L.sdcas_node_size(self.node))

    @property
    def uses_rccl(self):
        return bool(self.L.sdcas_node_uses_rccl(self.node))

    def close(self):
        if getattr(self, "node", None):
            self.L.sdcas_node_destroy(self.node)
            self.node = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what, partial=None):
        if rc != N.SDCAS_OK:
            msg = self.L.sdcas_node_last_error(self.node).decode(errors="replace")
            if rc == N.SDCAS_E_CANCELLED:
                raise N.Cancelled(f"{what}: {msg}", partial)
            raise N.SdcasError(rc, f"{what}: {msg}")

    def generate_cas_ids(self, paths, sizes):
        n = len(paths)
        buf, parr = _cpaths(paths)
        sizes = _arr(sizes, np.uint64)
        keys = np.zeros(n, np.uint64)
        st = np.zeros(n, np.int32)
        self._check(self.L.sdcas_node_cas_ids(self.node, _ptr(parr), _ptr(sizes), n, _ptr(keys), _ptr(st)),
                    "sdcas_node_cas_ids", (keys, st))
        del buf
        return keys, st

    def file_checksums(self, paths):
        n = len(paths)
        buf, parr = _cpaths(paths)
        out = np.zeros((n, 32), np.uint8)
        st = np.zeros(n, np.int32)
        self._check(self.L.sdcas_node_checksums(self.node, _ptr(parr), n, _ptr(out), _ptr(st)),
                    "sdcas_node_checksums", (out, st))
        del buf
        return out, st

    def identifier_dedup_window(self, keys, has_key, status=None, chunk_size=100, existing_keys=(), max_steps=0,
                                more=False):
        keys = _arr(keys, np.uint64)
        n = keys.size
        has_key = _arr(has_key, np.uint8)
        st = None if status is None else _arr(status, np.int32)
        ex = _arr(existing_keys, np.uint64)
        out = np.zeros(n, np.int64)
        created, linked = ctypes.c_int64(0), ctypes.c_int64(0)
        win = N.JobWindow(int(max_steps), int(bool(more)), 0, 0, 0, 0)
        self._check(self.L.sdcas_node_dedup_window(self.node, _ptr(keys), _ptr(has_key), _ptr(st), n, chunk_size,
                                                   _ptr(ex), ex.size, ctypes.byref(win), _ptr(out),
                                                   ctypes.byref(created), ctypes.byref(linked)),
                    "sdcas_node_dedup_window")
        return out, created.value, linked.value, {"steps": win.steps, "rows": win.rows, "rereads": win.rereads}

    def identifier_dedup(self, keys, has_key, status=None, chunk_size=100, existing_keys=()):
        link, c, l, _ = self.identifier_dedup_window(keys, has_key, status, chunk_size, existing_keys)
        return link, c, l
