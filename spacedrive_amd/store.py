"""The family store (include/sdcas.h, "family store") as an object: the recipes
of a set of files, the layout of their literal bytes, the packed store and
what it takes to prove that every file comes back from it."""
import os
import zipfile

import numpy as np

from . import _native as N
from .recipes import STORE_NONE, store_layout

_OP32 = ("op_chunk", "op_src_chunk", "op_row", "op_src_row")
_OP64 = ("op_dst_off", "op_src_off", "op_len")
_CHUNKS = ("chunk_file", "chunk_len", "rep", "family")  # what `remove` needs besides the recipes' chunk_off
_SLACK = 64   # readable bytes sdcas_dev_hash_messages wants after every message
_ALIGN = 128  # rows start on line boundaries in a window


def _place(n):
    """the room a row of n bytes takes in a window"""
    return (int(n) + _SLACK + _ALIGN - 1) // _ALIGN * _ALIGN


class FamilyStore:
    """recipes: Engine.family_recipes' dict; layout: Engine.family_store_layout's;
    store: uint8[store_bytes], the literal ops' bytes; sizes uint64[n] and
    digests uint8[n, 32]: every row's length and BLAKE3. Rows are numbered as
    the recipes number them. chunks (optional): {"chunk_file" uint32[m],
    "chunk_len" uint64[m], "rep" int64[m], "family" int64[n]}, the recipes'
    inputs, which `remove` needs; a store without them does everything else.
    `restore`, `verify` and `remove` run on the engine's GPU (engine None:
    default_engine()); everything else needs none."""

    def __init__(self, recipes, layout, store, sizes, digests, engine=None, chunks=None):
        self.recipes, self.layout = recipes, layout
        self.chunks = None if chunks is None else {
            "chunk_file": np.ascontiguousarray(chunks["chunk_file"], np.uint32).reshape(-1),
            "chunk_len": np.ascontiguousarray(chunks["chunk_len"], np.uint64).reshape(-1),
            "rep": np.ascontiguousarray(chunks["rep"], np.int64).reshape(-1),
            "family": np.ascontiguousarray(chunks["family"], np.int64).reshape(-1)}
        self.store = np.ascontiguousarray(store, np.uint8).reshape(-1)
        self.sizes = np.ascontiguousarray(sizes, np.uint64).reshape(-1)
        self.digests = np.ascontiguousarray(digests, np.uint8).reshape(-1, 32)
        self.engine = engine
        self._dev = None
        self.check(self.recipes, self.layout, self.store, self.sizes, self.digests, chunks=self.chunks)

    # -- the check a store passes before it is used (no GPU) ---------------------------
    @staticmethod
    def check(recipes, layout, store, sizes, digests, what="FamilyStore", chunks=None):
        """ValueError unless the parts make a store: array lengths, `ops`
        consistent, rows and chunk_op in range, every op inside its row, the
        layout that of the recipes, every offset within the store; with chunk
        arrays, their lengths against chunk_op, chunk_file in range and the
        chunks of every row that takes part adding up to its size"""
        ops = [np.asarray(recipes[k]) for k in _OP32 + _OP64]
        k, n = ops[0].size, np.asarray(sizes).size
        if not all(a.size == k for a in ops):
            raise ValueError(f"{what}: the op arrays differ in length")
        off = np.asarray(layout["op_store_off"])
        if off.size != k:
            raise ValueError(f"{what}: {k} ops, {off.size} store offsets")
        if int(recipes["counts"]["ops"]) != k or int(layout["counts"]["ops"]) != k:
            raise ValueError(f"{what}: the counts name another number of ops than {k}")
        if np.asarray(digests).size != 32 * n:
            raise ValueError(f"{what}: {n} sizes, {np.asarray(digests).size} digest bytes")
        for name in ("row_ops", "row_first_op"):
            if np.asarray(recipes[name]).size != n:
                raise ValueError(f"{what}: {n} sizes, {np.asarray(recipes[name]).size} entries of {name}")
        chunk_op = np.asarray(recipes["chunk_op"], np.uint32)
        if ((chunk_op >= k) & (chunk_op != 0xFFFFFFFF)).any():
            raise ValueError(f"{what}: chunk_op names an op past {k}")
        row, dst, ln = ops[2].astype(np.uint64), ops[4].astype(np.uint64), ops[6].astype(np.uint64)
        if (row >= n).any():
            raise ValueError(f"{what}: an op's row is past {n}")
        if ((dst + ln < dst) | (dst + ln > np.asarray(sizes, np.uint64)[row.astype(np.int64)])).any():
            raise ValueError(f"{what}: an op ends past its row's size")
        want = store_layout(recipes)
        if not np.array_equal(want["op_store_off"], off.astype(np.uint64)) or \
                any(int(layout["counts"][key]) != v for key, v in want["counts"].items()):
            raise ValueError(f"{what}: the layout is not that of the recipes")
        size = np.asarray(store).size
        if int(want["counts"]["store_bytes"]) != size:
            raise ValueError(f"{what}: a store of {size} bytes, the layout names {want['counts']['store_bytes']}")
        has = off.astype(np.uint64) != np.uint64(STORE_NONE)
        o, l = off.astype(np.uint64)[has], ln[has]
        if ((o > size) | (l > np.uint64(size) - np.minimum(o, np.uint64(size)))).any():
            raise ValueError(f"{what}: an op's bytes lie outside the store")
        if chunks is not None:
            fl, cl = np.asarray(chunks["chunk_file"], np.uint32), np.asarray(chunks["chunk_len"], np.uint64)
            fam, m = np.asarray(chunks["family"], np.int64), chunk_op.size
            if fl.size != m or cl.size != m or np.asarray(chunks["rep"]).size != m or \
                    np.asarray(recipes.get("chunk_off", ())).size != m:
                raise ValueError(f"{what}: {m} entries of chunk_op, other numbers of chunk_file, chunk_len, rep or "
                                 f"chunk_off")
            if fam.size != n:
                raise ValueError(f"{what}: {n} sizes, {fam.size} family labels")
            if (fl >= n).any():
                raise ValueError(f"{what}: chunk_file names a row past {n}")
            sums = np.zeros(n, np.uint64)
            np.add.at(sums, fl.astype(np.int64), cl)
            part = (fam >= 0) & (fam < n)
            if (sums[part] != np.asarray(sizes, np.uint64)[part]).any():
                raise ValueError(f"{what}: a row's chunks do not add up to its size")

    # -- across runs ---------------------------------------------------------------------
    def save(self, path):
        """the store as one .npz"""
        r, l = self.recipes, self.layout
        parts = {k: np.asarray(r[k], np.uint32) for k in _OP32 + ("chunk_op", "row_ops", "row_first_op")}
        parts.update({k: np.asarray(r[k], np.uint64) for k in _OP64})
        parts["recipes_counts"] = np.array([r["counts"][name] for name, _ in N.FamilyRecipesCounts._fields_], np.uint64)
        parts["layout_counts"] = np.array([l["counts"][name] for name, _ in N.FamilyStoreCounts._fields_], np.uint64)
        parts["op_store_off"] = np.asarray(l["op_store_off"], np.uint64)
        if self.chunks is not None:  # extra arrays: a reader that does not know them ignores them
            parts.update({"chunks_" + k: self.chunks[k] for k in _CHUNKS})
            parts["chunks_chunk_off"] = np.asarray(r["chunk_off"], np.uint64)
        with open(path, "wb") as f:
            np.savez(f, store=self.store, sizes=self.sizes, digests=self.digests, **parts)

    @classmethod
    def load(cls, path, engine=None):
        """a store saved by `save`, checked (`check`, no GPU) before it is
        used; ValueError when it is not one"""
        try:  # the archive's own checksums catch a byte that changed on disk
            with np.load(path) as z:
                recipes = {k: z[k].astype(np.uint32) for k in _OP32 + ("chunk_op", "row_ops", "row_first_op")}
                recipes.update({k: z[k].astype(np.uint64) for k in _OP64})
                rc, lc = z["recipes_counts"].astype(np.uint64), z["layout_counts"].astype(np.uint64)
                off = z["op_store_off"].astype(np.uint64)
                store, sizes, digests = z["store"].astype(np.uint8), z["sizes"].astype(np.uint64), \
                    z["digests"].astype(np.uint8)
                chunks = None  # a store saved before the chunk arrays were kept has none, and does all but `remove`
                if all("chunks_" + k in z.files for k in _CHUNKS + ("chunk_off",)):
                    chunks = {"chunk_file": z["chunks_chunk_file"].astype(np.uint32),
                              "chunk_len": z["chunks_chunk_len"].astype(np.uint64),
                              "rep": z["chunks_rep"].astype(np.int64), "family": z["chunks_family"].astype(np.int64)}
                    recipes["chunk_off"] = z["chunks_chunk_off"].astype(np.uint64)
        except (zipfile.BadZipFile, KeyError, EOFError, OSError, ValueError) as e:
            raise ValueError(f"{path}: not a saved family store ({e})") from e
        if rc.size != len(N.FamilyRecipesCounts._fields_) or lc.size != len(N.FamilyStoreCounts._fields_):
            raise ValueError(f"{path}: the counts are not a family store's")
        recipes["counts"] = {name: int(v) for (name, _), v in zip(N.FamilyRecipesCounts._fields_, rc)}
        recipes["op_literal"] = recipes["op_chunk"] == recipes["op_src_chunk"]
        layout = {"op_store_off": off, "counts": {name: int(v) for (name, _), v in zip(N.FamilyStoreCounts._fields_, lc)}}
        cls.check(recipes, layout, store, sizes, digests, os.fspath(path), chunks=chunks)
        return cls(recipes, layout, store, sizes, digests, engine, chunks)

    # -- on the device -------------------------------------------------------------------
    def _engine(self):
        if self.engine is None:
            from .engine import default_engine
            self.engine = default_engine()
        return self.engine

    @staticmethod
    def _up(a, device):
        """a host array's bytes on the device (uint64 and uint32 words travel as int64 and int32)"""
        import torch
        a = np.ascontiguousarray(a).reshape(-1)
        view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]
        if a.size == 0:  # a pointer the library may read 16 bytes from
            return torch.zeros(16, dtype=torch.uint8, device=device)
        return torch.from_numpy(a.view(view).copy()).to(device)

    @staticmethod
    def _ops_up(recipes, layout, device):
        """what the mover reads of the ops, on the device -> dict of tensors, and the number of ops under "k" """
        d = {name: FamilyStore._up(np.asarray(recipes[name], np.uint32), device)
             for name in ("op_chunk", "op_src_chunk", "op_row")}
        d.update({name: FamilyStore._up(np.asarray(recipes[name], np.uint64), device)
                  for name in ("op_dst_off", "op_len")})
        d["off"] = FamilyStore._up(np.asarray(layout["op_store_off"], np.uint64), device)
        d["k"] = int(np.asarray(recipes["op_row"]).size)
        d["ops"] = FamilyStore._up(np.array([d["k"]], np.uint64), device)
        return d

    def _device(self):
        """the ops and the store on the engine's GPU, uploaded once"""
        if self._dev is None:
            import torch
            eng = self._engine()
            device = torch.device(f"cuda:{eng.device_ordinal}")
            stream = torch.cuda.Stream(device)
            with torch.cuda.stream(stream):
                d = self._ops_up(self.recipes, self.layout, device)
                pad = -self.store.size % 16  # readable to the next multiple of 16
                d["store"] = self._up(np.concatenate([self.store, np.zeros(pad + 16, np.uint8)]), device)
            d["device"], d["stream"] = device, stream
            self._dev = d
        return self._dev

    def _restore_window(self, at, base, ln, blob_bytes):
        """one device restore of the rows with ln != 0 -> the window, a device
        tensor of blob_bytes (+ slack), zeros where no op writes"""
        import torch
        d, eng = self._device(), self._engine()
        blob = torch.zeros(int(blob_bytes) + _ALIGN, dtype=torch.uint8, device=d["device"])
        d_at, d_base, d_ln = (self._up(a, d["device"]) for a in (at, base, ln))
        eng.dev_family_restore(d["op_row"].data_ptr(), d["op_dst_off"].data_ptr(), d["op_len"].data_ptr(),
                               d["off"].data_ptr(), d["ops"].data_ptr(), d["k"], d_at.data_ptr(), d_base.data_ptr(),
                               d_ln.data_ptr(), self.sizes.size, d["store"].data_ptr(), self.store.size,
                               blob.data_ptr(), int(blob_bytes), stream=d["stream"].cuda_stream)
        return blob

    def _windows(self, rows, window_bytes):
        """the rows in windows: (rows, streamed) with whole rows sharing a
        window while their places fit, a larger row alone"""
        from .engine import Engine
        rows = list(rows)
        plan = Engine.plan_windows([_place(self.sizes[r]) for r in rows], window_bytes)
        return [(rows[first:first + nf], streamed) for first, nf, streamed in plan]

    def _rows(self, rows):
        n = self.sizes.size
        rows = range(n) if rows is None else sorted({int(r) for r in rows})
        if any(not 0 <= r < n for r in rows):
            raise ValueError(f"FamilyStore: a row outside [0, {n})")
        return rows

    def _whole(self, group):
        """a window of whole rows placed -> (at, base, ln, blob_bytes)"""
        n = self.sizes.size
        at, base, ln = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        pos = 0
        for r in group:
            at[r], ln[r] = pos, self.sizes[r]
            pos += _place(self.sizes[r])
        return at, base, ln, pos

    def _pieces(self, r, window_bytes):
        """row r, larger than a window, restored to the host piece by piece through row_base -> bytes"""
        import torch
        n, size = self.sizes.size, int(self.sizes[r])
        step = max(16, int(window_bytes) - _SLACK - _ALIGN) // 16 * 16
        out = bytearray()
        with torch.cuda.stream(self._device()["stream"]):
            for pos in range(0, size, step):
                at, base, ln = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
                base[r], ln[r] = pos, min(step, size - pos)
                out += self._restore_window(at, base, ln, int(ln[r]))[:int(ln[r])].cpu().numpy().tobytes()
        return bytes(out)

    def restore(self, rows=None, window_bytes=256 << 20):
        """-> {row: bytes} for every row (or the rows named), from the store
        alone through sdcas_dev_family_restore: whole rows share a window of at
        most window_bytes, a longer row comes piece by piece"""
        import torch
        out = {}
        d = self._device()
        for group, streamed in self._windows(self._rows(rows), window_bytes):
            if streamed:
                out[group[0]] = self._pieces(group[0], window_bytes)
                continue
            at, base, ln, used = self._whole(group)
            with torch.cuda.stream(d["stream"]):
                host = self._restore_window(at, base, ln, used).cpu().numpy()
            for r in group:
                out[r] = host[int(at[r]):int(at[r] + ln[r])].tobytes()
        return out

    def verify(self, window_bytes=256 << 20):
        """-> the sorted rows that do not come back: every row restored in device
        memory, its window hashed there (sdcas_dev_hash_messages) and the
        digest compared with `digests`. A row larger than a window is restored
        to the host in pieces and hashed through Engine.hash_messages."""
        import torch
        bad = []
        d, eng = self._device(), self._engine()
        for group, streamed in self._windows(self._rows(None), window_bytes):
            if streamed:
                r = group[0]
                data = np.frombuffer(self._pieces(r, window_bytes), np.uint8)
                got = eng.hash_messages(data, [0], [data.size])[0]
                if not np.array_equal(got, self.digests[r]):
                    bad.append(r)
                continue
            at, base, ln, used = self._whole(group)
            sel = np.array(group, np.int64)
            lens = ln[sel]
            eng.dev_reserve(len(group), int(np.maximum((lens + np.uint64(1023)) // np.uint64(1024), 1).sum()))
            with torch.cuda.stream(d["stream"]):
                blob = self._restore_window(at, base, ln, used)
                d_offs, d_lens = self._up(at[sel], d["device"]), self._up(lens, d["device"])
                out = torch.zeros(32 * len(group), dtype=torch.uint8, device=d["device"])
                eng.dev_hash_messages(blob.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), len(group),
                                      out.data_ptr(), 0, d["stream"].cuda_stream)
                got = out.cpu().numpy().reshape(-1, 32)
            bad += [r for j, r in enumerate(group) if not np.array_equal(got[j], self.digests[r])]
        return sorted(bad)

    # -- forgetting rows -------------------------------------------------------------------
    def remove(self, rows):
        """-> (FamilyStore, row_from): the store without `rows`, equal to the
        one built from the remaining files alone, and per new row its old
        number. No file is read: the chunk arrays lose the rows' chunks
        (dev_family_chunks_keep), the recipes and the layout run over the rest,
        and every literal byte of the new store is carried from where it lies
        in the old one (dev_family_store_moves, then the mover), all on the
        device. This object stays as it is. ValueError for a store without
        chunk arrays or a row out of range; SdcasError SDCAS_E_CAPACITY when
        the two stores do not fit in device memory."""
        import torch
        if self.chunks is None:
            raise ValueError("FamilyStore.remove: the store carries no chunk arrays (it was saved before they were kept)")
        n = self.sizes.size
        gone = sorted({int(r) for r in rows})
        if any(not 0 <= r < n for r in gone):
            raise ValueError(f"FamilyStore.remove: a row outside [0, {n})")
        keep = np.ones(n, np.uint8)
        keep[np.array(gone, np.int64)] = 0
        d, eng, ch, r = self._device(), self._engine(), self.chunks, self.recipes
        dev, m, k = d["device"], ch["chunk_file"].size, d["k"]
        n2 = int(keep.sum())
        m2 = int(keep[ch["chunk_file"].astype(np.int64)].sum())  # check: chunk_file < n

        def room(count, dtype):
            return torch.zeros(max(int(count), 2), dtype=dtype, device=dev)

        def down(t, count, dtype):
            return t[:int(count)].cpu().numpy().view(dtype).copy()

        i32, i64, st = torch.int32, torch.int64, d["stream"].cuda_stream
        with torch.cuda.stream(d["stream"]):
            o_file, o_off, o_len, o_rep, o_fam, o_keep, o_chunk_op, o_dst = (self._up(a, dev) for a in (
                ch["chunk_file"], np.asarray(r["chunk_off"], np.uint64), ch["chunk_len"], ch["rep"], ch["family"], keep,
                np.asarray(r["chunk_op"], np.uint32), np.asarray(r["op_dst_off"], np.uint64)))
            row_from, fam2 = room(n, i32), room(n, i64)
            c_from, c_file, c_off, c_len, c_rep = room(m, i32), room(m, i32), room(m, i64), room(m, i64), room(m, i64)
            kc, rc, lc, mc = room(6, i64), room(8, i64), room(6, i64), room(6, i64)
            eng.dev_family_chunks_keep(o_file.data_ptr(), o_off.data_ptr(), o_len.data_ptr(), o_rep.data_ptr(), m,
                                       o_fam.data_ptr(), o_keep.data_ptr(), n, 0, row_from.data_ptr(),
                                       fam2.data_ptr(), c_from.data_ptr(), c_file.data_ptr(), c_off.data_ptr(),
                                       c_len.data_ptr(), c_rep.data_ptr(), kc.data_ptr(), st)
            op32 = [room(m2, i32) for _ in range(4)]
            op64 = [room(m2, i64) for _ in range(3)]
            chunk_op, row_ops, row_first, off2 = room(m2, i32), room(n2, i32), room(n2, i32), room(m2, i64)
            eng.dev_family_recipes(c_file.data_ptr(), c_off.data_ptr(), c_len.data_ptr(), c_rep.data_ptr(), m2,
                                   fam2.data_ptr(), n2, *(t.data_ptr() for t in op32 + op64), chunk_op.data_ptr(),
                                   row_ops.data_ptr(), row_first.data_ptr(), rc.data_ptr(), st)
            eng.dev_family_store_layout(*(t.data_ptr() for t in op32 + op64), chunk_op.data_ptr(), m2,
                                        rc.data_ptr() + 16, m2, off2.data_ptr(), lc.data_ptr(), st)
            mv_dst, mv_src, mv_len = room(m2, i64), room(m2, i64), room(m2, i64)
            eng.dev_family_store_moves(o_off.data_ptr(), o_chunk_op.data_ptr(), m, o_dst.data_ptr(),
                                       d["off"].data_ptr(), d["ops"].data_ptr(), k, c_from.data_ptr(),
                                       c_off.data_ptr(), c_len.data_ptr(), chunk_op.data_ptr(), kc.data_ptr() + 16, m2,
                                       op32[0].data_ptr(), op32[1].data_ptr(), op64[0].data_ptr(), off2.data_ptr(),
                                       rc.data_ptr() + 16, m2, mv_dst.data_ptr(), mv_src.data_ptr(), mv_len.data_ptr(),
                                       mc.data_ptr(), st)
            kcs, rcs, lcs, mcs = (down(t, c, np.uint64) for t, c in ((kc, 6), (rc, 8), (lc, 6), (mc, 6)))
            if int(kcs[0]) != n2 or int(kcs[2]) != m2:
                raise RuntimeError("FamilyStore.remove: the device kept other rows or chunks than the host counted")
            if int(mcs[3]):
                raise ValueError(f"FamilyStore.remove: {int(mcs[3])} literal chunks of the new store have no place in "
                                 f"the old one")
            ops2, size2 = int(rcs[2]), int(lcs[4])
            if size2 > self.store.size:
                raise RuntimeError("FamilyStore.remove: the new store is larger than the old one")
            free, _ = torch.cuda.mem_get_info(dev)
            if size2 + 32 > free:
                raise N.SdcasError(N.SDCAS_E_CAPACITY, f"FamilyStore.remove: a second store of {size2} bytes does not "
                                                       f"fit in the {free} bytes free on the device")
            try:
                store2 = torch.zeros(size2 + 32, dtype=torch.uint8, device=dev)
            except torch.cuda.OutOfMemoryError as e:
                raise N.SdcasError(N.SDCAS_E_CAPACITY, f"FamilyStore.remove: a second store of {size2} bytes: {e}") from e
            # the moves as the mover's ops: one row, one window over the new store
            zero_rows = room(m2, i32)
            w_at, w_len = self._up(np.zeros(1, np.uint64), dev), self._up(np.array([size2], np.uint64), dev)
            moved = room(4, i64)
            eng.dev_family_restore(zero_rows.data_ptr(), mv_dst.data_ptr(), mv_len.data_ptr(), mv_src.data_ptr(),
                                   mc.data_ptr(), m2, w_at.data_ptr(), 0, w_len.data_ptr(), 1, d["store"].data_ptr(),
                                   self.store.size, store2.data_ptr(), size2, moved.data_ptr(), st)
            mvd = down(moved, 4, np.uint64)
            if int(mvd[1]) != size2 or int(mvd[2]):
                raise RuntimeError(f"FamilyStore.remove: {int(mvd[1])} of {size2} bytes moved, {int(mvd[2])} bad moves")
            names = ("op_chunk", "op_src_chunk", "op_row", "op_src_row", "op_dst_off", "op_src_off", "op_len")
            recipes = {name: down(t, ops2, np.uint32 if t.dtype == i32 else np.uint64)
                       for name, t in zip(names, op32 + op64)}
            recipes.update({"op_literal": recipes["op_chunk"] == recipes["op_src_chunk"],
                            "chunk_op": down(chunk_op, m2, np.uint32), "row_ops": down(row_ops, n2, np.uint32),
                            "row_first_op": down(row_first, n2, np.uint32), "chunk_off": down(c_off, m2, np.uint64),
                            "counts": {name: int(v) for (name, _), v in zip(N.FamilyRecipesCounts._fields_, rcs)}})
            layout = {"op_store_off": down(off2, ops2, np.uint64),
                      "counts": {name: int(v) for (name, _), v in zip(N.FamilyStoreCounts._fields_, lcs)}}
            chunks = {"chunk_file": down(c_file, m2, np.uint32), "chunk_len": down(c_len, m2, np.uint64),
                      "rep": down(c_rep, m2, np.int64), "family": down(fam2, n2, np.int64)}
            frm = down(row_from, n2, np.uint32)
            store = store2[:size2].cpu().numpy()
        sel = frm.astype(np.int64)
        return FamilyStore(recipes, layout, store, self.sizes[sel], self.digests[sel], self.engine, chunks), frm

    # -- from files ------------------------------------------------------------------------
    @classmethod
    def of_files(cls, engine, paths, k=4, max_holders=64, num=1, den=2, params=None, window_bytes=256 << 20):
        """Engine.store_files"""
        import torch
        paths = [os.fspath(p) for p in paths]
        # similar_recipes' steps, keeping the recipes' inputs: `remove` needs them
        from .engine import ChunkHolders
        ids = np.arange(len(paths), dtype=np.uint64)
        found = engine.similar_files_indexed(paths, ids, ChunkHolders(engine), params, window_bytes, peers=int(k),
                                             max_holders=max_holders, chunks=True)
        fam, fl, ln, rep = engine._family_inputs([found], [ids], num, den, "store_files")
        chunks = {"chunk_file": fl, "chunk_len": ln, "rep": rep, "family": fam["family"]}
        recipes, sizes = engine.family_recipes(fl, ln, rep, fam["family"]), np.asarray(found["sizes"], np.uint64)
        layout = engine.family_store_layout(recipes)
        store_bytes, n = int(layout["counts"]["store_bytes"]), len(paths)
        device = torch.device(f"cuda:{engine.device_ordinal}")
        free, _ = torch.cuda.mem_get_info(device)
        if store_bytes + 32 > free:
            raise N.SdcasError(N.SDCAS_E_CAPACITY, f"store_files: a store of {store_bytes} bytes does not fit in the "
                                                   f"{free} bytes free on the device")
        stream = torch.cuda.Stream(device)
        with torch.cuda.stream(stream):
            try:
                d_store = torch.zeros(store_bytes + 32, dtype=torch.uint8, device=device)
            except torch.cuda.OutOfMemoryError as e:
                raise N.SdcasError(N.SDCAS_E_CAPACITY, f"store_files: a store of {store_bytes} bytes: {e}") from e
            d = cls._ops_up(recipes, layout, device)

            def pack(blob, at, base, ln):
                d_blob = cls._up(np.concatenate([blob, np.zeros(-blob.size % 16 + 16, np.uint8)]), device)
                d_at, d_base, d_ln = (cls._up(a, device) for a in (at, base, ln))
                engine.dev_family_pack(d["op_chunk"].data_ptr(), d["op_src_chunk"].data_ptr(), d["op_row"].data_ptr(),
                                       d["op_dst_off"].data_ptr(), d["op_len"].data_ptr(), d["off"].data_ptr(),
                                       d["ops"].data_ptr(), d["k"], d_at.data_ptr(), d_base.data_ptr(),
                                       d_ln.data_ptr(), n, d_blob.data_ptr(), blob.size, d_store.data_ptr(),
                                       store_bytes, stream=stream.cuda_stream)
                stream.synchronize()  # the window's tensors are let go after the call has read them

            for first, nf, streamed in engine.plan_windows([int(s) for s in sizes], window_bytes):
                at, base, ln = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
                if not streamed:
                    data, pos = [], 0
                    for r in range(first, first + nf):
                        with open(paths[r], "rb") as f:
                            b = f.read()
                        if len(b) != int(sizes[r]):
                            raise OSError(f"{paths[r]}: {len(b)} bytes, {int(sizes[r])} when it was chunked")
                        at[r], ln[r] = pos, len(b)
                        data.append(b + bytes(-len(b) % 16))
                        pos += len(data[-1])
                    pack(np.frombuffer(b"".join(data), np.uint8), at, base, ln)
                    continue
                with open(paths[first], "rb") as f:
                    step = max(16, int(window_bytes)) // 16 * 16
                    for pos in range(0, int(sizes[first]), step):
                        f.seek(pos)
                        b = f.read(min(step, int(sizes[first]) - pos))
                        at[first], base[first], ln[first] = 0, pos, len(b)
                        pack(np.frombuffer(b, np.uint8), at, base, ln)
            store = d_store[:store_bytes].cpu().numpy()
        digests, st = engine.file_checksums(paths)
        if st.any():
            from .engine import io_error
            i = int(np.flatnonzero(st)[0])
            raise io_error(int(st[i]), paths[i])
        return cls(recipes, layout, store, sizes, digests, engine, chunks)
