"""Test infrastructure: device (or CPU) buffers with guard bands, for tests of
what a call does to the memory AROUND its arguments.

`Guarded(nbytes)` is one uint8 allocation laid out as

    [ front guard >= 4096 B | payload nbytes | back guard >= 4096 B ]

The guards hold a position-dependent pattern, so a stray store of any
constant (0x00 and 0xFF included) shows at all but one position in 256; the
payload is prefilled with `fill`, so a test sees which payload bytes a
call left alone. The payload starts at an address that is `align`-aligned and
NOT `2 * align`-aligned: a test runs at the alignment the contract promises,
not at the allocator's 256 bytes.

Every payload lies inside its allocation with at least 4096 readable bytes
behind it: the 64-byte over-read the device API allows itself lands in guard
memory. Nothing here places a buffer at the end of an allocation — a test must
never provoke a fault to make its point.

`MessageBlob` lays messages out in one guarded blob at chosen start residues
mod 64 with poisoned gaps between them.
"""
import numpy as np
import torch

GUARD = 4096
GAP = 64  # the blob is readable this far past every message's end (include/sdcas.h)


def _pattern(lo, hi):
    """guard bytes of allocation positions [lo, hi)"""
    return ((131 * np.arange(lo, hi, dtype=np.int64) + 17) & 0xFF).astype(np.uint8)


class Guarded:
    def __init__(self, nbytes, device="cuda", align=16, fill=0xC3):
        assert nbytes >= 0 and align >= 1 and (align & (align - 1)) == 0
        self.nbytes = int(nbytes)
        self.align = align
        self.fill = fill
        total = self.nbytes + 2 * GUARD + 2 * align
        self.raw = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        # the first position >= GUARD whose address is align (mod 2 * align)
        self.start = GUARD + (align - (base + GUARD)) % (2 * align)
        self.ptr = base + self.start
        assert self.ptr % align == 0 and self.ptr % (2 * align) == align
        assert self.start >= GUARD and total - self.start - self.nbytes >= GUARD
        img = np.full(total, fill, np.uint8)
        img[:self.start] = _pattern(0, self.start)
        img[self.start + self.nbytes:] = _pattern(self.start + self.nbytes, total)
        self.raw.copy_(torch.from_numpy(img))
        self._snap = None

    # -- the payload ------------------------------------------------------------
    def view(self, dtype=torch.uint8, count=None):
        """the payload's first `count` elements of `dtype` (all of it by
        default), as a tensor sharing the allocation"""
        size = torch.empty(0, dtype=dtype).element_size()
        count = self.nbytes // size if count is None else int(count)
        assert count * size <= self.nbytes
        return self.raw[self.start:self.start + count * size].view(dtype)

    def upload(self, arr):
        """copy a host array's bytes to the start of the payload"""
        b = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert b.size <= self.nbytes, (b.size, self.nbytes)
        if b.size:
            self.raw[self.start:self.start + b.size].copy_(torch.from_numpy(b.copy()))
        return self

    def download(self, dtype=np.uint8, count=None):
        """the payload's first `count` elements of numpy `dtype` on the host"""
        size = np.dtype(dtype).itemsize
        count = self.nbytes // size if count is None else int(count)
        assert count * size <= self.nbytes
        return self.raw[self.start:self.start + count * size].cpu().numpy().copy().view(dtype)

    # -- the checks -------------------------------------------------------------
    def check(self):
        """offsets, relative to the payload's start, of the guard bytes that
        no longer hold their pattern ([] when both guards are intact): -1 is
        the byte before the payload, nbytes the first one after it"""
        got = self.raw.cpu().numpy()
        end = self.start + self.nbytes
        front = np.flatnonzero(got[:self.start] != _pattern(0, self.start)) - self.start
        back = np.flatnonzero(got[end:] != _pattern(end, got.size)) + self.nbytes
        return [int(x) for x in front] + [int(x) for x in back]

    def snapshot(self):
        """remember the payload as it is now (an input, before a call)"""
        self._snap = self.download()
        return self

    def changed(self):
        """offsets of the payload bytes that differ from the snapshot"""
        assert self._snap is not None, "snapshot() first"
        return [int(x) for x in np.flatnonzero(self.download() != self._snap)]

    def unchanged(self):
        return not self.changed()

    def untouched(self, lo=0, hi=None):
        """True when payload bytes [lo, hi) still hold the prefill"""
        return bool((self.download()[lo:hi] == self.fill).all())


def guarded_from(arr, device="cuda", align=16, snapshot=True):
    """an input: a Guarded of exactly the array's bytes, uploaded (and
    snapshotted, for `unchanged()` after the call)"""
    b = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    g = Guarded(b.size, device, align).upload(b)
    return g.snapshot() if snapshot else g


def place(lengths, residues, base, gap=GAP):
    """offsets for messages of `lengths` bytes in a blob whose payload starts
    at address `base`: message i at the next offset whose ADDRESS is
    residues[i % len(residues)] mod 64, at least `gap` bytes after the end of
    the message before -> (offsets, bytes used including the last gap)"""
    offs, cur = [], 0
    for i, n in enumerate(lengths):
        r = residues[i % len(residues)]
        assert 0 <= r < 64
        off = cur + (r - (base + cur)) % 64
        offs.append(off)
        cur = off + int(n) + gap
    return offs, cur


class MessageBlob:
    """`messages` (bytes-like) in one guarded blob, message i starting at an
    address that is residues[i % len(residues)] mod 64, at least 64 bytes
    between the end of one and the start of the next and after the last, every
    byte that belongs to no message holding `poison`.

    .g the Guarded, .ptr its payload address, .offsets (list of int, relative
    to .ptr), .lengths, .image the payload's bytes as laid out on the host."""

    def __init__(self, messages, residues, poison, device="cuda", align=16, gap=GAP):
        self.lengths = [len(m) for m in messages]
        # room for any base address: up to 63 bytes of slack before each message
        room = sum(self.lengths) + (gap + 63) * len(messages) + gap
        self.g = Guarded(room, device, align, fill=poison)
        self.ptr = self.g.ptr
        self.offsets, used = place(self.lengths, residues, self.ptr, gap)
        assert used <= room
        self.image = np.full(room, poison, np.uint8)
        for off, m in zip(self.offsets, messages):
            self.image[off:off + len(m)] = np.frombuffer(bytes(m), np.uint8)
        self.g.upload(self.image).snapshot()

    def addresses(self):
        return [self.ptr + o for o in self.offsets]
