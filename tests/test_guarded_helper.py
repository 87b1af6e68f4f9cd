"""The guarded-buffer helper (tests/_guarded.py) on CPU tensors: it reports a
byte written just outside the payload at the right offset, stays silent on an
untouched buffer, places the payload at the promised residue, and lays
messages out at the residues asked for with poisoned gaps."""
import numpy as np
import pytest
import torch

from tests._guarded import GAP, GUARD, Guarded, MessageBlob, guarded_from, place


@pytest.mark.parametrize("nbytes", [0, 1, 48, 131, 4096])
def test_untouched_buffer_reports_nothing(nbytes):
    g = Guarded(nbytes, "cpu")
    assert g.check() == []
    assert g.untouched()
    assert g.download().size == nbytes


@pytest.mark.parametrize("nbytes", [1, 48, 131])
@pytest.mark.parametrize("value", [0x00, 0xFF, 0xC3])
def test_a_byte_past_either_end_is_reported(nbytes, value):
    g = Guarded(nbytes, "cpu")
    want = []
    for off in (nbytes, -1):
        pos = g.start + off
        if int(g.raw[pos]) == value:  # the one position in 256 whose pattern is this constant
            continue
        g.raw[pos] = value
        want.append(off)
    assert sorted(g.check()) == sorted(want) and want
    assert g.untouched()  # the payload itself was not written


def test_one_byte_past_and_one_before():
    g = Guarded(100, "cpu")
    g.raw[g.start + 100] ^= 0x5A
    assert g.check() == [100]
    g = Guarded(100, "cpu")
    g.raw[g.start - 1] ^= 0x5A
    assert g.check() == [-1]
    g = Guarded(100, "cpu")
    g.raw[0] ^= 1
    g.raw[g.raw.numel() - 1] ^= 1
    assert g.check() == [-g.start, g.raw.numel() - 1 - g.start]


def test_a_wide_stray_store_of_a_constant_shows():
    """sixteen bytes of one value, as a too-wide uint4 store would leave"""
    for value in (0x00, 0xFF):
        g = Guarded(64, "cpu")
        g.raw[g.start + 64:g.start + 80] = value
        bad = g.check()
        assert len(bad) >= 15 and set(bad) <= set(range(64, 80))


@pytest.mark.parametrize("align", [1, 4, 8, 16, 64])
def test_payload_address_residue_and_guard_sizes(align):
    for nbytes in (0, 1, 33, 1000):
        g = Guarded(nbytes, "cpu", align=align)
        assert g.ptr == g.raw.data_ptr() + g.start
        assert g.ptr % align == 0 and g.ptr % (2 * align) == align
        assert g.start >= GUARD
        assert g.raw.numel() - g.start - nbytes >= GUARD


def test_payload_access_and_snapshot():
    g = Guarded(48, "cpu", fill=0xC3)
    assert (g.download() == 0xC3).all()
    g.upload(np.arange(4, dtype=np.uint64))
    assert g.download(np.uint64, 4).tolist() == [0, 1, 2, 3]
    assert g.view(torch.int64, 4).tolist() == [0, 1, 2, 3]
    assert g.view(torch.int64, 4).data_ptr() == g.ptr
    assert not g.untouched() and g.untouched(32)
    g.snapshot()
    assert g.unchanged() and g.changed() == []
    g.view()[40] = 7
    assert not g.unchanged() and g.changed() == [40]
    assert g.check() == []
    a = np.arange(10, dtype=np.int32)
    h = guarded_from(a, "cpu")
    assert h.nbytes == 40 and h.unchanged() and h.download(np.int32).tolist() == a.tolist()


def test_place_honours_residues_and_gaps():
    lengths = [0, 1, 63, 64, 65, 1023, 1024, 1025, 5000]
    for base in (16, 48, 4096 + 16, 4096 + 48):
        offs, used = place(lengths, [16, 32, 48, 0], base)
        end = 0
        for i, (o, n) in enumerate(zip(offs, lengths)):
            assert (base + o) % 64 == [16, 32, 48, 0][i % 4]
            assert o % 16 == 0
            assert o >= end + (GAP if i else 0) and o - end < GAP + 64
            end = o + n
        assert used == end + GAP


@pytest.mark.parametrize("poison", [0x00, 0xFF, 0xA5])
def test_message_blob_layout_and_poison(poison):
    rng = np.random.default_rng(3)
    lengths = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3073, 7]
    msgs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]
    res = [16, 32, 48, 0]
    b = MessageBlob(msgs, res, poison, "cpu")
    assert b.g.check() == [] and b.g.unchanged()
    assert b.ptr % 32 == 16
    got = b.g.download()
    assert np.array_equal(got, b.image)
    covered = np.zeros(got.size, bool)
    for i, (o, m) in enumerate(zip(b.offsets, msgs)):
        assert (b.ptr + o) % 64 == res[i % 4]
        assert bytes(got[o:o + len(m)]) == m
        assert not covered[o:o + len(m) + GAP].any()  # 64 B after each message belong to no other
        covered[o:o + len(m)] = True
        assert o + len(m) + GAP <= got.size
        assert (got[o + len(m):o + len(m) + GAP] == poison).all()
    assert (got[~covered] == poison).all()
    assert b.addresses() == [b.ptr + o for o in b.offsets]
