"""The G step's instruction schedule (csrc/b3_device.h) through every product
kernel that carries one: one batch large enough for the big leaf kernel, with
every block-length edge and two messages that cross a tile, and three streamed
files through the piece kernels; every cas key and digest against the CPU
oracle, never against another GPU variant."""
import numpy as np
import pytest
import torch

from tests._oracle import content, content_key

pytestmark = pytest.mark.gpu
MiB = 1 << 20
KiB = 1 << 10

# the product kernels of the large-batch path and of the 1 MiB-piece path:
# all four run B3_G_ASM (the small-batch kernels keep the compiler's schedule)
LEAF_VARIANTS = [52, 67]
PIECE_VARIANTS = [17, 19]

EDGE_LENS = [0, 1, 55, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 16384, 16385]
FILLERS = 320  # x 64 KiB = 20 MiB: 20480 chunk slots, past the small-batch kernel's 2^14


@pytest.fixture(scope="module")
def leaf_batch(oracle):
    """(blob, offsets, lens, want digests, want keys, slot of every message),
    built and hashed by the oracle once. Caller order with the shape sort off:
    8 fillers (512 slots), the 1 MiB - 1 message (slots 512 .. 1535, across
    the tile boundary at 1024), the 1 MiB + 1 message (slots 1536 .. 2560,
    across 2048), the edge lengths, then the rest of the fillers."""
    lens = [64 * KiB] * 8 + [MiB - 1, MiB + 1] + EDGE_LENS + [64 * KiB] * (FILLERS - 8)
    msgs = [content("synth", 0, n, content_key(0x5D00A5, i)) for i, n in enumerate(lens)]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += (n + 127) // 128 * 128
    blob = np.zeros(pos + 64, np.uint8)
    for o, m in zip(offs, msgs):
        blob[o:o + m.size] = m
    want = [oracle.hash(m.tobytes()) for m in msgs]
    keys = [oracle.cas_key_of_message(m) for m in msgs]
    slots = np.cumsum([0] + [max(1, (n + 1023) // 1024) for n in lens])
    return blob, np.array(offs, np.uint64), np.array(lens, np.uint64), want, keys, slots


def test_leaf_batch_layout(leaf_batch):
    """the batch is what the docstring says: past 2^14 slots, the two long
    messages each across a 1024-slot tile boundary"""
    _, _, lens, _, _, slots = leaf_batch
    assert slots[-1] > 1 << 14
    for i in (8, 9):
        assert lens[i] in (MiB - 1, MiB + 1)
        assert slots[i] // 1024 != (slots[i + 1] - 1) // 1024, (i, slots[i], slots[i + 1])


@pytest.mark.parametrize("variant", LEAF_VARIANTS)
def test_leaf_variant_large_batch_vs_oracle(leaf_batch, variant):
    from spacedrive_amd import Engine
    blob, offs, lens, want, want_keys, slots = leaf_batch
    n = lens.size
    d_blob = torch.from_numpy(blob).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int64)).cuda()
    # poisoned outputs: a digest the kernel failed to write must not pass
    out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda")
    keys = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with Engine() as e:
        assert e.dev_set_leaf_variant(variant)
        e.dev_set_sort(0)
        e.dev_reserve(n, int(slots[-1]))
        e.dev_hash_messages(d_blob.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, out.data_ptr(),
                            keys.data_ptr())
        e.dev_sync()
        got = out.cpu().numpy()
        got_keys = keys.cpu().numpy().view(np.uint64)
    bad = [int(lens[i]) for i in range(n) if bytes(got[i]).hex() != want[i]]
    assert not bad, (variant, bad[:10])
    bad = [int(lens[i]) for i in range(n) if int(got_keys[i]) != want_keys[i]]
    assert not bad, (variant, bad[:10])


@pytest.mark.parametrize("variant", PIECE_VARIANTS)
def test_piece_variant_streamed_vs_oracle(oracle, variant):
    """1 MiB + 1, 2 MiB + 17 and 16 MiB + 1 bytes (level-4 nodes and the top
    kernel) through the streamed checksum, one segment per file"""
    from spacedrive_amd import Engine
    sizes = [MiB + 1, 2 * MiB + 17, 16 * MiB + 1]
    keys = [content_key(0x5D00A6, 32 * variant + i) for i in range(len(sizes))]
    boffs, used = [], 0
    for s in sizes:
        boffs.append(used)
        used += (s + MiB - 1) // MiB * MiB
    blob = torch.empty(used + 4096, dtype=torch.uint8, device="cuda")
    t = lambda a: torch.from_numpy(np.array(a, np.uint64).view(np.int64)).cuda()
    out = torch.full((len(sizes), 32), 0xA5, dtype=torch.uint8, device="cuda")
    args = [t(keys), t([0] * len(sizes)), t(sizes), t(boffs)]
    torch.cuda.synchronize()
    with Engine() as e:
        assert e.dev_set_piece_variant(variant)
        e.dev_synth_content(*(a.data_ptr() for a in args), len(sizes), blob.data_ptr())
        e.dev_sync()
        e.dev_stream_begin(sizes)
        e.dev_stream_update(list(range(len(sizes))), [0] * len(sizes), sizes, [blob.data_ptr() + b for b in boffs])
        e.dev_stream_finish(out.data_ptr())
        e.dev_sync()
        got = out.cpu().numpy()
    for i, (k, s) in enumerate(zip(keys, sizes)):
        assert bytes(got[i]).hex() == oracle.synth_checksum(k, s), (variant, s)
