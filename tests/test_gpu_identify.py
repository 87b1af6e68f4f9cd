"""GPU parity of the one-pass cas_id + checksum (sdcas_dev_identify,
sdcas_identify_checksums; csrc/b3_dual.hip): every cas key
(core/src/object/cas.rs:23-62) and every checksum
(core/src/object/validation/hash.rs:11-25) against the CPU oracle, at the
lengths where the two messages' last block, block count and chunk count
differ, where the branch changes (100 KiB, 1 MiB) and where chunks of one file
cross workgroup tiles."""
import os

import numpy as np
import pytest
import torch

from spacedrive_amd import _native as N
from tests._oracle import content_key

pytestmark = pytest.mark.gpu

MiB = 1 << 20
BOUNDARY = [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 121, 1015, 1016, 1017, 1023, 1024, 1025, 2039, 2040, 2041, 2047,
            2048, 2049, 65536, 102399, 102400, 102401, 102402, 114688, 1048576, 1048577]
SEED = 0x1DE7


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


_want = {}


def want(oracle, key, size):
    """(cas key or None, checksum hex) of the synthetic file (key, size), computed once"""
    if (key, size) not in _want:
        _want[(key, size)] = (oracle.synth_cas_key(key, size) if size else None, oracle.synth_checksum(key, size))
    return _want[(key, size)]


def _t(a):
    return torch.from_numpy(np.asarray(a, np.uint64).view(np.int64)).cuda()


def _chunks(size):
    return max(1, -(-size // 1024))


def reserve_for(eng, sizes):
    a = sum(_chunks(s + 8) if 1 <= s <= 102400 else 1 for s in sizes)
    b = sum(_chunks(s) for s in sizes if s > 102400)
    eng.dev_reserve(len(sizes), max(2 * (a + 2048), b) + 4096)


def dev_identify(eng, keys, sizes, poison=False, out_keys=True, out_digests=True):
    """lay the synthetic contents out with 16 B before and 64 B after each
    (poisoned: those gaps hold 0xA5 bytes), run sdcas_dev_identify"""
    n = len(sizes)
    offs, off = [], 16
    for s in sizes:
        offs.append(off)
        off = (off + s + 64 + 15) // 16 * 16 + 16
    blob = torch.full((off + 64,), 0xA5 if poison else 0, dtype=torch.uint8, device="cuda")
    args = [_t(keys), _t([0] * n), _t(sizes), _t(offs)]
    torch.cuda.synchronize()
    eng.dev_synth_content(*(a.data_ptr() for a in args), n, blob.data_ptr())
    reserve_for(eng, sizes)
    k = torch.zeros(n, dtype=torch.int64, device="cuda")
    d = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    h = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    eng.dev_identify(blob.data_ptr(), args[3].data_ptr(), args[2].data_ptr(), n,
                     k.data_ptr() if out_keys else 0, d.data_ptr() if out_digests else 0, h.data_ptr())
    eng.dev_sync()
    return k.cpu().numpy().view(np.uint64), d.cpu().numpy(), h.cpu().numpy()


def check(oracle, keys, sizes, got, has_keys=True, has_digests=True):
    k, d, h = got
    for i, (key, s) in enumerate(zip(keys, sizes)):
        wk, wd = want(oracle, key, s)
        assert h[i] == (1 if s else 0), (i, s)
        if has_keys and s:
            assert f"{int(k[i]):016x}" == f"{wk:016x}", f"cas key of file {i}, {s} bytes"
        if has_digests:
            assert bytes(d[i]).hex() == wd, f"checksum of file {i}, {s} bytes"


def _keys(n, base=0):
    return [content_key(SEED, base + i) for i in range(n)]


def test_boundary_lengths_one_batch(eng, oracle):
    keys = _keys(len(BOUNDARY))
    check(oracle, keys, BOUNDARY, dev_identify(eng, keys, BOUNDARY))


def test_boundary_lengths_reversed(eng, oracle):
    """a neighbouring file's bytes cannot stand in for a missing mask"""
    keys = _keys(len(BOUNDARY))[::-1]
    sizes = BOUNDARY[::-1]
    check(oracle, keys, sizes, dev_identify(eng, keys, sizes))


@pytest.mark.parametrize("idx", range(len(BOUNDARY)))
def test_boundary_length_alone(eng, oracle, idx):
    keys = [_keys(len(BOUNDARY))[idx]]
    check(oracle, keys, [BOUNDARY[idx]], dev_identify(eng, keys, [BOUNDARY[idx]]))


def test_tile_straddles(eng, oracle):
    """~25 MB of whole-file contents: chunks of one file cross workgroup tile
    boundaries in both plans (the cas plan's slots run ahead of the checksum
    plan's by one chunk per file whose cas message has the extra chunk)"""
    rng = np.random.default_rng(77)
    sizes = [int(x) for x in rng.integers(1, 102401, 400)] + [102400] * 40
    order = rng.permutation(len(sizes))
    sizes = [sizes[i] for i in order]
    keys = _keys(len(sizes), 1000)
    check(oracle, keys, sizes, dev_identify(eng, keys, sizes))


def test_null_outputs_and_poisoned_padding(eng, oracle):
    keys = _keys(len(BOUNDARY))
    got = dev_identify(eng, keys, BOUNDARY, poison=True)
    check(oracle, keys, BOUNDARY, got)
    k, d, h = dev_identify(eng, keys, BOUNDARY, poison=True, out_digests=False)
    check(oracle, keys, BOUNDARY, (k, d, h), has_digests=False)
    assert not d.any()
    k, d, h = dev_identify(eng, keys, BOUNDARY, poison=True, out_keys=False)
    check(oracle, keys, BOUNDARY, (k, d, h), has_keys=False)
    assert not k.any()


def test_a_batch_past_the_reserved_slots_is_a_capacity_error():
    """each plan has half of the reserved slots: a batch past them is reported
    by dev_sync (the kernels leave it unhashed), as dev_hash_messages reports it"""
    from spacedrive_amd import Engine
    sizes = [102400] * 64  # 6464 cas chunks against 2048 slots per plan
    n = len(sizes)
    offs = [i * 102528 for i in range(n)]
    blob = torch.zeros(n * 102528 + 64, dtype=torch.uint8, device="cuda")
    a = [_t(offs), _t(sizes)]
    k = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with Engine() as e:
        e.dev_reserve(n, 2048)
        e.dev_identify(blob.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), n, k.data_ptr(), 0, 0)
        with pytest.raises(N.SdcasError) as ei:
            e.dev_sync()
        assert ei.value.code == N.SDCAS_E_CAPACITY
    assert not k.any().item()


# ---- sdcas_identify_checksums on real files ----------------------------------

def _write(path, rng, size):
    with open(path, "wb") as f:
        f.write(rng.integers(0, 256, size, dtype=np.uint8).tobytes())


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the boundary lengths and a streamed file, plus an empty file, a
    directory, a missing path and an unreadable file"""
    root = tmp_path_factory.mktemp("identify")
    rng = np.random.default_rng(5)
    paths = []
    for s in BOUNDARY + [3 * MiB + 17]:
        p = root / f"f{s}.bin"
        _write(p, rng, s)
        paths.append(str(p))
    (root / "dir").mkdir()
    paths.append(str(root / "dir"))
    paths.append(str(root / "missing.bin"))
    un = root / "unreadable.bin"
    _write(un, rng, 300)
    os.chmod(un, 0)
    paths.append(str(un))
    return paths


def check_files(oracle, e, paths, got):
    """against file_metadata followed by file_checksums, and the oracle"""
    sizes, keys, dig, st, fl = got
    msz, mk, mst, mfl = e.file_metadata(paths)
    cd, cst = e.file_checksums(paths)
    for i, p in enumerate(paths):
        assert sizes[i] == msz[i], p
        assert st[i] == mst[i], p
        assert (fl[i] & 3) == mfl[i], p
        assert bool(fl[i] & N.SDCAS_META_HAS_CHECKSUM) == (cst[i] == 0), p
        if fl[i] & N.SDCAS_META_HAS_CAS_ID:
            assert keys[i] == mk[i], p
            assert f"{int(keys[i]):016x}" == oracle.generate_cas_id(p, int(sizes[i])), p
        if fl[i] & N.SDCAS_META_HAS_CHECKSUM:
            assert bytes(dig[i]) == bytes(cd[i]), p
            assert bytes(dig[i]).hex() == oracle.file_checksum(p), p
    n_reg = sum(1 for p in paths if os.path.isfile(p) and os.access(p, os.R_OK))
    assert int(((fl & N.SDCAS_META_HAS_CHECKSUM) != 0).sum()) == n_reg


def test_identify_checksums_files(eng, oracle, tree):
    check_files(oracle, eng, tree, eng.identify_checksums(tree))
    hints = [os.path.getsize(p) if os.path.isfile(p) else 0 for p in tree]
    check_files(oracle, eng, tree, eng.identify_checksums(tree, hints))


def test_identify_checksums_stale_hints(eng, oracle, tmp_path):
    rng = np.random.default_rng(6)
    sizes = [100, 102000, MiB - 100, 70000, 2 * MiB + 5, 5000]
    paths = []
    for i, s in enumerate(sizes):
        p = tmp_path / f"s{i}.bin"
        _write(p, rng, s)
        paths.append(str(p))
    hints = list(sizes)
    with open(paths[1], "ab") as f:  # across 102400
        f.write(b"x" * 5000)
    with open(paths[2], "ab") as f:  # across 1 MiB
        f.write(b"y" * 4096)
    os.truncate(paths[3], 10)        # shrunk
    os.truncate(paths[4], 1000)      # hinted as streamed, small now
    got = eng.identify_checksums(paths, hints)
    assert not got[3].any()
    assert list(got[0]) == [os.path.getsize(p) for p in paths]
    check_files(oracle, eng, paths, got)


def test_identify_checksums_direct_io(oracle, tree):
    from spacedrive_amd import Engine
    with Engine(direct_io=True) as e:
        check_files(oracle, e, tree, e.identify_checksums(tree))


def test_identify_checksums_batch_larger_than_a_slot(oracle, tmp_path):
    """both staging slots and the drain: 200 files of 1-100 KiB through 4 MiB slots"""
    from spacedrive_amd import Engine
    rng = np.random.default_rng(8)
    paths = []
    for i, s in enumerate(rng.integers(1024, 102401, 200)):
        p = tmp_path / f"b{i}.bin"
        _write(p, rng, int(s))
        paths.append(str(p))
    with Engine(staging_bytes=4 * MiB) as e:
        sizes, keys, dig, st, fl = e.identify_checksums(paths)
    assert not st.any() and (fl == (N.SDCAS_META_HAS_CAS_ID | N.SDCAS_META_HAS_CHECKSUM)).all()
    for i, p in enumerate(paths):
        assert f"{int(keys[i]):016x}" == oracle.generate_cas_id(p, int(sizes[i])), p
        assert bytes(dig[i]).hex() == oracle.file_checksum(p), p
