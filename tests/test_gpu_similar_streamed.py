"""similar_files_streamed (chunk_stream's windows, one confirm and one sharing
pass over all chunks) against similar_files on a corpus that similar_files can
hold: every array and both count dicts are equal. Windows of 4 KiB and
segments of 2112 bytes, so that files are grouped, streamed alone over many
windows, and cut in segments."""
import numpy as np
import pytest

from tests import _cdc_ref as R

pytestmark = pytest.mark.gpu

P = R.TEST_PARAMS
SEG = 2112


@pytest.fixture(scope="module")
def eng():
    from spacedrive_amd import Engine
    e = Engine()
    yield e
    e.close()


def test_streamed_equals_resident(eng, tmp_path, monkeypatch):
    monkeypatch.setenv("SDCAS_CHUNK_SEG_BYTES", str(SEG))
    rng = np.random.default_rng(40)
    files = []
    for i in range(40):
        if i and i % 3 == 0:  # its predecessor with one byte inserted
            src = files[-1]
            at = int(rng.integers(0, src.size + 1))
            files.append(np.concatenate([src[:at], rng.integers(0, 256, 1, dtype=np.uint8), src[at:]]))
        elif i == 17:
            files.append(np.zeros(0, np.uint8))
        else:
            n = rng.integers(1024, 1500) if i % 5 in (1, 2) else rng.integers(1024, 20 * 1024)  # some share a window
            files.append(rng.integers(0, 256, int(n), dtype=np.uint8))
    run = rng.integers(0, 256, 5 * SEG, dtype=np.uint8)  # two long files that share a long run
    files.append(np.concatenate([rng.integers(0, 256, SEG // 2, dtype=np.uint8), run]))
    files.append(np.concatenate([run, rng.integers(0, 256, SEG + 5, dtype=np.uint8)]))
    paths = []
    for i, x in enumerate(files):
        p = tmp_path / f"f{i:03d}.bin"
        p.write_bytes(x.tobytes())
        paths.append(p)
    lens = [x.size for x in files]
    plan = eng.plan_windows(lens, 4096)
    assert any(s for _, _, s in plan) and any(not s and n > 1 for _, n, s in plan)
    want = eng.similar_files(paths, params=P)
    got = eng.similar_files_streamed(paths, window_bytes=4096, params=P)
    assert set(got) == set(want)
    for name, v in want.items():
        if isinstance(v, dict):
            assert got[name] == v, name
        else:
            assert got[name].dtype == v.dtype and got[name].shape == v.shape and (got[name] == v).all(), name
    assert want["sharing_counts"]["files_with_peer"] >= 10 and int(want["peer"][-1]) == len(files) - 2
    # the chunks of each window are numbered file by file
    seen = -1
    for w in eng.chunk_stream(paths, 4096, P):
        assert w["first_file"] >= seen and (np.diff(w["chunk_file"].astype(np.int64)) >= 0).all()
        seen = w["first_file"]
