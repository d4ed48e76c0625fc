"""bench.py --dump-outputs on host tensors: the files, their layout, and the seeded sample that keeps a long series within 64 MB."""
import numpy as np
import torch

import bench


def _records(T, nl):
    return torch.arange(T * (16 + 21 * nl), dtype=torch.float64).reshape(T, -1)


def test_dump_splits_the_records_into_fp64_files(tmp_path):
    rec = _records(5, 3)
    bench.dump_outputs(str(tmp_path), rec, nanflag=torch.tensor([0, 1, 0, 0, 2], dtype=torch.int32))
    s, lv = np.load(tmp_path / "scalars.npy"), np.load(tmp_path / "levels.npy")
    t, nf = np.load(tmp_path / "time_index.npy"), np.load(tmp_path / "nanflag.npy")
    assert s.dtype == lv.dtype == t.dtype == nf.dtype == np.float64
    assert s.shape == (5, 16) and lv.shape == (5, 21, 3) and list(t) == list(range(5)) and list(nf) == [0, 1, 0, 0, 2]
    r = rec.numpy()
    assert np.array_equal(s, r[:, :16]) and np.array_equal(lv[:, 4, 2], r[:, 16 + 4 * 3 + 2])
    bench.dump_outputs(str(tmp_path), rec)                 # a run without nanflag leaves no stale one behind
    assert not (tmp_path / "nanflag.npy").exists()


def test_a_long_series_is_cut_to_the_same_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40 * 8 * (16 + 21 * 3 + 1))
    rec = _records(100, 3)
    picks = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rec)
        total = sum((tmp_path / d / f).stat().st_size - 128 for f in ("scalars.npy", "levels.npy", "time_index.npy"))
        assert total <= bench.DUMP_LIMIT_BYTES
        t = np.load(tmp_path / d / "time_index.npy").astype(int)
        assert len(t) == 40 and np.all(np.diff(t) > 0)
        assert np.array_equal(np.load(tmp_path / d / "scalars.npy"), rec.numpy()[t, :16])
        picks.append(t)
    assert np.array_equal(*picks)
