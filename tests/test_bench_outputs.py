"""bench.py --dump-outputs on the host: what is written, in which dtype, and the seeded frame sample beyond the size budget."""
import numpy as np
import torch

from bench import dump_outputs


def test_dump_outputs_writes_float32_arrays_whole_under_the_budget(tmp_path):
    pred = torch.rand(4, 3, 8, 8, dtype=torch.float64)
    rec = dump_outputs(str(tmp_path), {"prediction": pred}, "", 1 << 20)
    got = np.load(tmp_path / "prediction.npy")
    assert got.dtype == np.float32 and np.array_equal(got, pred.float().numpy())
    assert rec["arrays"] == {"prediction": {"shape": [4, 3, 8, 8], "frames_of": 4}}
    assert sorted(p.name for p in tmp_path.iterdir()) == ["prediction.npy"]


def test_dump_outputs_samples_the_same_frames_beyond_the_budget(tmp_path):
    pred = torch.rand(10, 3, 8, 8)
    frame = 3 * 8 * 8 * 4
    for run in ("a", "b"):
        rec = dump_outputs(str(tmp_path / run), {"prediction": pred}, ".rank1", 4 * frame + 7)
        assert rec["arrays"] == {"prediction.rank1": {"shape": [4, 3, 8, 8], "frames_of": 10}}
    idx_a, idx_b = (np.load(tmp_path / r / "prediction_frames.rank1.npy") for r in ("a", "b"))
    assert idx_a.dtype == np.float64 and np.array_equal(idx_a, idx_b) and len(set(idx_a)) == 4
    assert np.all(np.diff(idx_a) > 0) and 0 <= idx_a.min() and idx_a.max() < 10
    got = np.load(tmp_path / "a" / "prediction.rank1.npy")
    assert np.array_equal(got, pred.numpy()[idx_a.astype(np.int64)])
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 4 * frame + 7 + 2 * 128 + 4 * 8   # + .npy headers
