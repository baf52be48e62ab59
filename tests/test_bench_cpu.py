"""CPU test of bench.py's --dump-outputs writer (the GPU suite runs the whole command): at the headline workload
(4096x4096, 1 000 000 Gaussians) the files stay within 64 MB, are float32 / float64, and a sampled array keeps the same
rows in every run."""
import importlib
import os

import numpy as np

import bench

S2D = importlib.import_module("2dgaussiansplatting_amd")


class _Trainer:
    """What dump_outputs reads from a trainer, filled with values that name their own row."""
    def __init__(self, W, H, n):
        self.W, self.H, self.n = W, H, n

    def get_splats(self):
        a = np.zeros(self.n, dtype=S2D.SPLAT_DTYPE)
        a.view(np.float32).reshape(self.n, 9)[:] = np.arange(self.n, dtype=np.float32)[:, None]
        return a

    def get_adam(self):
        a = np.zeros(self.n, dtype=S2D.ADAM_DTYPE)
        a.view(np.float32).reshape(self.n, 18)[:] = np.arange(self.n, dtype=np.float32)[:, None]
        return a, np.float32(0.5), np.float32(0.25), 3

    def get_image_rows(self):
        return np.broadcast_to(np.arange(self.W * self.H, dtype=np.float32).reshape(self.H, self.W, 1), (self.H, self.W, 4)).copy()


def test_dump_outputs_stays_within_64_mb_and_samples_the_same_rows(tmp_path):
    t = _Trainer(4096, 4096, 1_000_000)
    mse = np.linspace(900.0, 800.0, 100)
    files = {}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), t, mse)
        files[run] = {f: np.load(tmp_path / run / f) for f in sorted(os.listdir(tmp_path / run))}
    assert sorted(files["a"]) == ["adam.npy", "image.npy", "mse.npy", "splats.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files["a"]) <= 64e6
    for f, a in files["a"].items():
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        assert np.array_equal(a, files["b"][f]), f
    assert np.array_equal(files["a"]["mse.npy"], mse)
    assert files["a"]["splats.npy"].shape == (1_000_000, 9)
    for f, width in (("adam.npy", 18), ("image.npy", 4)):
        a = files["a"][f]
        assert a.shape[1] == width and 0 < len(a) < 1_000_000
        rows = a[:, 0]
        assert (np.diff(rows) > 0).all() and (a == rows[:, None]).all()   # distinct rows, ascending, each kept whole
