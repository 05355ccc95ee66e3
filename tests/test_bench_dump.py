"""bench.py --dump-outputs, host side: what a training step returned is brought to the host in a fixed layout (per-ray arrays,
marched samples per ray in ray order whatever order the march packed the rays in) and written as float32 / float64 .npy files,
large arrays as a fixed seeded sample."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_dump", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model(n_table):
    w = [torch.arange(6, dtype=torch.float32).view(2, 3), torch.ones(4, dtype=torch.float16)]
    return SimpleNamespace(pos_encoder=SimpleNamespace(hash_table=torch.linspace(0, 1, n_table)), _mlp_weights=lambda: w)


def test_capture_keeps_fixed_shapes_in_ray_order():
    b = _bench()
    # three rays packed in the order 2, 0, 1 (ray 1 has no sample); the arena holds one unused slot at its end
    rays_a = torch.tensor([[2, 0, 2], [0, 2, 3], [1, 5, 0]], dtype=torch.int32)
    ts = torch.tensor([20., 21., 0., 1., 2., -1.])
    res = {"rays_a": rays_a, "ts": ts, "deltas": ts * 10, "rgb": torch.rand(3, 3, dtype=torch.float16),
           "rm_samples": torch.tensor([5], dtype=torch.int32), "vr_per_ray": torch.tensor([3, 0, 1], dtype=torch.int32)}
    out = b.capture_outputs(res, _model(16), 0.25)
    assert "ts" not in out and "deltas" not in out                         # (their length varies between runs)
    assert out["samples_per_ray"].tolist() == [3., 0., 2.]
    assert out["rm_samples"].dtype == np.float64 and out["rm_samples"].tolist() == [5.]
    assert out["vr_per_ray"].dtype == np.float64 and out["rgb"].dtype == np.float32 and out["rgb"].shape == (3, 3)
    assert out["loss"].tolist() == [0.25] and out["hash_table"].shape == (16,)
    assert out["mlp_weights"].tolist() == [0., 1., 2., 3., 4., 5., 1., 1., 1., 1.]


def test_dump_writes_float_files_and_samples_large_arrays(tmp_path):
    b = _bench()
    n = b.DUMP_SAMPLE + 1000
    out = b.capture_outputs({"rgb": torch.zeros(4, 3)}, _model(n), 1.0)
    b.dump_outputs(str(tmp_path / "a"), out)
    b.dump_outputs(str(tmp_path / "b"), out)
    got = {f: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert set(got) == {"rgb.npy", "loss.npy", "hash_table.npy", "mlp_weights.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    t = got["hash_table.npy"]
    assert t.shape == (b.DUMP_SAMPLE,) and np.all(np.diff(t) > 0)          # a sample of distinct positions, ascending
    assert np.array_equal(t, np.load(str(tmp_path / "b" / "hash_table.npy")))  # the same positions in every run
    assert sum(a.nbytes for a in got.values()) <= b.DUMP_LIMIT_BYTES


def test_dump_over_the_limit_writes_nothing(tmp_path):
    import pytest
    b = _bench()
    b.DUMP_LIMIT_BYTES = 1000
    with pytest.raises(SystemExit):
        b.dump_outputs(str(tmp_path / "c"), {"small": np.zeros(10, np.float32), "big": np.zeros(1000, np.float32)})
    assert not (tmp_path / "c").exists()
