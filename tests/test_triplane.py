"""Tri-plane position encoder (NGP(pos_encoder_type='triplane')), CPU tier: the numpy restatement (tests/triplane_reference.py) against
vectors the reference's own modules/triplane.py produced (tests/golden/ref_triplane.npz, scripts/gen_golden_triplane.py), and the
drop-in construction of the model."""
import json
import os

import numpy as np
import pytest

import triplane_reference as tr
from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "ref_triplane.npz")


def _golden_table(n):
    # oracle.gen_golden.golden_table, restated (the tests do not import the generator side)
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(2**32)
    return (h.astype(np.float64) / 2**32).astype(np.float32)


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


@pytest.mark.parametrize("max_res", [64, 1024])
def test_restatement_matches_the_reference(fix, max_res):
    t = "r%d" % max_res
    res = tr.resolutions(16, max_res, 8)
    assert res == fix[t + "_res"].tolist()
    table = _golden_table(int(fix[t + "_total_param_size"]))
    x, dout = fix[t + "_x"], fix[t + "_dout"]
    out = tr.forward(x, table, max_res, res)
    assert np.array_equal(out.view(np.uint32), fix[t + "_out"].view(np.uint32))
    idx, val, mag = tr.backward(x, dout, table, max_res, res)
    dense = np.zeros(table.size)
    dense[fix[t + "_grad_idx"]] = fix[t + "_grad_taichi"]
    tol = np.zeros(table.size)
    tol[idx] = 1e-6 * mag
    got = np.zeros(table.size)
    got[idx] = val
    assert np.all(np.abs(got - dense) <= tol), np.max(np.abs(got - dense) - tol)
    # the top-level collision is in the vectors: two corners of one lookup land on one entry (max_res 1024: grid points 0 and 1)
    if max_res == 1024:
        assert int(np.float32(1) / np.float32(1024) * np.float32(1023)) == 0


@pytest.mark.parametrize("max_res", [64, 1024])
def test_module_level_gradient_is_twice_the_true_one(fix, max_res):
    t = "r%d" % max_res
    assert np.array_equal(fix[t + "_grad_module"], 2 * fix[t + "_grad_taichi"])


def test_resolutions_of_the_driver_sizes():
    assert tr.resolutions(16, 1024, 8) == [16, 29, 53, 96, 173, 313, 566, 1024]
    assert tr.resolutions(16, 4096, 8) == [16, 36, 79, 173, 381, 841, 1855, 4096]


@pytest.mark.parametrize("max_res", [64, 1024, 4096])
def test_level_table_helper(hip_lib, max_res):
    from ngp_hip import ops
    lv = ops.make_triplane_levels(16, max_res, 8, 4)
    assert (lv.n_levels, lv.n_features, lv.max_res) == (8, 4, max_res)
    assert list(lv.resolution[:8]) == tr.resolutions(16, max_res, 8)


def test_ngp_triplane_constructs_like_the_reference(fix, hip_lib):
    from modules.networks import NGP
    m = NGP(scale=0.5, pos_encoder_type="triplane", max_res=1024)
    enc = m.pos_encoder
    assert enc.plane_embedding.numel() == 1024**2 * 3 * 4 == enc.total_param_size
    assert enc.out_dim == 32 and enc.levels == 8 and enc.feature_per_level == 4 and enc.base_res == 16 and enc.max_res == 1024
    assert enc.log_b == pytest.approx(float(fix["r1024_log_b"]), rel=0, abs=0)
    assert 0.0 <= float(enc.plane_embedding.min()) and float(enc.plane_embedding.max()) < 1.0
    shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert shapes == json.loads(str(fix["state_dict_json"]))
    assert m.use_fused_mlp                                       # out_dim 32: the MFMA shading kernels still apply
    with pytest.raises(ValueError):
        NGP(scale=0.5, pos_encoder_type="triplane", max_res=1024, table_dtype="bfloat16")
    with pytest.raises(NotImplementedError):
        NGP(scale=0.5, pos_encoder_type="voxels")


def test_triplane_model_takes_the_drop_in_path(hip_lib):
    import torch
    from modules.networks import NGP
    from ngp_hip.trainer import FusedTrainer
    m = NGP(scale=0.5, pos_encoder_type="triplane", max_res=64)
    assert not m.fused_train_ok(torch.zeros(1, 3))
    with pytest.raises(ValueError, match="drop-in"):
        FusedTrainer(m)


def test_ops_refuse_cpu_tensors(hip_lib):
    import torch
    from ngp_hip import ops
    lv = ops.make_triplane_levels(16, 64, 8, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.triplane_fwd(torch.zeros(4, 3), torch.zeros(3 * 64 * 64 * 4), lv)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.triplane_bwd(torch.zeros(4, 3), torch.zeros(4, 32), torch.zeros(3 * 64 * 64 * 4), lv, torch.zeros(3 * 64 * 64 * 4))
