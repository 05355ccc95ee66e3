"""Voxel-grid radiance field (MODEL_DICT['svox']), CPU tier: the torch restatement (tests/voxel_reference.py) against vectors the
reference's own helpers produced (tests/golden/ref_voxel_grid.npz, scripts/gen_golden_voxel_grid.py), the model's construction as
train.py builds it, its validation, and the C ABI symbols."""
import ctypes
import os

import numpy as np
import pytest
import torch

import voxel_reference as vr
from conftest import GOLDEN, ROOT

FIX = os.path.join(GOLDEN, "ref_voxel_grid.npz")
SVOX_KW = dict(scale=0.5, half_opt=False, sh_degree=2, grid_size=16, grid_radius=0.0125, origin_sh=0., origin_sigma=0.1)


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


@pytest.mark.parametrize("G", [16, 32])
def test_restatement_selects_the_reference_rows(fix, G):
    t = "g%d" % G
    assert np.array_equal(np.full(3, vr.grid_min(G, 0.0125), np.float32).view(np.uint32), fix[t + "_min"].view(np.uint32))
    x = torch.from_numpy(fix[t + "_x"])
    idx = vr.normalized_index(x, G, 0.0125).numpy()
    assert np.array_equal(idx.view(np.uint32), fix[t + "_idx"].view(np.uint32))
    rows = vr.rows(x, G, 0.0125).numpy()
    assert np.array_equal(rows, fix[t + "_row"])
    assert np.array_equal(rows >= 0, fix[t + "_mask"])
    # the fixture holds ties (index k + 0.5 exactly), rounded half to even, and points outside on every side
    fin = fix[t + "_idx"][np.isfinite(fix[t + "_idx"])]
    frac = np.abs(fin - np.floor(fin))
    assert (frac == 0.5).sum() > 20 and (~fix[t + "_mask"]).sum() > 40


@pytest.mark.parametrize("deg", range(5))
def test_restatement_eval_sh_matches_the_reference(fix, deg):
    D = (deg + 1)**2
    got = vr.eval_sh(deg, torch.from_numpy(fix["sh_coeffs"][..., :D]), torch.from_numpy(fix["sh_dirs"])).numpy()
    ref = fix["sh_deg%d" % deg]
    assert np.all(np.abs(got - ref) <= 1e-6 * np.maximum(np.abs(ref), 1.0)), np.abs(got - ref).max()


def test_model_dict_svox_builds_like_train_py():
    from modules.networks import MODEL_DICT, VoxelGrid
    m = MODEL_DICT['svox'](**SVOX_KW)
    assert isinstance(m, VoxelGrid)
    G, D = 16, 9
    assert m.sh_fields.shape == (G, G, G, 3 * D) and m.sh_fields.dtype == torch.float32
    assert m.density_fields.shape == (G, G, G, 1)
    assert bool((m.sh_fields == 0).all()) and bool((m.density_fields == np.float32(0.1)).all())
    assert m.cascades == 1 and m.grid_size == 16 and m.sh_dim == 9
    sd = m.state_dict()
    assert set(sd) == {"sh_fields", "density_fields", "center", "xyz_min", "xyz_max", "half_size", "density_bitfield", "density_grid",
                       "grid_coords"}
    assert sd["density_bitfield"].shape == (G**3 // 8,) and sd["density_bitfield"].dtype == torch.uint8
    assert sd["density_grid"].shape == (1, G**3) and sd["grid_coords"].shape == (G**3, 3) and sd["grid_coords"].dtype == torch.int32
    assert [p for p, _ in m.named_parameters()] == ["sh_fields", "density_fields"]
    assert m.fused_train_ok(torch.zeros(1, 3)) is False
    # cascades follow the scale as for NGP; the reference's initial field values
    assert VoxelGrid(**dict(SVOX_KW, scale=2.0)).cascades == 3
    assert float(m.grid_min) == float(vr.grid_min(16, 0.0125))


def test_state_dict_round_trip():
    from modules.networks import VoxelGrid
    a = VoxelGrid(**SVOX_KW)
    with torch.no_grad():
        a.sh_fields.normal_()
        a.density_fields.uniform_(-1, 1)
        a.density_grid.uniform_()
        a.density_bitfield.random_(0, 256)
    b = VoxelGrid(**SVOX_KW)
    b.load_state_dict(a.state_dict())
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k


@pytest.mark.parametrize("kw,match", [
    (dict(sh_degree=5), "sh_degree"), (dict(sh_degree=-1), "sh_degree"),
    (dict(grid_size=24), "power of two"), (dict(grid_size=8), "power of two"), (dict(grid_size=1024), "power of two"),
    (dict(grid_size=512, sh_degree=2), "2\\^31"), (dict(grid_radius=0.0), "grid_radius"),
])
def test_validation(kw, match):
    from modules.networks import VoxelGrid
    with pytest.raises(ValueError, match=match):
        VoxelGrid(**dict(SVOX_KW, **kw))


def test_half_opt_is_accepted_and_ignored():
    from modules.networks import VoxelGrid
    a = VoxelGrid(**dict(SVOX_KW, half_opt=True))
    assert a.sh_fields.dtype == torch.float32


def test_host_tensors_raise():
    from ngp_hip import ops
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.voxel_fwd(x, x, torch.zeros(16**3 * 27), torch.zeros(16**3), 16, 2, -0.0875, 0.0125)


def test_voxel_abi_symbols_exported(hip_lib):
    from ngp_hip import lib
    names = ["ngp_voxel_fwd", "ngp_voxel_density", "ngp_voxel_bwd", "ngp_voxel_occ_scratch_doubles", "ngp_voxel_occ_pack"]
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    experimental = open(os.path.join(ROOT, "include", "ngp_hip_experimental.h")).read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert n + "(" in header and n not in experimental
        assert n in lib.SIGNATURES
        getattr(so, n)
    assert so.ngp_voxel_occ_scratch_doubles() > 0
