"""tests/ray_grad_reference.py against torch float64 autograd of the geometry it models (xyz = o + t d, dirs = d, rays_d = R dir,
rays_o = t); that the yardstick is meetable by the kernels' summation order (and not by a broken one); ngp_hip.poses.PoseRefiner
against torch.matrix_exp in float64; the wiring of the three entry points into the header, the binding and the source list.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import ray_grad_reference as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("permute", [False, True])
def test_march_reference_is_the_adjoint(permute):
    inp = rg.ray_input(permute=permute)
    ra = torch.from_numpy(inp["rays_a"].astype(np.int64))
    n = inp["n"]
    o = torch.zeros(n, 3, dtype=torch.float64, requires_grad=True)
    d = torch.zeros(n, 3, dtype=torch.float64, requires_grad=True)
    ray_of = torch.zeros(inp["S"], dtype=torch.int64)
    live = torch.zeros(inp["S"], dtype=torch.bool)
    for r, s, c in ra.tolist():
        ray_of[s:s + c] = r
        live[s:s + c] = True
    t = torch.from_numpy(np.nan_to_num(inp["ts"]).astype(np.float64))
    xyzs = o[ray_of] + t[:, None] * d[ray_of]
    dirs = d[ray_of]
    gx, gd = torch.from_numpy(inp["d_xyzs"].astype(np.float64)), torch.from_numpy(inp["d_dirs"].astype(np.float64))
    ((xyzs * gx + dirs * gd) * live[:, None]).sum().backward()
    do, dd, So, Sd = rg.march_bwd_64(inp)
    np.testing.assert_allclose(do, o.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(dd, d.grad.numpy(), rtol=0, atol=1e-12)
    assert np.all(So >= np.abs(do) - 1e-12) and np.all(Sd >= np.abs(dd) - 1e-12)
    empty = inp["rays_a"][inp["rays_a"][:, 2] == 0, 0]
    assert len(empty) == 1 and np.all(do[empty] == 0) and np.all(Sd[empty] == 0)


@pytest.mark.parametrize("form", ["both", "img_null", "pix_null"])
def test_pose_reference_is_the_adjoint(form):
    inp = rg.pose_input(1000, 3)
    kw = dict(img_null=2 if form == "img_null" else None, pix_null=form == "pix_null")
    poses = torch.randn(3, 3, 4, dtype=torch.float64, requires_grad=True)
    img = torch.full((1000,), 2, dtype=torch.int64) if form == "img_null" else torch.from_numpy(inp["img"])
    pix = torch.arange(1000) if form == "pix_null" else torch.from_numpy(inp["pix"])
    dirs = torch.from_numpy(inp["directions"].astype(np.float64))[pix]
    rays_d = torch.einsum("krc,kc->kr", poses[img][:, :, :3], dirs)
    rays_o = poses[img][:, :, 3]
    (rays_d * torch.from_numpy(inp["g_d"].astype(np.float64)) + rays_o * torch.from_numpy(inp["g_o"].astype(np.float64))).sum().backward()
    ref, S = rg.pose_bwd_64(inp, **kw)
    np.testing.assert_allclose(ref, poses.grad.numpy(), rtol=0, atol=1e-11)
    assert np.all(ref[1] == 0) and np.all(S[1] == 0)                       # image 1 has no ray


def test_yardstick_is_meetable_and_catches_a_lost_term():
    """The kernels' order stays within K E32 S on the GPU test's inputs; dropping one sample of one ray, or one ray of one image, does
    not."""
    worst = {}
    for permute in (False, True):
        inp = rg.ray_input(permute=permute)
        do, dd, So, Sd = rg.march_bwd_64(inp)
        so, sd = rg.march_bwd_serial32(inp)
        wo, wd = rg.march_bwd_wave32(inp)
        Eo, Ed = rg.e32(so, do, So), rg.e32(sd, dd, Sd)
        assert 1e-8 < Eo < 1e-6 and 1e-8 < Ed < 1e-6
        assert rg.within(wo, do, So, Eo) and rg.within(wd, dd, Sd, Ed)
        worst["rays_o"] = max(worst.get("rays_o", 0), rg.worst_ratio(wo, do, So, Eo))
        worst["rays_d"] = max(worst.get("rays_d", 0), rg.worst_ratio(wd, dd, Sd, Ed))
        bad = dict(inp, rays_a=inp["rays_a"].copy())
        row = int(np.argmax(bad["rays_a"][:, 2] == 500))
        bad["rays_a"][row, 2] -= 1                                           # the last sample of the 500-sample ray is lost
        bo, _ = rg.march_bwd_wave32(bad)
        assert not rg.within(bo, do, So, Eo)
    for n, n_img in ((8192, 100), (1000, 3), (65, 1)):
        inp = rg.pose_input(n, n_img)
        ref, S = rg.pose_bwd_64(inp)
        E = rg.e32(rg.pose_bwd_serial32(inp), ref, S)
        w = rg.pose_bwd_wave32(inp)
        assert rg.within(w, ref, S, E)
        worst["poses"] = max(worst.get("poses", 0), rg.worst_ratio(w, ref, S, E))
        bad = dict(inp, g_d=inp["g_d"].copy())
        bad["g_d"][0] = 0                                                    # ray 0 does not reach its pose
        assert not rg.within(rg.pose_bwd_wave32(bad), ref, S, E)
    print("kernel-order emulation, worst |. - f64| / (E32 S):", {k: round(v, 3) for k, v in worst.items()}, "(bound %d)" % rg.K)
    assert max(worst.values()) <= rg.K


# ------------------------------------------------------------------------------------------------------------------ PoseRefiner
def _skew(w):
    z = torch.zeros_like(w[:, 0])
    return torch.stack([z, -w[:, 2], w[:, 1], w[:, 2], z, -w[:, 0], -w[:, 1], w[:, 0], z], -1).view(-1, 3, 3)


def _poses(n, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    return torch.cat([q, torch.randn(n, 3, 1, generator=g, dtype=torch.float64)], 2).to(dtype)


@pytest.mark.parametrize("angle", [0.0, 1e-5, 1e-2, 0.09, 0.11, 1.0])
def test_pose_refiner_matches_matrix_exp(angle):
    """Value and gradient (of a fixed random linear functional of the output) in float64, on both sides of the small-angle switch."""
    from ngp_hip.poses import PoseRefiner
    n = 5
    g = torch.Generator().manual_seed(3)
    axis = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=1)
    dT0 = 0.1 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    probe = torch.randn(n, 3, 4, generator=g, dtype=torch.float64)
    poses = _poses(n, torch.float64)
    ref_w = (angle * axis).clone().requires_grad_(True)
    ref_t = dT0.clone().requires_grad_(True)
    ref = torch.cat([torch.matrix_exp(_skew(ref_w)) @ poses[:, :, :3], poses[:, :, 3:] + ref_t[:, :, None]], 2)
    (ref * probe).sum().backward()
    m = PoseRefiner(n).double()
    with torch.no_grad():
        m.dR.copy_(angle * axis); m.dT.copy_(dT0)
    out = m(poses)
    (out * probe).sum().backward()
    assert torch.isfinite(m.dR.grad).all() and torch.isfinite(m.dT.grad).all()
    np.testing.assert_allclose(out.detach().numpy(), ref.detach().numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(m.dR.grad.numpy(), ref_w.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.dT.grad.numpy(), ref_t.grad.numpy(), rtol=0, atol=0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pose_refiner_is_the_identity_at_zero(dtype):
    from ngp_hip.poses import PoseRefiner
    poses = _poses(7, dtype, seed=1)
    poses[0, 0, 0], poses[1, 2, 3], poses[2, 1, 1] = -0.0, -0.0, 0.0          # signed zeros survive too
    m = PoseRefiner(7)
    out = m(poses)
    view = torch.int32 if dtype == torch.float32 else torch.int64
    assert out.dtype == dtype and torch.equal(out.view(view), poses.view(view))
    out.sum().backward()
    assert torch.isfinite(m.dR.grad).all() and m.dR.grad.abs().max() > 0      # the generators, not a dead zero
    assert torch.equal(m.dT.grad, torch.ones(7, 3))
    with pytest.raises(ValueError):
        m(poses[:3])


# ------------------------------------------------------------------------------------------------------------------ wiring
def test_entry_points_are_declared_bound_and_built():
    from ngp_hip import lib
    hdr = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    assert "#define NGP_ABI_VERSION 3" in hdr
    for name, n_args in (("ngp_march_train_bwd", 8), ("ngp_sample_rays_bwd", 10), ("ngp_get_rays_bwd", 6)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
        assert name in lib.SIGNATURES and name not in lib.EXPERIMENTAL and len(lib.SIGNATURES[name]) == n_args
    assert "ray_grad.hip" in lib.SOURCES and os.path.exists(os.path.join(lib.CSRC, "ray_grad.hip"))


def test_operators_refuse_cpu_tensors():
    from ngp_hip import ops
    from ngp_hip.rays import get_rays
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.march_train_bwd(z, None, torch.zeros(4), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sample_rays_bwd(z, None, 0, None, z, z, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.get_rays_bwd(z, z, z)
    with pytest.raises(RuntimeError, match="GPU"):
        get_rays(z, torch.zeros(3, 4, requires_grad=True))
