"""Ray and camera-pose gradients on the GPU: the kernels of csrc/ray_grad.hip element by element against the float64 model of
tests/ray_grad_reference.py; the wiring RayBatcher.sample(poses=PoseRefiner(..)) -> render -> loss.backward() against a float64 torch
evaluation of the same loss; the NGP fast path (fused MFMA shading + the hash position gradient); a closed-loop registration of
perturbed cameras against a known field; the example.  Every test prints the figures it measured (pytest -s);
profiles/pose_refine.json records them."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import ray_grad_reference as rg

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 1e-4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent(*shape):
    return torch.full(shape, rg.SENTINEL, device=DEV, dtype=torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def _ptr(t):
    from ngp_hip import ops
    return ops._ptr(t)


# ------------------------------------------------------------------------------------------------------------------ 1. kernels
def _march_launch(L, inp, with_x, with_d):
    from ngp_hip import ops
    n = inp["n"]
    o, d = sent(n + 1, 3), sent(n + 1, 3)                        # one row behind the last stays a sentinel
    gx, gd = dev(inp["d_xyzs"]) if with_x else None, dev(inp["d_dirs"]) if with_d else None       # (held until the launch is done)
    ts, ra = dev(inp["ts"]), dev(inp["rays_a"])
    rc = L.ngp_march_train_bwd(_ptr(gx), _ptr(gd), _ptr(ts), _ptr(ra), n, _ptr(o), _ptr(d), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((o[n] == rg.SENTINEL).all()) and bool((d[n] == rg.SENTINEL).all())
    return o[:n], d[:n]


@pytest.mark.parametrize("form", ["both", "no_dirs", "no_xyzs", "permuted"])
def test_march_train_bwd_against_float64(hip_lib, form):
    inp = rg.ray_input(permute=form == "permuted")
    ra = inp["rays_a"]
    assert ra.min() >= 0 and ra[:, 0].max() < inp["n"] and (ra[:, 1] + ra[:, 2]).max() <= inp["S"]     # every index inside its buffer
    assert sorted(ra[:, 0].tolist()) == list(range(inp["n"]))
    with_x, with_d = form != "no_xyzs", form != "no_dirs"
    model = dict(inp, d_xyzs=inp["d_xyzs"] if with_x else None, d_dirs=inp["d_dirs"] if with_d else None)
    do, dd, So, Sd = rg.march_bwd_64(model)
    so, sd = rg.march_bwd_serial32(model)
    o, d = _march_launch(hip_lib, inp, with_x, with_d)
    o2, d2 = _march_launch(hip_lib, inp, with_x, with_d)
    assert torch.equal(bits(o), bits(o2)) and torch.equal(bits(d), bits(d2)), "two launches differ"
    o, d = o.cpu().numpy(), d.cpu().numpy()
    empty = ra[ra[:, 2] == 0, 0]
    assert np.all(o[empty] == 0) and np.all(d[empty] == 0)
    if not with_x:
        assert np.all(o == 0)
    worst = {}
    for name, got, ref, S, ser in (("d_rays_o", o, do, So, so), ("d_rays_d", d, dd, Sd, sd)):
        if not S.any():
            continue
        E = rg.e32(ser, ref, S)
        worst[name] = (round(rg.worst_ratio(got, ref, S, E), 3), E)
    print("march_train_bwd %s: worst |gpu - f64| / (E32 S), E32: %s (bound %d)" % (form, worst, rg.K))
    for name, got, ref, S, ser in (("d_rays_o", o, do, So, so), ("d_rays_d", d, dd, Sd, sd)):
        assert rg.within(got, ref, S, rg.e32(ser, ref, S)), name


def test_march_train_bwd_keeps_a_nan_inside_its_ray(hip_lib):
    inp = rg.ray_input()
    row = int(np.argmax(inp["rays_a"][:, 2] == 129))
    ray, start = int(inp["rays_a"][row, 0]), int(inp["rays_a"][row, 1])
    clean_o, clean_d = _march_launch(hip_lib, inp, True, True)
    bad = dict(inp, d_xyzs=inp["d_xyzs"].copy())
    bad["d_xyzs"][start + 70, 1] = np.nan
    o, d = _march_launch(hip_lib, bad, True, True)
    assert bool(torch.isnan(o[ray, 1])) and bool(torch.isnan(d[ray, 1]))
    keep = torch.ones(inp["n"], dtype=torch.bool, device=DEV)
    keep[ray] = False
    assert torch.equal(bits(o[keep]), bits(clean_o[keep])) and torch.equal(bits(d[keep]), bits(clean_d[keep]))


def _pose_launch(L, inp, img_null, pix_null, g_o=True, g_d=True):
    from ngp_hip import ops
    n_img = inp["n_img"]
    out = sent(n_img + 1, 3, 4)
    dirs, img, pix = dev(inp["directions"]), None if img_null is not None else dev(inp["img"]), None if pix_null else dev(inp["pix"])
    go, gd = dev(inp["g_o"]) if g_o else None, dev(inp["g_d"]) if g_d else None                  # (held until the launch is done)
    rc = L.ngp_sample_rays_bwd(_ptr(dirs), _ptr(img), 0 if img_null is None else img_null, _ptr(pix), _ptr(go), _ptr(gd), inp["n"],
                               n_img, _ptr(out), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out[n_img] == rg.SENTINEL).all())
    return out[:n_img]


@pytest.mark.parametrize("n_img", [1, 3, 100])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 8192])
def test_sample_rays_bwd_against_float64(hip_lib, n, n_img):
    inp = rg.pose_input(n, n_img)
    assert inp["pix"].max() < len(inp["directions"]) and inp["img"].min() >= 0 and inp["img"].max() < n_img
    worst = {}
    for form, img_null, pix_null in (("indexed", None, False), ("img_idx=NULL", n_img - 1, False), ("pix_idx=NULL", None, True)):
        ref, S = rg.pose_bwd_64(inp, img_null, pix_null)
        E = rg.e32(rg.pose_bwd_serial32(inp, img_null, pix_null), ref, S)
        got = _pose_launch(hip_lib, inp, img_null, pix_null)
        assert torch.equal(bits(got), bits(_pose_launch(hip_lib, inp, img_null, pix_null))), "two launches differ"
        got = got.cpu().numpy()
        if n_img == 3 and img_null is None:
            assert np.all(got[1] == 0)                                      # the image without rays: written, exact zeros
        worst[form] = round(rg.worst_ratio(got, ref, S, E), 3)
        assert rg.within(got, ref, S, E), form
    print("sample_rays_bwd n=%d n_img=%d: worst |gpu - f64| / (E32 S): %s (bound %d)" % (n, n_img, worst, rg.K))


def test_sample_rays_bwd_skips_foreign_images_and_null_gradients(hip_lib):
    inp = rg.pose_input(1000, 3)
    ref, S = rg.pose_bwd_64(inp)
    E = rg.e32(rg.pose_bwd_serial32(inp), ref, S)
    stray = dict(inp, img=inp["img"].copy())
    moved = np.arange(0, 1000, 7)
    stray["img"][moved[::2]], stray["img"][moved[1::2]] = -1, 3             # outside [0, n_img): skipped, nothing outside d_poses written
    ref_s, S_s = rg.pose_bwd_64(stray)
    assert rg.within(_pose_launch(hip_lib, stray, None, False).cpu().numpy(), ref_s, S_s, E)
    only_o = _pose_launch(hip_lib, inp, None, False, g_d=False).cpu().numpy()
    assert np.all(only_o[:, :, :3] == 0) and rg.within(only_o[:, :, 3], ref[:, :, 3], S[:, :, 3], E)
    only_d = _pose_launch(hip_lib, inp, None, False, g_o=False).cpu().numpy()
    assert np.all(only_d[:, :, 3] == 0) and rg.within(only_d[:, :, :3], ref[:, :, :3], S[:, :, :3], E)


def test_get_rays_backward_both_forms(hip_lib):
    """get_rays is differentiable in c2w: [N,3,4] through ngp_get_rays_bwd (elementwise, exact to one rounding), [3,4] through
    ngp_sample_rays_bwd over one image."""
    from ngp_hip.rays import get_rays
    inp = rg.pose_input(1000, 1)
    dirs = dev(inp["directions"][:1000])
    g_o, g_d = dev(inp["g_o"]), dev(inp["g_d"])
    per_ray = torch.randn(1000, 3, 4, device=DEV, requires_grad=True)
    o, d = get_rays(dirs, per_ray)
    o_plain, d_plain = get_rays(dirs, per_ray.detach())
    assert torch.equal(o, o_plain) and torch.equal(d, d_plain) and not o_plain.requires_grad
    ((o * g_o).sum() + (d * g_d).sum()).backward()
    want = torch.cat([g_d[:, :, None] * dirs[:, None, :], g_o[:, :, None]], 2)
    assert torch.equal(bits(per_ray.grad), bits(want))
    one = torch.randn(4, 4, device=DEV, requires_grad=True)                # homogeneous form: the last row gets a zero gradient
    o, d = get_rays(dirs, one)
    ((o * g_o).sum() + (d * g_d).sum()).backward()
    ref, S = rg.pose_bwd_64(inp, img_null=0, pix_null=True)
    E = rg.e32(rg.pose_bwd_serial32(inp, img_null=0, pix_null=True), ref, S)
    got = one.grad.cpu().numpy()
    assert np.all(got[3] == 0) and rg.within(got[None, :3], ref, S, E)


# ------------------------------------------------------------------------------------------------------------------ the analytic field
CENTRES = ((0.12, 0.05, -0.1), (-0.15, 0.1, 0.08), (0.02, -0.16, 0.12))
WIDTHS = (0.09, 0.07, 0.08)
COLOURS = ((0.9, 0.2, 0.1), (0.1, 0.8, 0.3), (0.2, 0.3, 0.9))


class BlobField:
    """Three Gaussian blobs: sigma = amp sum_k exp(-r_k^2 / 2 s_k^2), colour = the blob-weighted mean of three colours times
    0.8 + 0.2 sin(25 (x + y + z)), and, when view_dep, times 0.75 + 0.25 cos(angle between d and a fixed axis)."""

    def __init__(self, amp, view_dep, device, dtype):
        kw = dict(device=device, dtype=dtype)
        self.c, self.s, self.col = torch.tensor(CENTRES, **kw), torch.tensor(WIDTHS, **kw), torch.tensor(COLOURS, **kw)
        self.axis = Fn.normalize(torch.tensor((0.3, -0.5, 0.8), **kw), dim=0)
        self.amp, self.view_dep = amp, view_dep

    def __call__(self, x, d):
        g = torch.exp(-((x[:, None, :] - self.c[None])**2).sum(-1) / (2 * self.s**2))
        rgb = (g[:, :, None] * self.col[None]).sum(1) / (g.sum(1, keepdim=True) + 1e-3)
        rgb = rgb * (0.8 + 0.2 * torch.sin(25 * x.sum(1, keepdim=True)))
        if self.view_dep:
            rgb = rgb * (0.75 + 0.25 * (d / d.norm(dim=1, keepdim=True)) @ self.axis)[:, None]
        return self.amp * g.sum(1), rgb


class FieldModel:
    """What render() needs of a model: the occupancy attributes of one all-ones cascade, render_func, and a callable."""

    def __init__(self, amp, view_dep):
        from modules.volume_train import VolumeRenderer
        self.scale, self.cascades, self.grid_size = 0.5, 1, 128
        self.density_bitfield = torch.full((128**3 // 8,), 255, device=DEV, dtype=torch.uint8)
        self.render_func = VolumeRenderer()
        self.field = BlobField(amp, view_dep, DEV, torch.float32)

    def __call__(self, x, d):
        return self.field(x, d)


def _example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_procedural
    finally:
        sys.path.pop(0)
    return train_procedural


def _cameras(wh=32):
    ex = _example()
    return ex.cameras(6, 1.39, 23, DEV), ex.pixel_dirs(wh, 1111.1 * wh / 800, DEV)


def _perturbed(poses, deg, shift, seed):
    """poses with a rotation of `deg` degrees and a translation of `shift` applied along seeded random axes."""
    from ngp_hip.poses import axis_angle_delta
    g = torch.Generator().manual_seed(seed)
    n = poses.shape[0]
    w = Fn.normalize(torch.randn(n, 3, generator=g), dim=1).to(poses) * math.radians(deg)
    dt = Fn.normalize(torch.randn(n, 3, generator=g), dim=1).to(poses) * shift
    R = (torch.eye(3, device=poses.device) + axis_angle_delta(w)) @ poses[:, :, :3]
    return torch.cat([R, poses[:, :, 3:] + dt[:, :, None]], 2)


def _pose_errors(est, true):
    """mean rotation angle of R_est R_true^T in degrees, mean |t_est - t_true|."""
    rel = est[:, :, :3] @ true[:, :, :3].transpose(1, 2)
    cos = ((rel.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1)
    return float(torch.rad2deg(torch.acos(cos.double())).mean()), float((est[:, :, 3] - true[:, :, 3]).norm(dim=1).mean())


# ------------------------------------------------------------------------------------------------------------------ 2. wiring
def _reference_pose_grads(dtype, poses, dR, dT, directions, img, pix, target, ts, deltas, rays_a, amp):
    """The loss of the GPU run recomputed on the CPU in `dtype` torch -- its ts, deltas and rays_a, the compositing contract of
    tests/composite_reference.py (stop at the first !(T > thr), w = a T, white background) -- differentiated to dR, dT.
    -> dR.grad, dT.grad, the smallest transmittance any sample (or ray end) sees."""
    from ngp_hip.poses import PoseRefiner
    n = poses.shape[0]
    ref = PoseRefiner(n).to(dtype)
    with torch.no_grad():
        ref.dR.copy_(dR); ref.dT.copy_(dT)
    P = ref(poses.to(dtype))[img]
    rays_d = torch.einsum("krc,kc->kr", P[:, :, :3], directions.to(dtype)[pix])
    rays_o = P[:, :, 3]
    ra = rays_a.long()
    n_rays, L = ra.shape[0], int(ra[:, 2].max())
    j = torch.arange(L)[None, :]
    valid = j < ra[:, 2:3]
    idx = torch.where(valid, ra[:, 1:2] + j, torch.zeros_like(j))                               # [rows, L] sample of (row, j)
    ray = ra[:, 0]
    t, dl = ts.to(dtype)[idx], deltas.to(dtype)[idx]
    x = rays_o[ray][:, None, :] + t[..., None] * rays_d[ray][:, None, :]
    d = rays_d[ray][:, None, :].expand_as(x)
    sigma, rgb = BlobField(amp, True, "cpu", dtype)(x.reshape(-1, 3), d.reshape(-1, 3))
    a = torch.where(valid, 1 - torch.exp(-sigma.view(n_rays, L) * dl), torch.zeros_like(dl))
    T_after = torch.cumprod(1 - a, 1)
    T = torch.cat([torch.ones_like(T_after[:, :1]), T_after[:, :-1]], 1)
    live = torch.cumprod((valid & (T > THR)).to(dtype), 1)                                      # a prefix, like the serial loop
    w = a * T * live
    colour = (w[..., None] * rgb.view(n_rays, L, 3)).sum(1)
    out = torch.zeros(n_rays, 3, dtype=dtype)
    out[ray] = colour + (1 - w.sum(1))[:, None]
    Fn.mse_loss(out, target.to(dtype)).backward()
    return ref.dR.grad, ref.dT.grad, float(T_after.detach().min())


def test_pose_gradient_through_render_against_float64(hip_lib):
    """64 rays of RayBatcher.sample(poses=PoseRefiner(..)(poses)) through render (no autocast), an MSE loss, backward; the gradient
    (dR, dT) against the same loss in float64 torch on the CPU: |gpu - ref64|_inf <= 4 |ref32 - ref64|_inf over the whole gradient.

    Measured on the MI355X: |gpu - ref64| 1.03e-6, |ref32 - ref64| 2.91e-7, ratio 3.54 (gradient entries up to 0.17).  By block: dR
    9.7e-7 / 2.9e-7 = 3.3, dT 1.03e-6 / 2.4e-7 = 4.3.  Nearly all of it is the float32 composite's a = 1 - exp(-sigma delta) at
    sigma delta <= 0.03, whose absolute error is an ulp of 1 and not of a: with the composite (only) evaluated in float64 torch on the
    GPU the ratios are 0.7 (dR) and 0.5 (dT), and with torch's own float32 composite on the GPU in place of composite.hip they are 3.5
    and 4.5 -- the device's expf against the CPU's, not a summation order.  The ray, march-adjoint and pose-adjoint kernels sit inside
    the 0.5 - 0.7."""
    from modules.rendering import render
    from ngp_hip.poses import PoseRefiner
    from ngp_hip.rays import RayBatcher
    amp = 6.0                                     # optical depth <= amp sqrt(2 pi) sum(widths) = 3.6: T >= 0.027 on every ray
    poses, dirs = _cameras()
    g = torch.Generator().manual_seed(5)
    images = torch.rand(6, dirs.shape[0], 3, generator=g).to(DEV)
    model = FieldModel(amp, view_dep=True)
    refiner = PoseRefiner(6).to(DEV)
    with torch.no_grad():
        refiner.dR.copy_(0.02 * torch.randn(6, 3, generator=g)); refiner.dT.copy_(0.01 * torch.randn(6, 3, generator=g))
    batcher = RayBatcher(images, poses, dirs, batch_size=64)
    torch.manual_seed(77)
    batch = batcher.sample(poses=refiner(batcher.poses))
    assert batch["rays_o"].requires_grad and batch["rays_d"].requires_grad and not batch["rgb"].requires_grad
    res = render(model, batch["rays_o"], batch["rays_d"], exp_step_factor=0.0, T_threshold=THR)
    Fn.mse_loss(res["rgb"], batch["rgb"]).backward()
    assert int(res["rm_samples"]) > 64 * 100
    cpu = lambda t: t.detach().cpu()
    args = (cpu(poses), cpu(refiner.dR), cpu(refiner.dT), cpu(dirs), cpu(batch["img_idxs"]), cpu(batch["pix_idxs"]), cpu(batch["rgb"]),
            cpu(res["ts"]), cpu(res["deltas"]), cpu(res["rays_a"]), amp)
    r64, t64, t_min = _reference_pose_grads(torch.float64, *args)
    r32, t32, _ = _reference_pose_grads(torch.float32, *args)
    assert t_min > 100 * THR, "the live counts are not decided: a transmittance of %g" % t_min
    assert float(r64.abs().max()) > 0 and float(t64.abs().max()) > 0
    got, ref64, ref32 = (torch.cat([a.double(), b.double()]) for a, b in ((cpu(refiner.dR.grad), cpu(refiner.dT.grad)), (r64, t64), (r32, t32)))
    err, unit = (got - ref64).abs().amax(1), (ref32 - ref64).abs().amax(1)                      # per row: 6 of dR, then 6 of dT
    print("pose gradient through render: |gpu - ref64| %.3g, |ref32 - ref64| %.3g, ratio %.3f (bound 4); dR alone %.3f, dT alone %.3f; "
          "min T %.3g" % (float(err.max()), float(unit.max()), float(err.max() / unit.max()), float(err[:6].max() / unit[:6].max()),
                          float(err[6:].max() / unit[6:].max()), t_min))
    assert float(err.max()) <= 4 * float(unit.max())


# ------------------------------------------------------------------------------------------------------------------ 3. NGP fast path
def _ngp(lego_bitfield, n=2048):
    from modules.networks import NGP
    from ngp_hip import synthetic
    torch.manual_seed(0)
    m = NGP(scale=0.5, max_res=1024).cuda()
    m.density_bitfield.copy_(torch.from_numpy(lego_bitfield).cuda())
    with torch.no_grad():
        m.pos_encoder.hash_table.mul_(0.2)          # keep exp(h0) moderate so rays are neither empty nor saturated
    o, d = synthetic.lego_rays(n, seed=3)
    return m, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.rand(n, 3, device="cuda")


def _clear(m):
    for p in m.parameters():
        p.grad = None


def test_ngp_fast_path_ray_gradients(hip_lib, lego_bitfield, monkeypatch):
    from modules.intersection import ray_aabb_intersection
    from modules.ray_march import raymarching_train
    from modules.rendering import MAX_SAMPLES, TrainResults, render
    from ngp_hip import ops
    m, o, d, target = _ngp(lego_bitfield)

    def run(o, d):
        _clear(m)
        torch.manual_seed(123)
        with torch.autocast("cuda", dtype=torch.float16):
            res = render(m, o, d, exp_step_factor=0.0)
            loss = Fn.mse_loss(res["rgb"], target)
        (loss * 1024.0).backward()
        return res, m.pos_encoder.hash_table.grad.clone()

    og, dg = o.clone().requires_grad_(), d.clone().requires_grad_()
    res, table_grad = run(og, dg)
    assert not isinstance(res, TrainResults) and int(res["rm_samples"]) > 0
    for g in (og.grad, dg.grad):
        assert g.shape == (o.shape[0], 3) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0

    # the same render by hand: march, xyzs as a leaf, shade, composite; its d_xyzs through the operator gives the same bits
    _clear(m)
    torch.manual_seed(123)
    hits_t = ray_aabb_intersection(o, d, m.scale)
    rays_a, xyzs, dirs, deltas, ts, _ = raymarching_train(o, d, hits_t, m.density_bitfield, m.cascades, m.scale, 0.0, m.grid_size,
                                                          MAX_SAMPLES)
    assert torch.equal(rays_a, res["rays_a"]) and torch.equal(ts, res["ts"])
    xyzs.requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        sigmas, rgbs = m(xyzs, dirs)
        _, opacity, _, rgb, _ = m.render_func(sigmas, rgbs, deltas, ts, rays_a, THR)
        loss = Fn.mse_loss(rgb + (1 - opacity)[:, None], target)
    (loss * 1024.0).backward()
    d_o, d_d = ops.march_train_bwd(xyzs.grad, None, ts, rays_a)
    assert torch.equal(bits(d_o), bits(og.grad)) and torch.equal(bits(d_d), bits(dg.grad))

    # the table gradient is the one of the composable path without a ray gradient.  Both scatter the same d_enc; the scatter-add's
    # default plan meets its coarse-level replicas with float atomics, so two runs of it agree to a summation order: 2^-17 of the
    # largest entry (128 ulps of it) is far above that and far below a missing or doubled contribution
    monkeypatch.setenv("NGP_FUSED_RENDER", "0")
    res0, table_grad0 = run(o, d)
    _, table_grad1 = run(o, d)
    monkeypatch.delenv("NGP_FUSED_RENDER")
    assert torch.equal(res0["rgb"], res["rgb"].detach()) and not res0["rgb"].grad_fn is None
    tol = 2.0**-17 * float(table_grad0.abs().max())
    print("table gradient: |with ray grad - without| = %.3g, run to run %.3g, bound %.3g"
          % (float((table_grad - table_grad0).abs().max()), float((table_grad1 - table_grad0).abs().max()), tol))
    assert float((table_grad - table_grad0).abs().max()) <= tol

    # rays that do not require grad still take the fused node, with the results of a plain call
    torch.manual_seed(9)
    with torch.autocast("cuda", dtype=torch.float16):
        plain = render(m, o, d, exp_step_factor=0.0)
        plain = {k: plain[k].clone() for k in ("rgb", "opacity", "depth", "rays_a")}
    plain["rays_a"] = plain["rays_a"][:, [0, 2]]            # (the fused node packs the ranges in block-completion order: starts vary)
    torch.manual_seed(9)
    with torch.autocast("cuda", dtype=torch.float16):
        again = render(m, og.detach(), dg.detach(), exp_step_factor=0.0)
    assert isinstance(again, TrainResults)
    for k, v in plain.items():
        assert torch.equal(again[k][:, [0, 2]] if k == "rays_a" else again[k], v), k
    # and with grad mode off the rays' flag changes nothing either
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert not render(m, og, dg, exp_step_factor=0.0)["rgb"].requires_grad


def test_models_without_a_position_gradient_refuse(hip_lib):
    from modules.networks import NGP, VoxelGrid
    from modules.rendering import render
    o = torch.zeros(8, 3, device=DEV).requires_grad_()
    d = Fn.normalize(torch.ones(8, 3, device=DEV), dim=1)
    for model in (NGP(scale=0.5, pos_encoder_type="triplane", max_res=256).to(DEV), VoxelGrid(scale=0.5, grid_size=16).to(DEV)):
        with pytest.raises(NotImplementedError, match="position gradient"):
            render(model, o, d, exp_step_factor=0.0)
        with torch.autocast("cuda", dtype=torch.float16), pytest.raises(NotImplementedError, match="position gradient"):
            render(model, o.detach(), d.clone().requires_grad_(), exp_step_factor=0.0)


# ------------------------------------------------------------------------------------------------------------------ 4. registration
def test_registration_closed_loop(hip_lib):
    """Six cameras 1.5 degrees and 0.02 off, a known field, nothing trained: 300 Adam steps on dR, dT alone must at least halve the mean
    rotation and translation errors.

    Measured on the MI355X: rotation 1.5 -> 0.189 degrees (x0.126), translation 0.02 -> 0.00453 (x0.226)."""
    from modules.rendering import render
    from ngp_hip.poses import PoseRefiner
    from ngp_hip.rays import RayBatcher, get_rays
    true, dirs = _cameras()
    model = FieldModel(60.0, view_dep=False)
    with torch.no_grad():
        images = torch.stack([render(model, *get_rays(dirs, p), test_time=True, exp_step_factor=0.0)["rgb"] for p in true])
    assert float(images.std()) > 0.05                                       # the views show the blobs
    start = _perturbed(true, 1.5, 0.02, seed=4)
    rot0, tr0 = _pose_errors(start, true)
    assert abs(rot0 - 1.5) < 1e-2 and abs(tr0 - 0.02) < 1e-4
    batcher = RayBatcher(images, start, dirs, batch_size=512)
    refiner = PoseRefiner(6).to(DEV)
    opt = torch.optim.Adam(refiner.parameters(), lr=4e-3)
    torch.manual_seed(31)
    for _ in range(300):
        batch = batcher.sample(poses=refiner(batcher.poses))
        loss = Fn.mse_loss(render(model, batch["rays_o"], batch["rays_d"], exp_step_factor=0.0)["rgb"], batch["rgb"])
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        rot1, tr1 = _pose_errors(refiner(batcher.poses), true)
    print("registration: rotation %.4f -> %.4f deg (x%.3f), translation %.5f -> %.5f (x%.3f), bound x0.5"
          % (rot0, rot1, rot1 / rot0, tr0, tr1, tr1 / tr0))
    assert rot1 <= 0.5 * rot0 and tr1 <= 0.5 * tr0


# ------------------------------------------------------------------------------------------------------------------ 5. the example
def test_example_runs(hip_lib, flag=()):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "refine_poses.py"), "--steps", "48", "--wh", "64", "--n_train", "12",
           "--n_test", "2", "--batch", "2048", *flag]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    print("examples/refine_poses.py %s: %s" % (" ".join(flag), out))
    assert out["refine"] is (not flag)
    for k in ("rot_err_deg_before", "rot_err_deg_after", "trans_err_before", "trans_err_after", "test_psnr_mean"):
        assert math.isfinite(out[k]), k
    if flag:
        assert out["rot_err_deg_after"] == out["rot_err_deg_before"] and out["trans_err_after"] == out["trans_err_before"]
