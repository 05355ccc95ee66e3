"""Trilinear lookup of the voxel-grid radiance field (VoxelGrid(use_trilinear=True)) on the GPU: ngp_voxel_trilinear_fwd / _density /
_bwd against the torch restatement (tests/voxel_trilinear_reference.py) evaluated in f64, the exact cases of the contract, the
module, the occupancy update of a fresh model, a drop-in training trajectory and a train.py-shaped run in both modes."""
import copy

import numpy as np
import pytest
import torch

import test_gpu_voxel_grid as base
import voxel_reference as vr
import voxel_trilinear_reference as vt

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 0.0125
EPS = 2.0**-24


def _points(G, radius, n, seed, lo=-2.0, hi=None):
    """f32 positions whose index u = (p - m) / r is uniform in [lo, hi) per axis (default hi: G + 1)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(lo, G + 1 if hi is None else hi, (n, 3))
    return torch.from_numpy((np.float64(vr.grid_min(G, radius)) + u * np.float64(np.float32(radius))).astype(np.float32))


def _forward_bounds(x, d, sh, dens, G, deg, radius):
    """The f64 yardstick with the two bounds of the forward: sigma 32 * 2^-24 * max|density| (7 lerps, 3 deep, at most 3 roundings each
    on magnitudes <= 2 max: 18 * 2^-24 * max), rgb 4 x the f32 restatement's own distance from its f64 evaluation, at least 1e-6."""
    s64, c64 = vt.forward(x, d.double(), sh.double(), dens.double(), G, deg, radius)
    s32, c32 = vt.forward(x, d, sh, dens, G, deg, radius)
    own_s, own_c = float((s32.double() - s64).abs().max()), float((c32.double() - c64).abs().max())
    return s64, c64, 32 * EPS * float(dens.abs().max()), max(4 * own_c, 1e-6), own_s, own_c


@pytest.mark.parametrize("deg", range(5))
@pytest.mark.parametrize("G", [16, 32])
def test_forward_against_the_f64_restatement(hip_lib, G, deg):
    from ngp_hip import ops
    sh, dens = base._fields(G, deg, 10 * G + deg)
    x = _points(G, R, 8192, 100 * G + deg)
    x[17, 1] = float("nan")
    d = base._dirs(x.shape[0], deg)
    inside, b, _ = vt.cell_fraction(x, G, R)
    border = inside & ((b < 0) | (b >= G - 1)).any(1)
    assert min(int((~inside).sum()), int(border.sum()), int((inside & ~border).sum())) > 800          # all three kinds occur
    m = float(vr.grid_min(G, R))
    s, c = ops.voxel_fwd(x.to(DEV), d.to(DEV), sh.to(DEV), dens.to(DEV), G, deg, m, R, trilinear=True)
    s64, c64, tol_s, tol_c, own_s, own_c = _forward_bounds(x, d, sh, dens, G, deg, R)
    err_s, err_c = float((s.cpu().double() - s64).abs().max()), float((c.cpu().double() - c64).abs().max())
    print("trilinear forward G=%d deg=%d: sigma %.2f eps*max (f32 restatement %.2f), rgb %.3g (f32 restatement %.3g, bound %.3g)"
          % (G, deg, err_s / (EPS * float(dens.abs().max())), own_s / (EPS * float(dens.abs().max())), err_c, own_c, tol_c))
    assert err_s <= tol_s, (err_s, tol_s)
    assert err_c <= tol_c, (err_c, tol_c)
    assert bool((s.cpu()[~inside] == 0).all()) and bool((c.cpu()[~inside] == 0.5).all())
    sd = ops.voxel_density(x.to(DEV), dens.to(DEV), G, m, R, trilinear=True)
    assert torch.equal(sd, s)


@pytest.mark.parametrize("G", [16, 64])
def test_grid_points_give_their_row_exactly(hip_lib, G):
    """grid_radius = 2^-6: u is exact, so on-grid samples have f = 0 and the lerps return the row itself."""
    from ngp_hip import ops
    r, deg = 2.0**-6, 2
    sh, dens = base._fields(G, deg, G)
    g = torch.Generator().manual_seed(G)
    k = torch.randint(0, G, (8192, 3), generator=g)
    m = float(vr.grid_min(G, r))
    x = (m + k.double() * r).float()
    d = base._dirs(x.shape[0], 3)
    args = (x.to(DEV), d.to(DEV), sh.to(DEV), dens.to(DEV), G, deg, m, r)
    s, c = ops.voxel_fwd(*args, trilinear=True)
    s_n, c_n = ops.voxel_fwd(*args)
    assert torch.equal(s.cpu(), torch.relu(dens[k[:, 0], k[:, 1], k[:, 2], 0]))
    assert float((c - c_n).abs().max()) <= 1e-6
    assert torch.equal(ops.voxel_density(args[0], args[3], G, m, r, trilinear=True), s)


def test_constant_field_is_returned_exactly(hip_lib):
    from ngp_hip import ops
    G, deg = 32, 2
    x = _points(G, R, 8192, 5, lo=0.0, hi=G - 1).to(DEV)
    sh, dens = torch.full((G, G, G, 27), 0.3, device=DEV), torch.full((G, G, G, 1), 0.1, device=DEV)
    m = float(vr.grid_min(G, R))
    s, _ = ops.voxel_fwd(x, base._dirs(8192, 1).to(DEV), sh, dens, G, deg, m, R, trilinear=True)
    assert bool((s == np.float32(0.1)).all())
    assert bool((ops.voxel_density(x, dens, G, m, R, trilinear=True) == np.float32(0.1)).all())


def _check_backward(x, d, sh, dens, G, deg, g_s, g_c, rel=1e-5, ref_dev=DEV):
    """Per entry |got - ref| <= rel * mag against f64 autograd of the restatement; mag is the same sum over absolute contributions
    (sum w_corner |g| (|Y| + 0.1) for SH, sum w_corner |g_sigma| for density), and entries with mag == 0 are exactly 0.  The
    reference is evaluated on `ref_dev` (the host where every sample adds into the same rows: torch's f64 index_add serialises there)."""
    from ngp_hip import ops
    m = float(vr.grid_min(G, R))
    X, Dd, SH, DE, GS, GC = (t.to(DEV) for t in (x, d, sh, dens, g_s, g_c))
    s, c = ops.voxel_fwd(X, Dd, SH, DE, G, deg, m, R, trilinear=True)
    dsh, dden = torch.zeros_like(SH), torch.zeros_like(DE)
    ops.voxel_bwd(X, Dd, s, c, GS, GC, G, deg, m, R, dsh, dden, trilinear=True)
    X, Dd, SH, DE, GS, GC = (t.to(ref_dev) for t in (x, d, sh, dens, g_s, g_c))
    sh64, de64 = SH.double().requires_grad_(True), DE.double().requires_grad_(True)
    s64, c64 = vt.forward(X, Dd.double(), sh64, de64, G, deg, R)
    ((s64 * GS.double()).sum() + (c64 * GC.double()).sum()).backward()
    D = (deg + 1)**2
    n = X.shape[0]
    inside, b, f = vt.cell_fraction(X, G, R)
    w = vt.corner_weights(f.double())
    dn = Dd.double() / torch.norm(Dd.double(), dim=1, keepdim=True)
    eye = torch.eye(D, dtype=torch.float64, device=ref_dev)
    Y = torch.stack([vr.eval_sh(deg, eye[k].expand(n, 1, D), dn)[:, 0] for k in range(D)], 1)             # basis [n, D]
    gc = (GC.double() * c64.detach() * (1 - c64.detach())).abs()
    # (+0.1: the kernel evaluates each basis polynomial in f32; near a root its rounding error is relative to the polynomial's terms)
    per_sh = (gc[:, :, None] * (Y.abs() + 0.1)[:, None, :]).reshape(n, 3 * D)
    mag_sh = torch.zeros(G**3, 3 * D, dtype=torch.float64, device=ref_dev)
    mag_de = torch.zeros(G**3, dtype=torch.float64, device=ref_dev)
    rows, valid = vt.corner_rows(inside, b, G)
    for c8 in range(8):
        ok = valid[:, c8]
        mag_sh.index_add_(0, rows[ok, c8], (per_sh * w[:, c8:c8 + 1])[ok])
        mag_de.index_add_(0, rows[ok, c8], (GS.double().abs() * w[:, c8])[ok])
    for got, ref, mag in ((dsh.to(ref_dev).double().reshape(G**3, -1), sh64.grad.reshape(G**3, -1), mag_sh),
                          (dden.to(ref_dev).double().reshape(-1), de64.grad.reshape(-1), mag_de)):
        bad = (got - ref).abs() > rel * mag + 1e-30
        assert not bool(bad.any()), (int(bad.sum()), float(((got - ref).abs() - rel * mag).max()))
        assert bool((got[mag == 0] == 0).all())
    return dsh, dden


@pytest.mark.parametrize("deg", range(5))
@pytest.mark.parametrize("G", [64, 16])
def test_backward_ray_runs(hip_lib, G, deg):
    """G = 64 holds the rays; at G = 16 the field (+-0.1) is smaller than the scene, so rays cross the border and corners are invalid."""
    sh, dens = base._fields(G, deg, 100 + deg, -0.5, 0.5)
    x, d = base._ray_samples(512, 200, G, deg)
    g = torch.Generator().manual_seed(deg)
    g_s, g_c = torch.randn(x.shape[0], generator=g), torch.randn(x.shape[0], 3, generator=g)
    g_s[::7] = 0.0
    g_c[::5] = 0.0
    x[::97] = 5.0                                                                # out of the grid: no gradient
    inside, b, _ = vt.cell_fraction(x, G, R)
    if G == 16:
        assert int((~inside).sum()) > 1000 and int((inside & ((b < 0) | (b >= G - 1)).any(1)).sum()) > 1000
    _check_backward(x, d, sh, dens, G, deg, g_s, g_c)


def test_backward_hot_cell_and_outside(hip_lib):
    """One hot cell: (a) every sample in it, so every wave is one 64-lane run and all waves add into the same eight rows; (b) the same
    interleaved with out-of-grid samples (runs of one or two lanes); (c) the cell's eight densities negative: no density gradient."""
    G, deg = 32, 2
    g = torch.Generator().manual_seed(1)
    sh = torch.rand(G, G, G, 27, generator=g) - 0.5
    dens = torch.full((G, G, G, 1), 0.3)
    m = vr.grid_min(G, R)
    n = 65536
    x = (torch.full((n, 3), float(m + np.float32(10.5) * np.float32(R))) + (torch.rand(n, 3, generator=g) - 0.5) * 0.8 * R).float()
    d = base._dirs(n, 2)
    g_s, g_c = torch.randn(n, generator=g), torch.randn(n, 3, generator=g)
    inside, b, _ = vt.cell_fraction(x, G, R)
    assert bool(inside.all()) and bool((b == 10).all())
    dsh, dden = _check_backward(x, d, sh, dens, G, deg, g_s, g_c, ref_dev="cpu")
    assert int(torch.count_nonzero(dden)) == 8 and int(torch.count_nonzero(dsh.reshape(G**3, -1).any(1))) == 8
    x[1::3] = torch.tensor([-9.0, 0.0, 0.0])
    _check_backward(x, d, sh, dens, G, deg, g_s, g_c, ref_dev="cpu")
    dens[10:12, 10:12, 10:12, 0] = -0.2
    _, dden = _check_backward(x, d, sh, dens, G, deg, g_s, g_c, ref_dev="cpu")
    assert int(torch.count_nonzero(dden)) == 0


class TorchVoxelTri(torch.nn.Module):
    """The same model with the trilinear restatement's torch forward (autograd backward) in place of the kernels."""

    def __init__(self, m):
        super().__init__()
        self.inner = m

    def forward(self, x, d):
        k = self.inner
        return vt.forward(x.float(), d.to(k.sh_fields.dtype), k.sh_fields, k.density_fields, k.grid_size, k.sh_degree, k.grid_radius)


def test_module_matches_restatement_with_and_without_autocast(hip_lib):
    from modules.networks import VoxelGrid
    from ngp_hip import ops
    a = VoxelGrid(grid_size=64, sh_degree=3, use_trilinear=True).to(DEV)
    with torch.no_grad():
        a.sh_fields.uniform_(-1, 1)
        a.density_fields.uniform_(-0.5, 2)
    b = copy.deepcopy(a)
    x, d = base._ray_samples(256, 300, 64, 4)
    x, d = x.to(DEV), d.to(DEV)
    # the f64 yardstick, once: outputs, both gradients, and the forward's bounds
    sh64, de64 = a.sh_fields.detach().double().requires_grad_(True), a.density_fields.detach().double().requires_grad_(True)
    s64, c64 = vt.forward(x, d.double(), sh64, de64, 64, 3, R)
    ((s64 * 1e-2).sum() + c64.square().sum()).backward()
    tol_s = 32 * EPS * float(de64.abs().max())
    for ac in (False, True):
        outs = []
        for fwd, m in ((a, a), (TorchVoxelTri(b), b)):
            m.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                s, c = fwd(x, d)
                loss = (s * 1e-2).sum() + c.square().sum()
            assert s.dtype == torch.float32 and c.dtype == torch.float32
            loss.backward()
            outs.append((s, c, m.sh_fields.grad, m.density_fields.grad))
        (sa, ca, ga, da), (sb, cb, _, _) = outs
        tol_c = max(4 * float((cb.double() - c64).abs().max()), 1e-6)
        assert float((sa.double() - s64).abs().max()) <= tol_s
        assert float((ca.double() - c64).abs().max()) <= tol_c
        assert float((ga.double() - sh64.grad).abs().max()) <= 1e-5 * float(sh64.grad.abs().max())
        assert float((da.double() - de64.grad).abs().max()) <= 1e-5 * float(de64.grad.abs().max())
    assert torch.equal(a.density(x), sa)
    with torch.no_grad():
        assert torch.equal(a.density(x), sa)
    # a checkpoint saved in nearest mode loads into trilinear mode and back
    near = VoxelGrid(grid_size=64, sh_degree=3, use_trilinear=False).to(DEV)
    near.load_state_dict(a.state_dict())
    s_n, c_n = near(x, d)
    assert torch.equal(s_n, ops.voxel_fwd(x, d, a.sh_fields, a.density_fields, *a._cfg())[0]) and not torch.equal(s_n, sa)
    tri = VoxelGrid(grid_size=64, sh_degree=3, use_trilinear=True).to(DEV)
    tri.load_state_dict(near.state_dict())
    with torch.no_grad():
        s_t, c_t = tri(x, d)
    assert torch.equal(s_t, sa) and torch.equal(c_t, ca)


def test_fresh_trilinear_model_fully_occupied_after_warmup(hip_lib):
    """The check that the lerp form was kept: every visible cell of a fresh model reads exactly origin_sigma, so the `>= mean`
    threshold keeps all of them."""
    from modules.networks import VoxelGrid
    m = VoxelGrid(grid_size=128, use_trilinear=True).to(DEV)
    m.mark_invisible_cells(*base._cams())
    visible = m.density_grid[0] >= 0
    assert int(visible.sum()) > 0
    with torch.autocast("cuda", dtype=torch.float16):
        m.update_density_grid(0.01 * 1024 / 3**0.5, warmup=True)
    bits = torch.from_numpy(np.unpackbits(m.density_bitfield.cpu().numpy(), bitorder="little").astype(bool))
    assert torch.equal(bits, visible.cpu()), (int(bits.sum()), int(visible.sum()))
    assert bool((m.density_grid[0][visible] == np.float32(0.1)).all())


def _train(model, fwd, steps, rays=1024, seed=3):
    """train.py's loop shape (render + compat FusedAdam + GradScaler under autocast fp16) on a fully occupied grid."""
    base._compat()
    from apex.optimizers import FusedAdam
    from modules.rendering import render
    from ngp_hip import synthetic
    model.density_bitfield.fill_(255)
    opt = FusedAdam(model.parameters(), lr=1e-2, eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**19)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    losses = []
    for step in range(steps):
        o, d = synthetic.lego_rays(rays, seed=100 + step)
        o, d = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
        target = torch.rand(rays, 3, generator=gen).to(DEV) * 0.2 + 0.4
        torch.manual_seed(1000 + step)
        with torch.autocast("cuda", dtype=torch.float16):
            res = render(base._Bound(model, fwd), o, d, exp_step_factor=0.0)
            loss = torch.nn.functional.mse_loss(res["rgb"], target)
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss))
    return np.array(losses)


def test_training_trajectory_matches_torch_restatement(hip_lib):
    from modules.networks import VoxelGrid
    torch.manual_seed(0)
    a = VoxelGrid(grid_size=64, use_trilinear=True).to(DEV)
    with torch.no_grad():
        a.sh_fields.uniform_(-0.3, 0.3)
        a.density_fields.uniform_(0.0, 20.0)
    b = copy.deepcopy(a)
    la = _train(a, a, 16)
    lb = _train(b, TorchVoxelTri(b), 16)
    assert np.all(np.isfinite(la)) and la[-1] < la[0]
    rel = np.abs(la - lb) / np.abs(lb)
    assert rel.max() < 1e-3, rel


def _procedural_run(trilinear, steps=400):
    """train.py's svox run in miniature (test_gpu_voxel_grid's, at G = 128: the same resolution inside the +-0.5 box, an eighth of
    the fields): held-out PSNR before and after."""
    base._compat()
    from apex.optimizers import FusedAdam
    from modules.networks import MODEL_DICT
    from modules.rendering import render
    from ngp_hip import synthetic
    torch.manual_seed(0)
    model = MODEL_DICT['svox'](scale=0.5, half_opt=False, sh_degree=2, grid_size=128, grid_radius=0.0125, origin_sh=0.,
                               origin_sigma=0.1, use_trilinear=trilinear).to(DEV)
    model.mark_invisible_cells(*base._cams())
    o_t, d_t = synthetic.lego_rays(8192, seed=777)
    o_t, d_t = torch.from_numpy(o_t).to(DEV), torch.from_numpy(d_t).to(DEV)
    gt_t = synthetic.procedural_render_gt(o_t, d_t)
    psnr0 = base._psnr(model, o_t, d_t, gt_t)
    opt = FusedAdam(model.parameters(), lr=1e-2, eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**19)
    for step in range(steps):
        o, d = synthetic.lego_rays(8192, seed=step)
        o, d = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
        target = synthetic.procedural_render_gt(o, d)
        with torch.autocast("cuda", dtype=torch.float16):
            if step % 16 == 0:
                model.update_density_grid(0.01 * 1024 / 3**0.5, warmup=step < 256)
            res = render(model, o, d, exp_step_factor=0.0)
            loss = torch.nn.functional.mse_loss(res["rgb"], target)
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    return psnr0, base._psnr(model, o_t, d_t, gt_t)


def test_train_py_shaped_run_in_both_modes(hip_lib):
    n0, n1 = _procedural_run(False)
    t0, t1 = _procedural_run(True)
    print("svox procedural run at G=128, 400 steps: nearest %.2f -> %.2f dB, trilinear %.2f -> %.2f dB" % (n0, n1, t0, t1))
    # measured on one MI355X: nearest 8.60 -> 15.05 dB, trilinear 8.60 -> 15.64 dB (voxel grid)
    assert t1 >= 13.0 and t1 - t0 >= 4.0, (t0, t1)
    assert t1 >= n1, (n1, t1)
