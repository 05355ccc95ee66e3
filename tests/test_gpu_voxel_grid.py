"""Voxel-grid radiance field (model_name='svox') on the GPU: ngp_voxel_fwd / _bwd against the torch restatement
(tests/voxel_reference.py) and the reference's own rows (tests/golden/ref_voxel_grid.npz), the march and the occupancy update at
G = 256, the module, a drop-in training trajectory and a train.py-shaped run on the procedural scene."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import voxel_reference as vr
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 0.0125


def _fields(G, deg, seed, lo=-1.5, hi=1.5):
    g = torch.Generator().manual_seed(seed)
    D = (deg + 1)**2
    sh = (torch.rand(G, G, G, 3 * D, generator=g) * (hi - lo) + lo)
    dens = torch.rand(G, G, G, 1, generator=g) * 2 - 0.5                     # about a quarter of the rows <= 0
    return sh, dens


def _dirs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g) * 3.0                               # not unit: the kernel normalises


@pytest.mark.parametrize("deg", range(5))
@pytest.mark.parametrize("G", [16, 32])
def test_forward_on_the_reference_rows(hip_lib, G, deg):
    from ngp_hip import ops
    fix = np.load(os.path.join(GOLDEN, "ref_voxel_grid.npz"))
    x = torch.from_numpy(fix["g%d_x" % G])
    d = _dirs(x.shape[0], deg)
    sh, _ = _fields(G, deg, 10 * G + deg)
    rowcode = torch.arange(1, G**3 + 1, dtype=torch.float32).reshape(G, G, G, 1)   # sigma names the row (exact below 2^24)
    m = float(vr.grid_min(G, R))
    s, c = ops.voxel_fwd(x.to(DEV), d.to(DEV), sh.to(DEV), rowcode.to(DEV), G, deg, m, R)
    rows = s.cpu().to(torch.int64) - 1
    assert np.array_equal(rows.numpy(), fix["g%d_row" % G])
    s_ref, c_ref = vr.forward(x, d, sh, rowcode, G, deg, R)
    assert torch.equal(s.cpu(), s_ref)
    assert float((c.cpu() - c_ref).abs().max()) <= 1e-6


@pytest.mark.parametrize("deg", range(5))
def test_forward_g256(hip_lib, deg):
    from ngp_hip import ops
    G = 256
    sh, dens = _fields(G, deg, deg)
    rng = np.random.default_rng(deg)
    m = vr.grid_min(G, R)
    x = rng.uniform(m - 3 * R, m + (G + 2) * R, (65536, 3)).astype(np.float32)
    k = rng.integers(-1, G + 1, (4096, 3)).astype(np.float32)
    x[:4096] = m + (k + np.float32(0.5)) * np.float32(R)                       # ties
    x = torch.from_numpy(x)
    d = _dirs(x.shape[0], 7)
    s, c = ops.voxel_fwd(x.to(DEV), d.to(DEV), sh.to(DEV), dens.to(DEV), G, deg, float(m), R)
    s_ref, c_ref = vr.forward(x, d, sh, dens, G, deg, R)
    assert torch.equal(s.cpu(), s_ref)
    assert float((c.cpu() - c_ref).abs().max()) <= 1e-6
    sd = ops.voxel_density(x.to(DEV), dens.to(DEV), G, float(m), R)
    assert torch.equal(sd.cpu(), s_ref)


def test_ops_reject_mismatched_shapes(hip_lib):
    from ngp_hip import ops
    G, m = 16, float(vr.grid_min(16, R))
    sh, dens = torch.zeros(G, G, G, 27, device=DEV), torch.zeros(G, G, G, 1, device=DEV)
    x = torch.zeros(64, 3, device=DEV)
    with pytest.raises(ValueError, match="dirs"):
        ops.voxel_fwd(x, torch.zeros(32, 3, device=DEV), sh, dens, G, 2, m, R)         # fewer direction rows than samples
    with pytest.raises(ValueError, match="dirs"):
        ops.voxel_fwd(x.reshape(-1), torch.zeros(64, 3, device=DEV).reshape(-1), sh, dens, G, 2, m, R)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        ops.voxel_density(torch.zeros(64, 2, device=DEV), dens, G, m, R)


def _ray_samples(n_rays, per_ray, G, seed):
    """Consecutive samples along rays at the default step (sqrt(3)/1024): ~7 samples per voxel of 0.0125."""
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(n_rays, 3, generator=g) - 0.5) * 0.6
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=1)
    t = torch.arange(per_ray, dtype=torch.float32) * (3**0.5 / 1024)
    x = (o[:, None] + t[None, :, None] * d[:, None]).reshape(-1, 3)
    return x.contiguous(), d[:, None].expand(n_rays, per_ray, 3).reshape(-1, 3).contiguous()


def _check_backward(x, d, sh, dens, G, deg, g_s, g_c, rel=1e-5):
    from ngp_hip import ops
    m = float(vr.grid_min(G, R))
    X, Dd = x.to(DEV), d.to(DEV)
    s, c = ops.voxel_fwd(X, Dd, sh.to(DEV), dens.to(DEV), G, deg, m, R)
    dsh, dden = torch.zeros_like(sh, device=DEV), torch.zeros_like(dens, device=DEV)
    ops.voxel_bwd(X, Dd, s, c, g_s.to(DEV), g_c.to(DEV), G, deg, m, R, dsh, dden)
    sh64, de64 = sh.double().requires_grad_(True), dens.double().requires_grad_(True)
    s64, c64 = vr.forward(x, d.double(), sh64, de64, G, deg, R)
    ((s64 * g_s.double()).sum() + (c64 * g_c.double()).sum()).backward()
    # per-entry magnitude: the same sums over absolute contributions
    rows = vr.rows(x, G, R)
    valid = rows >= 0
    D = (deg + 1)**2
    dn = d.double() / torch.norm(d.double(), dim=1, keepdim=True)
    eye = torch.eye(D, dtype=torch.float64)
    Y = torch.stack([vr.eval_sh(deg, eye[k].expand(x.shape[0], 1, D), dn)[:, 0] for k in range(D)], 1)    # basis [n, D]
    gc = (g_c.double() * c64.detach() * (1 - c64.detach())).abs()
    mag_sh = torch.zeros(G**3, 3 * D, dtype=torch.float64)
    # (+0.1: the kernel evaluates each basis polynomial in f32; near a root such as 2zz - xx - yy = 0 its rounding error is relative to
    # the polynomial's terms, not to the small value)
    mag_sh.index_add_(0, rows[valid], (gc[:, :, None] * (Y.abs() + 0.1)[:, None, :]).reshape(-1, 3 * D)[valid])
    mag_de = torch.zeros(G**3, dtype=torch.float64)
    mag_de.index_add_(0, rows[valid], g_s.double().abs()[valid])
    for got, ref, mag in ((dsh.cpu().double().reshape(G**3, -1), sh64.grad.reshape(G**3, -1), mag_sh),
                          (dden.cpu().double().reshape(-1), de64.grad.reshape(-1), mag_de.reshape(-1))):
        bad = (got - ref).abs() > rel * mag + 1e-30
        assert not bool(bad.any()), (int(bad.sum()), float(((got - ref).abs() - rel * mag).max()))
        assert bool((got[mag == 0] == 0).all())
    return dsh, dden


@pytest.mark.parametrize("deg", range(5))
def test_backward_ray_runs(hip_lib, deg):
    G = 64
    sh, dens = _fields(G, deg, 100 + deg, -0.5, 0.5)        # moderate colours: rgb (1 - rgb) from the saved f32 rgb stays accurate
    x, d = _ray_samples(512, 200, G, deg)
    g = torch.Generator().manual_seed(deg)
    g_s, g_c = torch.randn(x.shape[0], generator=g), torch.randn(x.shape[0], 3, generator=g)
    g_s[::7] = 0.0
    g_c[::5] = 0.0
    x[::97] = 5.0                                                                # out of the grid: no gradient
    _check_backward(x, d, sh, dens, G, deg, g_s, g_c)


def test_backward_hot_voxel_and_outside(hip_lib):
    """One hot voxel: (a) every sample in it, so every wave is one 64-lane run and all waves add into the same row; (b) the same
    samples interleaved with out-of-grid ones (runs of one or two lanes; the outside samples get no gradient); (c) the row's
    density <= 0: its density gradient must be zero."""
    G, deg = 32, 2
    g = torch.Generator().manual_seed(1)
    sh = torch.rand(G, G, G, 27, generator=g) - 0.5
    dens = torch.full((G, G, G, 1), 0.3)
    m = vr.grid_min(G, R)
    n = 65536
    x = (torch.full((n, 3), float(m + 10 * np.float32(R))) + (torch.rand(n, 3, generator=g) - 0.5) * 0.8 * R).float()
    d = _dirs(n, 2)
    g_s, g_c = torch.randn(n, generator=g), torch.randn(n, 3, generator=g)
    assert bool((vr.rows(x, G, R) == (10 * G + 10) * G + 10).all())
    dsh, dden = _check_backward(x, d, sh, dens, G, deg, g_s, g_c)
    assert int(torch.count_nonzero(dden)) == 1 and int(torch.count_nonzero(dsh.reshape(G**3, -1).any(1))) == 1
    x[1::3] = torch.tensor([-9.0, 0.0, 0.0])
    _check_backward(x, d, sh, dens, G, deg, g_s, g_c)
    dens[10, 10, 10, 0] = -0.2
    _, dden = _check_backward(x, d, sh, dens, G, deg, g_s, g_c)
    assert int(torch.count_nonzero(dden)) == 0


def _packbits_ref(grid, threshold):
    """numpy statement of ngp_voxel_occ_pack: bit = v > 0 and v >= f32(min(f64 mean of the positive cells, threshold))."""
    v = grid.astype(np.float64)
    pos = v > 0
    if not pos.any():
        return np.zeros(grid.size // 8, np.uint8)
    thr = np.float32(min(v[pos].mean(), threshold))
    return np.packbits((grid > 0) & (grid >= thr), bitorder="little")


def test_occupancy_packbits_threshold(hip_lib):
    from ngp_hip import ops
    rng = np.random.default_rng(4)
    n = 1 << 21
    grid = rng.uniform(-1, 3, n).astype(np.float32)
    grid[rng.random(n) < 0.1] = 0.0
    grid[rng.random(n) < 0.1] = -1.0
    mean = grid[grid > 0].astype(np.float64).mean()
    bits = torch.zeros(n // 8, dtype=torch.uint8, device=DEV)
    g = torch.from_numpy(grid).to(DEV)
    for thr in (10.0, mean * 0.5, 0.25):                             # the mean decides; the threshold decides (twice)
        got = ops.voxel_occ_pack(g, thr, bits).cpu().numpy()
        ref = _packbits_ref(grid, thr)
        assert np.array_equal(got, ref), (thr, int((got != ref).sum()))
    assert 0 < int(np.unpackbits(got).sum()) < n
    # the fresh-field case: one value in every visible cell, -1 elsewhere -> every visible cell, on every run
    fresh = np.where(rng.random(n) < 0.7, np.float32(0.1), np.float32(-1.0)).astype(np.float32)
    for _ in range(3):
        got = ops.voxel_occ_pack(torch.from_numpy(fresh).to(DEV), 0.01 * 1024 / 3**0.5, bits).cpu().numpy()
        assert np.array_equal(got, np.packbits(fresh > 0, bitorder="little"))
    # no positive cell: nothing is marked
    none = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-1.0)).astype(np.float32)
    got = ops.voxel_occ_pack(torch.from_numpy(none).to(DEV), 0.5, bits.fill_(255)).cpu().numpy()
    assert int(got.sum()) == 0
    with pytest.raises(ValueError, match="16-byte"):
        ops.voxel_occ_pack(torch.zeros(n + 1, device=DEV)[1:], 0.5, bits)


def test_march_at_g256_matches_the_oracle(hip_lib, oracle):
    from ngp_hip import ops, synthetic
    G = 256
    bits = synthetic.ball_slab_bitfield(1, 0.5, grid_size=G)
    o, d = synthetic.lego_rays(1024, seed=9)
    noise = np.random.default_rng(3).random(1024, dtype=np.float32)
    hits = oracle.ray_aabb(o, d, 0.5)
    ra_ref, total_ref = oracle.march_train(o, d, hits, bits, noise, 1, 0.5, 0.0, G, 1024, count_only=True)
    cnt_ref = np.zeros(1024, np.int64)
    cnt_ref[ra_ref[:, 0]] = ra_ref[:, 2]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rays_a, xyzs, *_ , total = ops.march_train(t(o), t(d), t(hits), t(bits), t(noise), 1, 0.5, 0.0, G, 1024)
    ra = rays_a.cpu().numpy()
    cnt = np.zeros(1024, np.int64)
    cnt[ra[:, 0]] = ra[:, 2]
    assert np.array_equal(cnt, cnt_ref) and int(cnt.sum()) == total_ref > 10000
    # test-time march, two rounds
    alive = np.arange(1024, dtype=np.int64)
    h_ref, h_gpu = hits.copy(), t(hits).contiguous()
    for n_step in (4, 16):
        _, _, _, _, c_ref = oracle.march_test(o, d, h_ref, alive, bits, 1, 0.5, 0.0, G, n_step)
        _, _, _, _, c_gpu = ops.march_test(t(o), t(d), h_gpu, t(alive), t(bits), 1, 0.5, 0.0, G, n_step)
        assert np.array_equal(c_gpu.cpu().numpy(), c_ref)


def _cams(n=20, seed=5, radius=1.39):
    """K, [n, 3, 4] poses and image size of Blender-like cameras on the upper hemisphere (ngp_hip.synthetic.lego_rays' rig)."""
    from ngp_hip import synthetic
    rng = np.random.default_rng(seed)
    z = 0.05 + 0.9 * rng.random(n)
    phi = rng.random(n) * 2 * np.pi
    rxy = np.sqrt(1 - z * z)
    cams = radius * np.stack([rxy * np.cos(phi), rxy * np.sin(phi), z], -1)
    rot = synthetic._look_at(cams.copy(), np.zeros_like(cams), np.zeros(n))
    poses = np.concatenate([rot, cams[:, :, None]], 2)
    K = torch.tensor([[1111.1, 0, 400], [0, 1111.1, 400], [0, 0, 1]])
    return K.to(DEV), torch.from_numpy(poses).float().to(DEV), (800, 800)


def test_fresh_model_fully_occupied_after_warmup_g256(hip_lib):
    from modules.networks import VoxelGrid
    m = VoxelGrid().to(DEV)
    m.mark_invisible_cells(*_cams())
    visible = m.density_grid[0] >= 0
    assert int(visible.sum()) > 0
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.autocast("cuda", dtype=torch.float16):
        m.update_density_grid(0.01 * 1024 / 3**0.5, warmup=True)
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 1.75 * 2**30, peak                                         # no [G^3, 32] f32 encoding buffer (2 GiB)
    bits = torch.from_numpy(np.unpackbits(m.density_bitfield.cpu().numpy(), bitorder="little").astype(bool))
    assert torch.equal(bits, visible.cpu()), (int(bits.sum()), int(visible.sum()))
    assert bool((m.density_grid[0][visible] == np.float32(0.1)).all())
    # the regular (non-warm-up) update runs at this size too (cells not redrawn decay below the mean and drop out, as for NGP)
    with torch.autocast("cuda", dtype=torch.float16):
        m.update_density_grid(0.01 * 1024 / 3**0.5, warmup=False)
    bits2 = torch.from_numpy(np.unpackbits(m.density_bitfield.cpu().numpy(), bitorder="little").astype(bool))
    assert int(bits2.sum()) > 0 and not bool((bits2 & ~visible.cpu()).any())


class TorchVoxel(torch.nn.Module):
    """The same model with the restatement's torch forward (autograd backward) in place of the kernels."""

    def __init__(self, m):
        super().__init__()
        self.inner = m

    def forward(self, x, d):
        k = self.inner
        return vr.forward(x.float(), d.float(), k.sh_fields, k.density_fields, k.grid_size, k.sh_degree, k.grid_radius)


def test_module_matches_restatement_with_and_without_autocast(hip_lib):
    from modules.networks import VoxelGrid
    a = VoxelGrid(grid_size=64, sh_degree=3).to(DEV)
    with torch.no_grad():
        a.sh_fields.uniform_(-1, 1)
        a.density_fields.uniform_(-0.5, 2)
    b = copy.deepcopy(a)
    x, d = _ray_samples(256, 300, 64, 4)
    x, d = x.to(DEV), d.to(DEV)
    for ac in (False, True):
        outs = []
        for fwd, m in ((a, a), (TorchVoxel(b), b)):
            m.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                s, c = fwd(x, d)
                loss = (s * 1e-2).sum() + c.square().sum()
            assert s.dtype == torch.float32 and c.dtype == torch.float32
            loss.backward()
            outs.append((s, c, m.sh_fields.grad, m.density_fields.grad))
        (sa, ca, ga, da), (sb, cb, gb, db) = outs
        assert torch.equal(sa, sb)
        assert float((ca - cb).abs().max()) <= 1e-6
        assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max())
        assert float((da - db).abs().max()) <= 1e-5 * float(db.abs().max())
    assert torch.equal(a.density(x), sa)
    with torch.no_grad():
        assert torch.equal(a.density(x), sa)


def test_fused_trainer_refuses_the_voxel_grid(hip_lib):
    from modules.networks import VoxelGrid
    from ngp_hip.trainer import FusedTrainer
    m = VoxelGrid(grid_size=16).to(DEV)
    with pytest.raises(ValueError, match="drop-in"):
        FusedTrainer(m)


def _compat():
    compat = os.path.join(ROOT, "taichi-nerfs_amd", "compat")
    if compat not in sys.path:
        sys.path.insert(0, compat)


def _train(model, fwd, steps, seed=3):
    """train.py's loop shape (render + compat FusedAdam + GradScaler under autocast fp16) on a fully occupied grid."""
    _compat()
    from apex.optimizers import FusedAdam
    from modules.rendering import render
    from ngp_hip import synthetic
    model.density_bitfield.fill_(255)
    opt = FusedAdam(model.parameters(), lr=1e-2, eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**19)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    losses = []
    for step in range(steps):
        o, d = synthetic.lego_rays(2048, seed=100 + step)
        o, d = torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV)
        target = torch.rand(2048, 3, generator=gen).to(DEV) * 0.2 + 0.4
        torch.manual_seed(1000 + step)
        with torch.autocast("cuda", dtype=torch.float16):
            res = render(_Bound(model, fwd), o, d, exp_step_factor=0.0)
            loss = torch.nn.functional.mse_loss(res["rgb"], target)
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss))
    return np.array(losses)


class _Bound:
    """render()'s view of a model whose shading is `fwd` (the kernels or the torch restatement)."""

    def __init__(self, model, fwd):
        self._m, self._fwd = model, fwd

    def __getattr__(self, k):
        return getattr(self._m, k)

    def __call__(self, x, d):
        return self._fwd(x, d)


def test_training_trajectory_matches_torch_restatement(hip_lib):
    from modules.networks import VoxelGrid
    torch.manual_seed(0)
    a = VoxelGrid(grid_size=128).to(DEV)
    with torch.no_grad():
        a.sh_fields.uniform_(-0.3, 0.3)
        a.density_fields.uniform_(0.0, 20.0)
    b = copy.deepcopy(a)
    la = _train(a, a, 24)
    lb = _train(b, TorchVoxel(b), 24)
    assert np.all(np.isfinite(la)) and la[-1] < la[0]
    rel = np.abs(la - lb) / np.abs(lb)
    assert rel.max() < 1e-3, rel


def _psnr(model, o, d, gt):
    from modules.rendering import render
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        rgb = render(model, o, d, test_time=True, exp_step_factor=0.0)["rgb"]
    return float(-10 * torch.log10(((rgb.float().clamp(0, 1) - gt) ** 2).mean()))


def test_train_py_shaped_run_on_the_procedural_scene(hip_lib):
    """train.py's svox run in miniature: MODEL_DICT['svox'] with the driver's defaults, mark_invisible_cells, the occupancy update
    every 16 steps (warm-up for the first 256), render + FusedAdam(lr 1e-2) + GradScaler(2^19) under autocast, 8192 rays a step on
    the analytic scene of ngp_hip.synthetic; PSNR on held-out rays before and after."""
    _compat()
    from apex.optimizers import FusedAdam
    from modules.networks import MODEL_DICT
    from modules.rendering import render
    from ngp_hip import synthetic
    torch.manual_seed(0)
    model = MODEL_DICT['svox'](scale=0.5, half_opt=False, sh_degree=2, grid_size=256, grid_radius=0.0125, origin_sh=0.,
                               origin_sigma=0.1).to(DEV)
    model.mark_invisible_cells(*_cams())
    o_t, d_t = synthetic.lego_rays(8192, seed=777)
    o_t, d_t = torch.from_numpy(o_t).to(DEV), torch.from_numpy(d_t).to(DEV)
    gt_t = synthetic.procedural_render_gt(o_t, d_t)
    psnr0 = _psnr(model, o_t, d_t, gt_t)
    opt = FusedAdam(model.parameters(), lr=1e-2, eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**19)
    steps = 400
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
    psnr1 = _psnr(model, o_t, d_t, gt_t)
    print("svox procedural run: PSNR %.2f dB -> %.2f dB after %d steps" % (psnr0, psnr1, steps))
    # measured on one MI355X: 8.60 -> 15.05 dB (voxel grid); the bar keeps ~2 dB of margin on both
    assert psnr1 >= 13.0 and psnr1 - psnr0 >= 4.0, (psnr0, psnr1)
