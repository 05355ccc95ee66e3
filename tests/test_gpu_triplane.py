"""Tri-plane position encoder on the GPU: ngp_triplane_fwd_f32 / _bwd_f32 against the numpy restatement (tests/triplane_reference.py),
the module against a pure-torch restatement of the encoder, the occupancy update, a drop-in training trajectory and the example."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import triplane_reference as tr
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _table(max_res, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(3 * max_res * max_res * 4, generator=g)


def _edge_points(rng, n, res_top):
    x = rng.random((n, 3), dtype=np.float32)
    x[:10] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1, 0, 0.5], [0, 1, 1], [0.999999, 1e-7, 0.5], [-0.25, 1.5, 0.5],
              [0.3 / (res_top - 1), 0.5, 0.9 / (res_top - 1)], [0.25, 0.75, 1.0], [np.nan, 0.5, 0.5]]
    return x


def _check_grad(got, idx, val, mag, rel=1e-5):
    got = got.double()
    ref = torch.zeros_like(got)
    ref[torch.from_numpy(idx)] = torch.from_numpy(val)
    tol = torch.zeros_like(got)
    tol[torch.from_numpy(idx)] = torch.from_numpy(rel * mag + 1e-30)
    bad = (got - ref).abs() > tol
    assert not bool(bad.any()), (int(bad.sum()), float(((got - ref).abs() - tol).max()))


@pytest.mark.parametrize("max_res", [64, 1024, 4096])
def test_forward_bit_exact(hip_lib, max_res):
    from ngp_hip import ops
    res = tr.resolutions(16, max_res, 8)
    table = _table(max_res, max_res)
    x = _edge_points(np.random.default_rng(max_res), 4096, res[-1])
    lv = ops.make_triplane_levels(16, max_res, 8, 4)
    got = ops.triplane_fwd(torch.from_numpy(x).to(DEV), table.to(DEV), lv).cpu().numpy()
    xr = np.where(np.isnan(x), np.float32(0), x)                   # NaN coordinates clamp to 0 like fmaxf(NaN, 0)
    ref = tr.forward(xr, table.numpy(), max_res, res)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_forward_and_backward_on_the_reference_vectors(hip_lib):
    """The fixture the reference's own kernel produced: the forward bit for bit, the gradient the TRUE one (the fixture's Taichi-level
    adjoint, not the module-level 2x)."""
    from ngp_hip import ops
    fix = np.load(os.path.join(GOLDEN, "ref_triplane.npz"))
    for max_res in (64, 1024):
        t = "r%d" % max_res
        i = np.arange(int(fix[t + "_total_param_size"]), dtype=np.uint64)
        table = ((((i * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(2**32)).astype(np.float64)) / 2**32).astype(np.float32)
        lv = ops.make_triplane_levels(16, max_res, 8, 4)
        x, dout = torch.from_numpy(fix[t + "_x"]).to(DEV), torch.from_numpy(fix[t + "_dout"]).to(DEV)
        tab = torch.from_numpy(table).to(DEV)
        out = ops.triplane_fwd(x, tab, lv).cpu().numpy()
        assert np.array_equal(out.view(np.uint32), fix[t + "_out"].view(np.uint32))
        g = ops.triplane_bwd(x, dout, tab, lv, torch.zeros_like(tab)).cpu().double()
        ref = torch.zeros_like(g)
        ref[torch.from_numpy(fix[t + "_grad_idx"])] = torch.from_numpy(fix[t + "_grad_taichi"]).double()
        assert torch.allclose(g, ref, rtol=1e-5, atol=1e-6)
        half = torch.zeros_like(g)
        half[torch.from_numpy(fix[t + "_grad_idx"])] = torch.from_numpy(fix[t + "_grad_module"]).double() / 2
        assert torch.allclose(g, half, rtol=1e-5, atol=1e-6)


def _march_batch(lego_bitfield, n_rays=2048):
    from ngp_hip import ops, synthetic
    o, d = synthetic.lego_rays(n_rays, seed=5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    hits = ops.ray_aabb(t(o), t(d), 0.5)
    noise = t(np.random.default_rng(1).random(n_rays, dtype=np.float32))
    _, xyzs, *_ = ops.march_train(t(o), t(d), hits, t(lego_bitfield), noise, 1, 0.5, 0.0, 128, 1024)
    return xyzs.contiguous()


@pytest.mark.parametrize("max_res", [1024, 4096])
def test_ray_ordered_batch(hip_lib, lego_bitfield, max_res):
    """Samples of ops.march_train (ray order: runs of shared cells), with the (x - lo) / (hi - lo) normalisation in the kernel."""
    from ngp_hip import ops
    xyzs = _march_batch(lego_bitfield)
    n = xyzs.shape[0]
    assert n > 10000
    res = tr.resolutions(16, max_res, 8)
    table = _table(max_res, 7)
    lv = ops.make_triplane_levels(16, max_res, 8, 4)
    tab = table.to(DEV)
    got = ops.triplane_fwd(xyzs, tab, lv, -0.5, 0.5).cpu().numpy()
    xn = xyzs.cpu().numpy()
    x01 = (xn - np.float32(-0.5)) / (np.float32(0.5) - np.float32(-0.5))
    assert np.array_equal(got.view(np.uint32), tr.forward(x01, table.numpy(), max_res, res).view(np.uint32))
    dout = torch.randn(n, 32, generator=torch.Generator().manual_seed(3))
    dout[::5] = 0.0                                                  # rows that contribute nothing
    g = ops.triplane_bwd(xyzs, dout.to(DEV), tab, lv, torch.zeros_like(tab), -0.5, 0.5).cpu()
    _check_grad(g, *tr.backward(x01, dout.numpy(), table.numpy(), max_res, res))


def test_backward_hot_spot_and_zero_rows(hip_lib):
    """65 536 samples inside ONE level-0 cell (every lane of every wave on the same entries), plus the top-level collision."""
    from ngp_hip import ops
    max_res = 1024
    res = tr.resolutions(16, max_res, 8)
    rng = np.random.default_rng(11)
    x = (np.float32(0.40) + rng.random((65536, 3), dtype=np.float32) * np.float32(0.03)).astype(np.float32)   # level 0: g = 6
    x[:512] = rng.random((512, 3), dtype=np.float32) * np.float32(1.4 / 1023)     # the top level's grid points 0 and 1 share entry 0
    table = _table(max_res, 3)
    lv = ops.make_triplane_levels(16, max_res, 8, 4)
    dout = rng.normal(0, 1, (65536, 32)).astype(np.float32)
    dout[1000:3000] = 0.0
    xt, tab = torch.from_numpy(x).to(DEV), table.to(DEV)
    g = ops.triplane_bwd(xt, torch.from_numpy(dout).to(DEV), tab, lv, torch.zeros_like(tab)).cpu()
    _check_grad(g, *tr.backward(x, dout, table.numpy(), max_res, res))
    # all-zero dout: nothing is written
    z = ops.triplane_bwd(xt, torch.zeros(65536, 32, device=DEV), tab, lv, torch.zeros_like(tab))
    assert int(torch.count_nonzero(z)) == 0


class TorchTriPlane(torch.nn.Module):
    """Pure-torch restatement of the encoder (autograd gives the true gradient): the drop-in reference for the module tests."""

    def __init__(self, enc):
        super().__init__()
        self.plane_embedding = torch.nn.Parameter(enc.plane_embedding.detach().clone())
        self.max_res, self.res, self.out_dim = enc.max_res, tr.resolutions(16, enc.max_res, 8), 32

    def forward(self, x):
        x = x.float().clamp(0, 1)
        M = self.max_res
        T = self.plane_embedding.view(-1, 4)
        cols = []
        for r in self.res:
            pos = x * float(r - 1) + 0.5
            g = torch.floor(pos)
            fr = pos - g
            w = (1.0 - fr, fr)
            ori = [((g + k) / float(r) * float(M - 1)).to(torch.int64) for k in (0, 1)]
            lf = []
            for p in range(3):
                a, b = p, (p + 1) % 3
                s = 0.0
                for c in range(4):
                    idx = p * M * M + ori[c & 1][:, a] + ori[c >> 1][:, b] * M
                    s = s + (w[c & 1][:, a] * w[c >> 1][:, b])[:, None] * T[idx]
                lf.append(s)
            cols.append(lf[0] * lf[1] * lf[2])
        return torch.stack(cols, 2).reshape(x.shape[0], -1)          # [n, F, L] -> column j*L + level


def _pair(max_res=1024, seed=0):
    from modules.networks import NGP
    torch.manual_seed(seed)
    a = NGP(scale=0.5, pos_encoder_type="triplane", max_res=max_res).to(DEV)
    b = copy.deepcopy(a)
    b.pos_encoder = TorchTriPlane(a.pos_encoder).to(DEV)
    return a, b


def test_module_matches_torch_restatement_under_autocast(hip_lib, lego_bitfield):
    a, b = _pair()
    xyzs = _march_batch(lego_bitfield, 2048)
    d = torch.nn.functional.normalize(torch.randn_like(xyzs), dim=1)
    outs = []
    for m in (a, b):
        m.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            s, c = m(xyzs, d)
            loss = (s.float() * 1e-2).sum() + c.float().square().sum()
        loss.backward()
        outs.append((s.float(), c.float(), m.pos_encoder.plane_embedding.grad, [w.grad for w in m._mlp_weights()]))
    (sa, ca, ga, wa), (sb, cb, gb, wb) = outs
    torch.testing.assert_close(sa, sb, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(ca, cb, rtol=1e-3, atol=1e-4)
    scale = gb.abs().max()
    assert scale > 0
    assert float((ga - gb).abs().max()) <= 1e-3 * float(scale)
    for x, y in zip(wa, wb):
        torch.testing.assert_close(x, y, rtol=2e-3, atol=1e-3 * float(y.abs().max()))


def test_fused_occupancy_update_matches_torch_formulation(hip_lib, monkeypatch):
    from modules.networks import NGP
    torch.manual_seed(0)
    m_a = NGP(scale=0.5, pos_encoder_type="triplane", max_res=1024).cuda()
    with torch.no_grad():
        m_a.density_grid[0, ::7] = -1.0
    m_b = copy.deepcopy(m_a)
    monkeypatch.setattr(torch, "rand", lambda *a, **k: torch.full(a if not isinstance(a[0], (tuple, list)) else tuple(a[0]), 0.5,
                                                                  device=k.get("device")))
    monkeypatch.setattr(torch, "rand_like", lambda x, *a, **k: torch.full_like(x, 0.5))
    with torch.autocast("cuda", dtype=torch.float16):
        monkeypatch.setenv("NGP_FUSED_OCCUPANCY", "1")
        m_a.update_density_grid(0.01, warmup=True)
        monkeypatch.setenv("NGP_FUSED_OCCUPANCY", "0")
        m_b.update_density_grid(0.01, warmup=True)
    assert getattr(m_a, "_occ_updater", None) is not None and m_a._occ_updater.triplane
    assert (m_a.density_grid[0, ::7] == -1).all()
    torch.testing.assert_close(m_a.density_grid, m_b.density_grid, rtol=2e-3, atol=1e-4)
    agree = (m_a.density_bitfield == m_b.density_bitfield).float().mean().item()
    assert agree > 0.995, agree


def _train(model, steps, seed=3):
    """train.py's loop shape: render + compat FusedAdam + GradScaler under autocast(fp16), on the trained-Lego occupancy grid."""
    import sys
    compat = os.path.join(ROOT, "taichi-nerfs_amd", "compat")
    if compat not in sys.path:
        sys.path.insert(0, compat)
    from apex.optimizers import FusedAdam
    from modules.rendering import render
    from ngp_hip import synthetic
    torch.manual_seed(seed)
    bits = np.load(os.path.join(GOLDEN, "lego_density_bitfield.npz"))["density_bitfield"]
    model.density_bitfield.copy_(torch.from_numpy(bits).to(DEV))
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
            res = render(model, o, d, exp_step_factor=0.0)
            loss = torch.nn.functional.mse_loss(res["rgb"], target)
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss))
    return np.array(losses)


def test_training_trajectory_matches_torch_encoder(hip_lib):
    a, b = _pair(seed=5)
    la, lb = _train(a, 32), _train(b, 32)
    assert np.all(np.isfinite(la)) and la[-1] < la[0]
    rel = np.abs(la - lb) / np.abs(lb)
    assert rel.max() < 2e-3, rel


def test_fused_trainer_refuses_triplane(hip_lib):
    from modules.networks import NGP
    from ngp_hip.trainer import FusedTrainer
    m = NGP(scale=0.5, pos_encoder_type="triplane", max_res=1024).to(DEV)
    with pytest.raises(ValueError, match="drop-in"):
        FusedTrainer(m)


def test_example_trains_with_triplane(tmp_path):
    spec = importlib.util.spec_from_file_location("train_reference_shape", os.path.join(ROOT, "examples", "train_reference_shape.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--max_steps", "300", "--wh", "200", "--n_train", "12", "--n_test", "2", "--val_dir", str(tmp_path / "results"),
                    "--out", str(tmp_path / "run.json"), "--encoder_type", "triplane"])
    assert out["log(elapsed_s,step,psnr,loss,rays,rm_s,vr_s)"][0][1] == 0
    print("triplane example: test_psnr_avg %.2f dB, %.0f rays/s" % (out["test_psnr_avg"], out["train_rays_per_sec"]))
    assert out["test_psnr_avg"] > 20.0, out
