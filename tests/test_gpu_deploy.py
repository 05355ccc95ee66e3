"""ngp_deploy_shade and the deployment renderer on the GPU, against the reference's own run (tests/golden/ref_deploy.npz, made by
scripts/gen_golden_deploy.py), the numpy restatement (tests/deploy_reference.py) and the training modules."""
import importlib.util
import os

import numpy as np
import pytest

import deploy_reference as dr
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "ref_deploy.npz")))


@pytest.fixture(scope="module")
def dev(hip_lib):
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model(fx, tag, amplitude, bits):
    from ngp_hip.deploy import DeployedModel
    return DeployedModel(dr.synthetic_table(amplitude), fx["sigma_weights_" + tag], fx["rgb_weights_" + tag], bits, poses=fx["pose"][None],
                         per_level_scale=float(fx["per_level_scale"]))


@pytest.fixture(scope="module")
def image_model(fx, dev, lego_bitfield):
    return _model(fx, "syn", float(fx["img_table_amplitude"]), lego_bitfield)


def test_embedding_equals_the_training_encoder_and_the_reference(fx, dev, lego_bitfield):
    """enc_out is ops.hash_fwd_f32 on x01 = xyz + 0.5 bit for bit (same table, same level struct), and the reference's embedding bit for
    bit on every level whose scale the library's host expf and the reference's f32 exp agree on.  Where they differ in the last place
    (level 1, profiles/PARITY_NOTES.md) the trilinear interpolant moves by at most 6 A |d scale| (three axes, a slope of at most 2 A per
    axis for table values in [-A, A], x01 <= 1) plus rounding."""
    import torch
    from ngp_hip import ops
    m = _model(fx, "syn", float(fx["rows_table_amplitude"]), lego_bitfield)
    rng = np.random.default_rng(3)
    xyz = np.concatenate([fx["rows_xyz"], (rng.random((20000, 3), dtype=np.float32) - np.float32(0.5))])
    d = np.concatenate([fx["rows_dirs"], rng.normal(0, 1, (20000, 3)).astype(np.float32)])
    sig, rgb, enc = m.shade(_t(xyz, dev), _t(d, dev), return_enc=True)
    x01 = (_t(xyz, dev) + 0.5).contiguous()
    want = ops.hash_fwd_f32(x01, m._tensors()[0], m.levels)
    assert want.shape == (len(xyz), 16) and torch.equal(enc.view(torch.int32), want.view(torch.int32))
    scale = ops.levels_to_numpy(m.levels)[0]
    got = enc[:len(fx["rows_xyz"])].cpu().numpy()
    A = float(fx["rows_table_amplitude"])
    for l in range(4):
        g, r = got[:, 4 * l:4 * l + 4], fx["rows_enc"][:, 4 * l:4 * l + 4]
        if scale[l].view(np.uint32) == fx["level_scale"][l].view(np.uint32):
            assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), "level %d" % l
        else:
            bound = 6 * A * abs(float(scale[l]) - float(fx["level_scale"][l])) + 16 * np.finfo(np.float32).eps * A
            print("level %d: scale %r vs the reference's %r, embedding differs by %.3e (bound %.3e)" % (
                l, scale[l], fx["level_scale"][l], np.abs(g - r).max(), bound))
            assert np.abs(g - r).max() <= bound


@pytest.mark.parametrize("tag", ["lego", "syn"])
def test_sigma_rgb_rows(fx, dev, lego_bitfield, tag):
    """Every row of the fixture, both weight sets: sigma relative, rgb absolute, at 4x the reference's own distance from float64."""
    m = _model(fx, tag, float(fx["rows_table_amplitude"]), lego_bitfield)
    sig, rgb = m.shade(_t(fx["rows_xyz"], dev), _t(fx["rows_dirs"], dev))
    sig, rgb = sig.cpu().numpy().astype(np.float64), rgb.cpu().numpy().astype(np.float64)
    es = np.abs(sig / fx["rows_sigma_" + tag].astype(np.float64) - 1).max()
    ec = np.abs(rgb - fx["rows_rgb_" + tag]).max()
    print("%s: kernel vs reference: sigma rel %.3e (bound %.1e) rgb abs %.3e (bound %.1e)" % (tag, es, dr.BOUNDS[tag][0], ec, dr.BOUNDS[tag][1]))
    assert sig.shape == (len(fx["rows_xyz"]),) and np.isfinite(sig).all() and np.isfinite(rgb).all()
    assert es <= dr.BOUNDS[tag][0] and ec <= dr.BOUNDS[tag][1]


def test_box_faces_and_outside_follow_the_modulo_rule(fx, dev, lego_bitfield):
    """Positions on the faces (all six, the z = +0.5 face the reference's kernel cannot do included), on edges and corners, just outside
    and far outside: every output finite and the embedding that of the modulo rule's restatement bit for bit (an index past a level or
    past the table would show there).  sigma / rgb are held to the row bounds on the box itself (x01 in [0, 1], where those bounds were
    measured); outside, the trilinear weights leave [0, 1] and the embedding grows, so only the embedding is compared there."""
    m = _model(fx, "syn", 1.0, lego_bitfield)
    rng = np.random.default_rng(11)
    base = rng.random((64, 3), dtype=np.float32) - np.float32(0.5)
    pts = []
    for ax in range(3):
        for v in (-0.5, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(-0.5), np.float32(-1)), 0.5001, -0.5001,
                  0.51, -0.53):
            p = base[:8].copy(); p[:, ax] = v; pts.append(p)
    pts.append(np.array([[0.5, 0.5, 0.5], [-0.5, -0.5, -0.5], [0.5, -0.5, 0.5], [0.5, 0.5, -0.5], [0.5000001, 0.5000001, 0.5000001],
                         [3.0, 2.5, 2.0], [1e6, 0.0, 0.0]], np.float32))                  # far outside: the indices wrap, nothing else
    xyz = np.concatenate(pts).astype(np.float32)
    d = rng.normal(0, 1, xyz.shape).astype(np.float32)
    sig, rgb, enc = (t.cpu().numpy() for t in m.shade(_t(xyz, dev), _t(d, dev), return_enc=True))
    from ngp_hip import ops
    levels = (ops.levels_to_numpy(m.levels)[0],) + dr.level_table()[1:]
    want_enc, want_sig, want_rgb = dr.shade(xyz, d, m.hash_table, levels, m.sigma_weights, m.rgb_weights)
    assert np.isfinite(sig).all() and np.isfinite(rgb).all() and np.isfinite(enc).all()
    assert np.array_equal(enc.view(np.uint32), want_enc.view(np.uint32))
    box = (np.abs(xyz) <= 0.5).all(1)
    assert box.sum() >= 3 * 2 * 8 + 4 and (~box).sum() >= 3 * 6 * 8
    es = np.abs(sig[box] / want_sig[box].astype(np.float64) - 1).max()
    ec = np.abs(rgb[box] - want_rgb[box]).max()
    print("faces: sigma rel %.3e rgb abs %.3e on %d box points, %d points outside" % (es, ec, box.sum(), (~box).sum()))
    assert es <= dr.BOUNDS["syn"][0] and ec <= dr.BOUNDS["syn"][1]


def test_progressive_reproduces_the_reference_image(fx, image_model):
    w, h = (int(v) for v in fx["img_res_wh"])
    out = image_model.render(fx["pose"], res=(w, h), T_threshold=float(fx["img_T_threshold"]), max_samples=int(fx["img_max_samples"]),
                             mode="progressive")
    assert out["schedule"] == [tuple(r) for r in fx["img_schedule"].tolist()]
    assert int(out["total_samples"]) == int(fx["img_total_samples"])
    assert np.array_equal(np.sort(out["alive"].cpu().numpy()), fx["img_alive_at_end"])
    ec = np.abs(out["rgb"].cpu().numpy() - fx["img_rgb"]).max()
    eo = np.abs(out["opacity"].cpu().numpy() - fx["img_opacity"]).max()
    print("progressive vs the reference: rgb %.3e opacity %.3e" % (ec, eo))
    assert ec <= 1e-3 and eo <= 1e-3


def test_oneshot_agrees_where_progressive_finished(fx, image_model):
    """One-shot and progressive differ only for rays that exhausted the reference's round budget: every other ray (ended by
    T_threshold, or left the box) agrees within 1e-3; the rays that differ are counted and must be among the exhausted ones."""
    w, h = (int(v) for v in fx["img_res_wh"])
    kw = dict(res=(w, h), T_threshold=float(fx["img_T_threshold"]))
    prog = image_model.render(fx["pose"], max_samples=int(fx["img_max_samples"]), mode="progressive", **kw)
    one = image_model.render(fx["pose"], **kw)
    exhausted = np.zeros(w * h, bool)
    exhausted[prog["alive"].cpu().numpy()] = True
    err = np.maximum(np.abs(one["rgb"].cpu().numpy() - prog["rgb"].cpu().numpy()).max(1),
                     np.abs(one["opacity"].cpu().numpy() - prog["opacity"].cpu().numpy()))
    differ = err > 1e-3
    print("one-shot vs progressive: %d rays exhausted the budget, %d of them differ (max %.3e); finished rays differ by at most %.3e"
          % (exhausted.sum(), differ.sum(), err.max(), err[~exhausted].max()))
    assert exhausted.sum() == len(fx["img_alive_at_end"]) >= 1
    assert err[~exhausted].max() <= 1e-3
    assert not (differ & ~exhausted).any() and differ.sum() >= 1


def _example():
    spec = importlib.util.spec_from_file_location("render_deployment_example", os.path.join(ROOT, "examples", "render_deployment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_save_export_load_render(dev, tmp_path):
    """train.py's deployment configuration trains on the procedural scene through the drop-in modules (the loss falls); the trained model
    renders the same image bit for bit from the live module, from deployment.npy and from fp32 blobs; and that image is the training
    renderer's own test-time image (fp32, no autocast, same T_threshold and cap, same white background) within 1e-3."""
    import torch
    from modules.rendering import render
    from modules.utils import save_deployment_model
    from ngp_hip.deploy import DeployedModel
    from ngp_hip.export import export_deployment_bins
    from ngp_hip.rays import get_rays
    ex = _example()
    model, poses, dirs, losses = ex.train_deployment_model(400, dev, wh=64, n_views=24, batch=4096)
    first, last = float(losses[:20].mean()), float(losses[-20:].mean())
    print("deployment configuration: loss %.5f -> %.5f over %d steps" % (first, last, len(losses)))
    assert np.isfinite(losses).all() and last < first
    model.eval()

    class Data:
        pass
    Data.poses = poses
    save_deployment_model(model, Data, tmp_path)
    export_deployment_bins(str(tmp_path / "deployment.npy"), tmp_path / "bins", dtype=np.float32, pose_index=3)
    a = DeployedModel.from_module(model)
    b = DeployedModel.from_npy(str(tmp_path / "deployment.npy"))
    c = DeployedModel.from_bins(tmp_path / "bins")
    assert np.array_equal(c.poses[0], poses[3].cpu().numpy())
    pose = poses[3]
    outs = [m.render(pose, directions=dirs, T_threshold=1e-2, max_samples=1024) for m in (a, b, c)]
    for o in outs[1:]:
        for k in ("rgb", "opacity", "depth"):
            assert torch.equal(o[k].view(torch.int32), outs[0][k].view(torch.int32)), k
        assert int(o["total_samples"]) == int(outs[0]["total_samples"])
    rays_o, rays_d = get_rays(dirs, pose)
    with torch.no_grad():
        ref = render(model, rays_o, rays_d, test_time=True, exp_step_factor=0, T_threshold=1e-2, max_samples=1024)
    mine = outs[0]["rgb"] + (1 - outs[0]["opacity"])[:, None]                    # over the white background render() uses
    ec = (mine - ref["rgb"].float()).abs().max().item()
    eo = (outs[0]["opacity"] - ref["opacity"]).abs().max().item()
    print("deployed render vs modules.rendering.render: rgb %.3e opacity %.3e, %d samples, mean opacity %.3f"
          % (ec, eo, int(outs[0]["total_samples"]), outs[0]["opacity"].mean().item()))
    assert outs[0]["opacity"].max().item() > 0.5 and abs(int(outs[0]["total_samples"]) - int(ref["total_samples"])) <= 1e-3 * int(ref["total_samples"])
    assert ec <= 1e-3 and eo <= 1e-3


@pytest.mark.parametrize("res", [(300, 600), (800, 800)])
def test_full_size_renders_are_finite_and_deterministic(fx, image_model, res):
    import torch
    a = image_model.render(fx["pose"], res=res)
    b = image_model.render(fx["pose"], res=res)
    n = res[0] * res[1]
    assert a["rgb"].shape == (n, 3) and a["opacity"].shape == (n,) and a["depth"].shape == (n,)
    for k in ("rgb", "opacity", "depth"):
        assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), k
    assert int(a["total_samples"]) == int(b["total_samples"]) > n // 4
    assert (a["opacity"] > 0).float().mean().item() > 0.2
    p = image_model.render(fx["pose"], res=res, mode="progressive")
    assert torch.isfinite(p["rgb"]).all() and p["rgb"].shape == (n, 3)
