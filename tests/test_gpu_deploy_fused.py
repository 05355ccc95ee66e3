"""ngp_deploy_render and DeployedModel.render(mode="fused") on the GPU against the serial float64 reference of
tests/deploy_render_reference.py: per ray the composited-sample count, the t of the last composited sample bit for bit (the CPU oracle's
sample) and rgb / opacity / depth within BOUNDS.  Every direct call writes into outputs pre-filled with NaN that have guard rows behind
them."""
import ctypes

import numpy as np
import pytest

import deploy_reference as dr
import deploy_render_reference as rr

pytestmark = pytest.mark.gpu

GUARD = 67            # rows behind every output that no launch may touch
SENTINEL = -123456    # the int32 output's pre-fill


@pytest.fixture(scope="module")
def dev(hip_lib):
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def levels(hip_lib):
    from ngp_hip import ops
    return ops.make_levels(2**21, 4, 32, 128, 4)


@pytest.fixture(scope="module")
def scenes(oracle, lego_bitfield, levels):
    from ngp_hip import ops
    scale = ops.levels_to_numpy(levels)[0]
    return lambda name: rr.scene(name, oracle, lego_bitfield, scale)


@pytest.fixture(scope="module")
def on_device(dev):
    """Device copies of a scene's model, one per table / bitfield."""
    import torch
    from ngp_hip import ops
    cache = {}

    def get(sc):
        key = (id(sc.table), sc.bitfield[:4096].tobytes(), int(sc.bitfield.sum()))
        if key not in cache:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            bits = t(sc.bitfield)
            cache[key] = dict(table=t(sc.table), sigma_w=t(sc.sigma_w), rgb_w=t(sc.rgb_w), density_bitfield=bits,
                              coarse=ops.coarse_bitfield(bits, 1, 128))
        return cache[key]
    return get


def _outputs(n, dev):
    """NaN-filled (the counts: SENTINEL) outputs of n rays with GUARD rows behind them -> (the views a launch gets, the whole buffers)."""
    import torch
    full = (torch.full((n + GUARD, 3), float("nan"), device=dev), torch.full((n + GUARD,), float("nan"), device=dev),
            torch.full((n + GUARD,), float("nan"), device=dev), torch.full((n + GUARD,), SENTINEL, device=dev, dtype=torch.int32),
            torch.full((n + GUARD,), float("nan"), device=dev))
    return tuple(f[:n] for f in full), full


def _untouched(full, n):
    import torch
    return all(bool(torch.isnan(f[n:]).all()) if f.is_floating_point() else bool((f[n:] == SENTINEL).all()) for f in full)


def _launch(sc, model, levels, dev, n, thr, cap=rr.MAX_SAMPLES, order=None, coarse=True):
    """ngp_deploy_render (through ops.deploy_render) on the first n rays of a scene, optionally reordered -> numpy outputs; asserts
    that every ray was written and no guard row was."""
    import torch
    from ngp_hip import ops
    idx = np.arange(n) if order is None else order
    o = torch.from_numpy(np.ascontiguousarray(sc.rays_o[idx])).to(dev)
    d = torch.from_numpy(np.ascontiguousarray(sc.rays_d[idx])).to(dev)
    out, full = _outputs(n, dev)
    got = ops.deploy_render(o, d, model["density_bitfield"], model["coarse"] if coarse else None, model["table"], levels, model["sigma_w"],
                            model["rgb_w"], thr, cap, out=out)
    torch.cuda.synchronize()
    assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, out))
    assert _untouched(full, n), "a guard row was written"
    res = [g.cpu().numpy() for g in got]
    assert all(np.isfinite(r).all() for r in res) and (res[3] >= 0).all(), "a ray's outputs were not written"
    return res


def _compare(sc, got, n, thr, cap, bounds, what):
    """The first n rays against the float64 reference; near-tie rays (at most 1 %) are left out of every comparison."""
    ref = [a[:n] for a in sc.composite(thr, cap, np.float64)]
    tie = ref[5] < rr.TIE
    assert tie.mean() <= rr.TIE_SHARE, "the reference excludes %d of %d rays" % (tie.sum(), n)
    keep = ~tie
    rgb, op, dep, cnt, t_last = got
    assert np.array_equal(cnt[keep], ref[3][keep]), "%s: composited-sample counts differ on %d rays" % (what, (cnt[keep] != ref[3][keep]).sum())
    assert np.array_equal(t_last[keep].view(np.uint32), ref[4][keep].view(np.uint32)), what
    assert (cnt <= cap).all()
    none = ref[3] == 0
    assert not rgb[none].any() and not op[none].any() and not dep[none].any() and not t_last[none].any()      # a miss: zeros
    if bounds is not None and keep.any():
        err = [np.abs(g[keep].astype(np.float64) - r[keep]).max() for g, r in zip((rgb, op, dep), ref[:3])]
        print("%s: %d rays (%d near ties left out), %d composited samples: rgb %.3e opacity %.3e depth %.3e = %.2f %.2f %.2f of the bounds"
              % (what, n, tie.sum(), cnt.sum(), err[0], err[1], err[2], err[0] / bounds[0], err[1] / bounds[1], err[2] / bounds[2]))
        assert err[0] <= bounds[0] and err[1] <= bounds[1] and err[2] <= bounds[2]
    return ref


# ---------------------------------------------------------------------------------------------------- 1  the fixture image
@pytest.mark.parametrize("thr", [1e-2, 0.3])
def test_fixture_image(scenes, on_device, levels, dev, lego_bitfield, thr):
    """24x48, max_samples 1024: the kernel on the image's rays, and DeployedModel.render(mode="fused") bit-identical to it."""
    import torch
    from ngp_hip.deploy import DeployedModel
    sc = scenes("image")
    n = sc.rays_o.shape[0]
    got = _launch(sc, on_device(sc), levels, dev, n, thr)
    ref = _compare(sc, got, n, thr, rr.MAX_SAMPLES, rr.BOUNDS[("image", thr)], "fixture image, T_threshold %g" % thr)
    assert (ref[3] < sc.marched).sum() >= 50                                       # rays that end by the threshold, not by the box
    fx = rr.fixture()
    w, h = (int(v) for v in fx["img_res_wh"])
    m = DeployedModel(sc.table, sc.sigma_w, sc.rgb_w, lego_bitfield, per_level_scale=float(fx["per_level_scale"]))
    out = m.render(fx["pose"], res=(w, h), T_threshold=thr, mode="fused")
    assert sorted(out) == ["depth", "n_samples", "opacity", "rgb", "total_samples"]
    assert out["total_samples"].dtype == torch.int64 and out["total_samples"].is_cuda and out["n_samples"].dtype == torch.int32
    assert int(out["total_samples"]) == int(got[3].sum()) == int(out["n_samples"].sum())
    for k, g in (("rgb", got[0]), ("opacity", got[1]), ("depth", got[2]), ("n_samples", got[3])):
        assert np.array_equal(out[k].cpu().numpy().view(np.uint32), g.view(np.uint32)), k


# ---------------------------------------------------------------------------------------------------- 2  batch shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1153])
def test_batch_shapes(scenes, on_device, levels, dev, n):
    """A list that mixes rays into the box, misses, rays that start inside it and rays with zero direction components: the first n."""
    import torch
    from ngp_hip import ops
    sc = scenes("list")
    hits = ops.ray_aabb(torch.from_numpy(sc.rays_o[:n]).to(dev), torch.from_numpy(sc.rays_d[:n]).to(dev), rr.SCALE).cpu().numpy()
    assert np.array_equal(hits.view(np.uint32), sc.hits[:n].view(np.uint32))      # the slab test both sides start from, zero components included
    got = _launch(sc, on_device(sc), levels, dev, n, 1e-2)
    _compare(sc, got, n, 1e-2, rr.MAX_SAMPLES, rr.BOUNDS[("list", 1e-2)], "ray list, first %d" % n)
    if n == 1153:
        zero, miss = (sc.rays_d == 0).any(1), sc.hits[:, 0] < 0
        assert (got[3][zero] > 0).sum() >= 50 and (got[3][zero & miss] == 0).all() and (got[3][miss] == 0).all()
        without = _launch(sc, on_device(sc), levels, dev, n, 1e-2, coarse=False)    # no coarse table: the same result from the bitfield alone
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, without))


# ---------------------------------------------------------------------------------------------------- 3  the cap
@pytest.mark.parametrize("cap", [1, 7, 64])
def test_max_samples_caps_the_ray(scenes, on_device, levels, dev, cap):
    sc = scenes("image")
    n = sc.rays_o.shape[0]
    got = _launch(sc, on_device(sc), levels, dev, n, 1e-2, cap=cap)
    ref = _compare(sc, got, n, 1e-2, cap, None, "cap %d" % cap)
    assert got[3].max() == cap == ref[3].max() and (got[3] == cap).sum() >= 100


# ---------------------------------------------------------------------------------------------------- 4  bitfield extremes
def test_empty_bitfield_gives_zeros(scenes, on_device, levels, dev):
    sc = scenes("zeros")
    n = sc.rays_o.shape[0]
    for coarse in (True, False):
        got = _launch(sc, on_device(sc), levels, dev, n, 1e-2, coarse=coarse)
        assert all(not g.any() for g in got)
    _compare(sc, got, n, 1e-2, rr.MAX_SAMPLES, None, "all-zero bitfield")


def test_full_bitfield_samples_every_orbit_point(scenes, on_device, levels, dev):
    """Every orbit point inside the box is a sample: the longest rays reach the cap of 1024."""
    sc = scenes("ones")
    n = sc.rays_o.shape[0]
    got = _launch(sc, on_device(sc), levels, dev, n, 1e-2)
    _compare(sc, got, n, 1e-2, rr.MAX_SAMPLES, rr.BOUNDS[("ones", 1e-2)], "all-ones bitfield")
    assert got[3].max() == rr.MAX_SAMPLES and (got[3] == rr.MAX_SAMPLES).sum() >= 10 and np.array_equal(got[3], sc.marched)


# ---------------------------------------------------------------------------------------------------- 5  order independence
def test_outputs_do_not_depend_on_the_order_of_the_rays(scenes, on_device, levels, dev):
    sc = scenes("image")
    n = sc.rays_o.shape[0]
    a = _launch(sc, on_device(sc), levels, dev, n, 0.3)
    b = _launch(sc, on_device(sc), levels, dev, n, 0.3)
    perm = np.random.default_rng(41).permutation(n)
    c = _launch(sc, on_device(sc), levels, dev, n, 0.3, order=perm)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))                # two runs
        assert np.array_equal(x[perm].view(np.uint32), z.view(np.uint32))          # the permuted rays give the permuted outputs


# ---------------------------------------------------------------------------------------------------- 6  against one-shot
def test_fused_agrees_with_oneshot(scenes, lego_bitfield, dev):
    """128x128 rays: the chain of separately pinned operators (march, shade, composite) and the one launch, within the bar the project
    holds its render paths to."""
    from ngp_hip.deploy import DeployedModel
    sc = scenes("image")
    fx = rr.fixture()
    m = DeployedModel(sc.table, sc.sigma_w, sc.rgb_w, lego_bitfield, per_level_scale=float(fx["per_level_scale"]))
    one = m.render(fx["pose"], res=(128, 128))
    fused = m.render(fx["pose"], res=(128, 128), mode="fused")
    ec = (one["rgb"] - fused["rgb"]).abs().max().item()
    eo = (one["opacity"] - fused["opacity"]).abs().max().item()
    t1, tf = int(one["total_samples"]), int(fused["total_samples"])
    print("fused vs one-shot, 128x128: rgb %.3e opacity %.3e, composited samples %d vs %d" % (ec, eo, tf, t1))
    assert fused["rgb"].shape == (128 * 128, 3) and t1 > 128 * 128
    assert ec <= 1e-3 and eo <= 1e-3 and abs(tf - t1) <= 1e-3 * t1


# ---------------------------------------------------------------------------------------------------- 7  loaders
def test_loaders_render_bit_identically(dev, tmp_path):
    import torch
    from ngp_hip.deploy import DeployedModel
    from ngp_hip.export import export_deployment_bins
    rng = np.random.default_rng(77)
    d = {'poses': rr.fixture()["pose"].astype(np.float32).reshape(1, 3, 4),
         'model.density_bitfield': rng.integers(0, 256, dr.BITFIELD_BYTES, dtype=np.uint8) & rng.integers(0, 256, dr.BITFIELD_BYTES, dtype=np.uint8),
         'model.hash_encoder.params': rng.uniform(-1, 1, dr.TOTAL_ENTRIES * 4).astype(np.float32), 'model.per_level_scale': dr.LOG_B,
         'model.xyz_encoder.params': rng.normal(0, 0.5, 512).astype(np.float32), 'model.rgb_net.params': rng.normal(0, 0.5, 768).astype(np.float32)}
    np.save(tmp_path / "deployment.npy", d)
    export_deployment_bins(d, tmp_path / "bins", dtype=np.float32)
    models = (DeployedModel.from_npy(str(tmp_path / "deployment.npy")), DeployedModel.from_bins(tmp_path / "bins"),
              DeployedModel(d['model.hash_encoder.params'], d['model.xyz_encoder.params'], d['model.rgb_net.params'], d['model.density_bitfield']))
    outs = [m.render(d['poses'][0], res=(24, 48), mode="fused") for m in models]
    assert int(outs[0]["total_samples"]) > 1000
    for o in outs[1:]:
        for k in ("rgb", "opacity", "depth", "n_samples"):
            assert torch.equal(o[k].view(torch.int32), outs[0][k].view(torch.int32)), k
        assert int(o["total_samples"]) == int(outs[0]["total_samples"])


# ---------------------------------------------------------------------------------------------------- 8  validation
def test_bad_arguments_launch_nothing(hip_lib, scenes, on_device, levels, dev):
    """A wrong level table, max_samples = 0, a table pointer off by 4 bytes and a null pointer: -1 from the C entry, ValueError from the
    operator, and the NaN-filled outputs stay as they were."""
    import torch
    from ngp_hip import ops
    sc = scenes("image")
    m = on_device(sc)
    n = 100
    o, d = torch.from_numpy(sc.rays_o[:n]).to(dev), torch.from_numpy(sc.rays_d[:n]).to(dev)
    out, full = _outputs(n, dev)
    wrong = ops.make_levels(2**19, 16, 16, 1024, 2)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(table_ptr=None, lv=levels, cap=1024, rgb_ptr=None):
        return hip_lib.ngp_deploy_render(P(o), P(d), P(m["density_bitfield"]), P(m["coarse"]), P(m["table"]) if table_ptr is None else table_ptr,
                                         ctypes.byref(lv), P(m["sigma_w"]), P(m["rgb_w"]), n, cap, 1e-2, P(out[0]) if rgb_ptr is None else rgb_ptr,
                                         P(out[1]), P(out[2]), P(out[3]), P(out[4]), None)
    assert call(lv=wrong) == -1 and call(cap=0) == -1 and call(cap=-5) == -1
    assert call(table_ptr=ctypes.c_void_p(m["table"].data_ptr() + 4)) == -1
    assert call(rgb_ptr=ctypes.c_void_p(0)) == -1
    assert hip_lib.ngp_deploy_render(P(o), P(d), P(m["density_bitfield"]), None, P(m["table"]), ctypes.byref(levels), P(m["sigma_w"]), P(m["rgb_w"]),
                                     0, 1024, 1e-2, P(out[0]), P(out[1]), P(out[2]), P(out[3]), P(out[4]), None) == 0          # no rays: nothing to do
    kw = dict(rays_o=o, rays_d=d, density_bitfield=m["density_bitfield"], coarse=m["coarse"], table=m["table"], lv=levels, sigma_w=m["sigma_w"],
              rgb_w=m["rgb_w"], out=out)
    for bad in (dict(lv=wrong), dict(max_samples=0), dict(table=torch.zeros(dr.TOTAL_ENTRIES * 4 + 4, device=dev)[1:-3])):
        with pytest.raises(ValueError):
            ops.deploy_render(**dict(kw, **bad))
    torch.cuda.synchronize()
    assert _untouched(full, 0)
    assert call() == 0                                                                                                           # and the good call runs
    torch.cuda.synchronize()
    assert _untouched(full, n) and bool(torch.isfinite(out[0]).all())
