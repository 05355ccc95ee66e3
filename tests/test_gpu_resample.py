"""csrc/resample.hip -- ngp_resample_count / _scan / _write -- against the float64 evaluation of tests/resample_reference.py on its named
sets (sections per ray 0, 1, 63, 64, 65, 129, 1024; K in {1, 7, 64, 65, 128, 256}; 1, 4, 5, 37 rays; all weight in one section; zeros
between weights; negative weights; a floor on an all-zero ray; gaps; permuted ray indices; a NaN ray; rays of 1025 and 1500 sections, whose
CDF the count kernel keeps in global memory instead of LDS; noise exactly 0), through buffers in which
everything the kernels must not touch holds a sentinel; then the operator, an analytic sphere end to end, and render_surface.

Section choice, counts, parent and rays_a' are exact on decided rays (resample_reference.decide); ts, deltas, xyzs are within
4 E32 scale of float64 there; the invariants hold on every ray, decided or not; two launches give the same bits.  Every test prints
what it measured (pytest -s); profiles/PARITY_NOTES.md records the ratios."""
import numpy as np
import pytest
import torch

import resample_reference as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENT = rr.SENTINEL
PAD = 64
SETS = list(rr.case_table())
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent(shape, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), SENT if dtype.is_floating_point else -77, device=DEV, dtype=dtype)


def is_sent(t):
    return bool((t == (SENT if t.dtype.is_floating_point else -77)).all())


class Dev:
    def __init__(self, case, seed):
        self.case, self.lay = case, rr.Layout(case, seed)
        lay = self.lay
        assert lay.rays_a.min() >= 0 and lay.rays_a[:, 0].max() < lay.n_orig and (lay.rays_a[:, 1] + lay.rays_a[:, 2]).max() <= lay.S
        self.t = {k: dev(getattr(lay, k)) for k in ("ws", "deltas", "ts", "rays_a", "rays_o", "rays_d", "noise")}


def device_case(name):
    if name not in _cache:
        _cache[name] = Dev(rr.case_table()[name], sum(map(ord, name)))
    return _cache[name]


def launch(d, n_rays=None, tensors=None):
    """The three launches on sentinel-filled buffers, every output with PAD sentinels in front of and behind it.
    -> (buffers on the device, numpy copies of the outputs, the per-ray split)."""
    from ngp_hip import ops
    L, lay, case, t = ops._lib(), d.lay, d.case, dict(d.t, **(tensors or {}))
    n, K, S, p = (lay.n if n_rays is None else n_rays), case.K, lay.S, ops._ptr
    b = dict(cdf=sent(S + 2 * PAD), stage_t=sent(lay.n * K + 2 * PAD), stage_j=sent(lay.n * K + 2 * PAD, torch.int32),
             counts=sent(lay.n + 2 * PAD, torch.int32), rays_a_out=sent((lay.n + 2 * PAD, 3), torch.int32))
    total = torch.zeros(2, device=DEV, dtype=torch.int32)
    v = lambda name, m: b[name][PAD:PAD + m]
    st = ops._stream()
    ops.check(L.ngp_resample_count(p(t["ws"]), p(t["deltas"]), p(t["ts"]), p(t["rays_a"]), p(t["noise"]), n, lay.n_orig, S, K, case.floor,
                                   p(v("cdf", S)), p(v("stage_t", lay.n * K)), p(v("stage_j", lay.n * K)), p(v("counts", lay.n)), p(total),
                                   st), "count")
    ops.check(L.ngp_resample_scan(p(v("counts", lay.n)), p(t["rays_a"]), n, p(v("rays_a_out", lay.n)), p(total), st), "scan")
    S_out, bad = total.tolist()
    assert bad == 0 and lay.N[:n].sum() <= S_out <= lay.N[:n].sum() + n * K
    b.update(xyzs=sent((S_out + 2 * PAD, 3)), dirs=sent((S_out + 2 * PAD, 3)), deltas=sent(S_out + 2 * PAD), ts=sent(S_out + 2 * PAD),
             parent=sent(S_out + 2 * PAD, torch.int32))
    if S_out:
        ops.check(L.ngp_resample_write(p(t["rays_o"]), p(t["rays_d"]), p(t["deltas"]), p(t["ts"]), p(t["rays_a"]), p(v("rays_a_out", lay.n)),
                                       p(v("stage_t", lay.n * K)), p(v("stage_j", lay.n * K)), n, lay.n_orig, S, K, p(v("xyzs", S_out)),
                                       p(v("dirs", S_out)), p(v("deltas", S_out)), p(v("ts", S_out)), p(v("parent", S_out)), st), "write")
    torch.cuda.synchronize()
    # sentinels: the pads of every buffer, the rows behind n_rays, the CDF of samples no launched ray owns, and no hole in the outputs
    for k, x in b.items():
        m = {"cdf": S, "stage_t": lay.n * K, "stage_j": lay.n * K, "counts": lay.n, "rays_a_out": lay.n}.get(k, S_out)
        assert is_sent(x[:PAD]) and is_sent(x[PAD + m:]), "%s was written outside its buffer" % k
    assert is_sent(v("counts", lay.n)[n:]) and is_sent(v("rays_a_out", lay.n)[n:]) and is_sent(v("stage_t", lay.n * K)[n * K:])
    own = np.zeros(S, bool)
    for r in range(n):
        own[lay.start[r]:lay.start[r] + lay.N[r]] = True
    assert is_sent(v("cdf", S)[dev(~own)]), "the CDF workspace was written outside the rays"
    h = {k: v(k, S_out if k in ("xyzs", "dirs", "deltas", "ts", "parent") else lay.n).cpu().numpy() for k in
         ("xyzs", "dirs", "deltas", "ts", "parent", "counts", "rays_a_out")}
    h["total"] = S_out
    assert not np.any(h["ts"] == F(SENT)) and not np.any(h["parent"] == -77) and not np.any(h["xyzs"] == F(SENT)), "a child was never written"
    ra = h["rays_a_out"][:n]
    assert np.array_equal(ra, np.stack([lay.ray_idx[:n], np.concatenate([[0], np.cumsum(h["counts"][:n])[:-1]]), h["counts"][:n]], 1))
    assert int(h["counts"][:n].sum()) == S_out
    got = lay.split(np.concatenate([ra, np.zeros((lay.n - n, 3), np.int32)]), h["ts"], h["deltas"], h["parent"], h["xyzs"], h["dirs"])[:n]
    return b, h, got


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


@pytest.mark.parametrize("name", SETS)
def test_named_set_against_float64(hip_lib, name):
    d = device_case(name)
    case = d.case
    b, h, got = launch(d)
    assert rr.invariants(case, got) == []
    e32 = rr.case_e32(case)
    fails, worst, judged = rr.judge(case, got, e32)
    ref = case.ref()
    all_decided = all(x[2]["ray_decided"] for x in ref)
    print("resample %s K=%d: %d / %d rays decided, |gpu - f64| / (E32 scale): ts %.3f deltas %.3f xyzs %.3f (E32 %.2e %.2e %.2e)"
          % (name, case.K, judged, len(case.rays), worst["ts"], worst["deltas"], worst["xyzs"], e32["ts"], e32["deltas"], e32["xyzs"]))
    assert fails == [], fails[:5]
    if all_decided:
        assert np.array_equal(h["rays_a_out"], rr.expected_rays_a(d.lay, [len(x[0]["ts"]) for x in ref]))
    else:
        assert case.tie, "only a set whose point is a tie may have undecided rays"
        # judged on its decided part: every decided draw of an undecided ray lands where float64 puts it
        for g, (r64, _, dec) in zip(got, ref):
            want = np.bincount(r64["sec"][dec["decided"] & r64["kept"]], minlength=len(r64["c"]) + 1)[:len(r64["c"])]
            have = np.bincount(g["parent"], minlength=len(r64["c"])) - 1
            assert np.all(have >= want) and have.sum() <= want.sum() + int((~dec["decided"]).sum())
    for g, (r64, _, _) in zip(got, ref):                    # pass-through rays are bit-identical copies
        if r64["passthrough"]:
            assert np.array_equal(g["parent"], np.arange(len(g["ts"])))
    b2, h2, _ = launch(d)                                    # determinism
    for k in ("xyzs", "dirs", "deltas", "ts", "parent", "rays_a_out", "counts"):
        assert same_bits(b[k], b2[k]), k


@pytest.mark.parametrize("m", (1, 4, 5))
def test_ragged_ray_counts(hip_lib, m):
    """The first m rows of the 37-ray set (4 rays per block): the rows behind keep their sentinels (checked in launch), the rows in front
    are what the full launch gives them."""
    d = device_case("rays37")
    _, _, got_m = launch(d, n_rays=m)
    _, _, got = launch(d)
    sub = rr.Case("rays37[:%d]" % m, d.case.rays[:m], d.case.K, d.case.floor)
    assert rr.invariants(sub, got_m) == []
    for a, g in zip(got_m, got[:m]):
        for k in ("ts", "deltas", "parent", "xyzs", "dirs"):
            assert np.array_equal(a[k], g[k]), k


def test_a_nan_ray_changes_no_other_ray(hip_lib):
    d = device_case("nan")
    _, _, got = launch(d)
    ws = d.lay.ws.copy()
    for r, ray in enumerate(d.case.rays):
        if not np.all(np.isfinite(ray.ws)):
            s = slice(d.lay.start[r], d.lay.start[r] + ray.N)
            ws[s] = np.where(np.isfinite(ray.ws), ray.ws, F(0.5))
    _, _, clean = launch(d, tensors=dict(ws=dev(ws)))
    n_bad = 0
    for ray, a, c in zip(d.case.rays, got, clean):
        if np.all(np.isfinite(ray.ws)):
            for k in ("ts", "deltas", "parent", "xyzs", "dirs"):
                assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == F else a[k], c[k].view(np.uint32) if c[k].dtype == F else c[k]), k
        else:
            n_bad += 1
            assert len(a["ts"]) == ray.N and len(c["ts"]) > ray.N       # copied through with the NaN, cut without it
    assert n_bad == 2


def test_the_operator(hip_lib):
    """ops.resample_rays gives the bits of the three launches, and refuses what it cannot run: host tensors, K < 1, a negative floor,
    shapes that do not match, and a rays_a row that points outside the buffers (refused by the count kernel's own check: it follows no
    such row)."""
    import ngp_hip
    from ngp_hip import ops
    assert ngp_hip.resample_rays is ops.resample_rays
    d = device_case("permuted")
    t, case = d.t, d.case
    b, h, _ = launch(d)
    ra, xyzs, dirs, deltas, ts, parent, total = ops.resample_rays(t["ws"], t["deltas"], t["ts"], t["rays_a"], t["rays_o"], t["rays_d"],
                                                                  t["noise"], case.K, case.floor)
    S_out = h["total"]
    assert int(total) == S_out and parent.dtype == torch.int32 and ra.dtype == torch.int32
    for k, x in (("xyzs", xyzs), ("dirs", dirs), ("deltas", deltas), ("ts", ts), ("parent", parent)):
        assert same_bits(b[k][PAD:PAD + S_out], x), k
    assert same_bits(b["rays_a_out"][PAD:PAD + d.lay.n], ra)
    args = [t[k] for k in ("ws", "deltas", "ts", "rays_a", "rays_o", "rays_d", "noise")]
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resample_rays(*[x.cpu() for x in args], 4)
    with pytest.raises(ValueError, match="K must"):
        ops.resample_rays(*args, 0)
    with pytest.raises(ValueError, match="floor"):
        ops.resample_rays(*args, 4, floor=-1.0)
    with pytest.raises(ValueError, match="noise"):
        ops.resample_rays(*args[:6], t["noise"][:-1].contiguous(), 4)
    for col, val in ((0, d.lay.n_orig), (0, -1), (1, d.lay.S), (2, -1)):
        bad = d.lay.rays_a.copy()
        bad[3, col] = val
        with pytest.raises(ValueError, match="outside the buffers"):
            ops.resample_rays(args[0], args[1], args[2], dev(bad), *args[4:], 4)
    # no rays, and rays without samples
    out = ops.resample_rays(t["ws"], t["deltas"], t["ts"], t["rays_a"][:0].contiguous(), t["rays_o"], t["rays_d"], t["noise"], 4)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and int(out[6]) == 0
    z = torch.zeros(0, device=DEV)
    out = ops.resample_rays(z, z, z, torch.zeros(2, 3, device=DEV, dtype=torch.int32), t["rays_o"], t["rays_d"], t["noise"], 4)
    assert out[0].tolist() == [[0, 0, 0], [0, 0, 0]] and out[4].shape == (0,) and int(out[6]) == 0


def _sphere_pass(o, d, xyzs, dirs, deltas, ts, rays_a, inv_s):
    from ngp_hip import ops
    r = torch.linalg.norm(xyzs, dim=1)
    f = (r - 0.3).contiguous()
    cosv = ((dirs * xyzs).sum(1) / r.clamp_min(1e-12)).contiguous()
    s = torch.full((1,), float(inv_s), device=DEV)
    out = ops.surface_composite_fwd(f, cosv, torch.zeros_like(xyzs), deltas, ts, rays_a, s, 1.0, 1e-4)
    return out[1], out[2], out[6]                             # opacity, depth, ws


def test_refinement_sharpens_the_depth_of_a_sphere(hip_lib):
    """A sphere of radius 0.3, 512 rays from outside, 48 equal sections per ray across the box: coarse ws at inv_s = 64, 32 draws, then
    coarse and refined samples composited at inv_s = 512.  The mean |depth - analytic hit distance| over the rays that hit must be
    strictly smaller on the refined samples; the ratio is printed, not promised."""
    from ngp_hip import ops
    rng = np.random.default_rng(11)
    n, N = 512, 48
    o = rng.standard_normal((n, 3))
    o = 0.9 * o / np.linalg.norm(o, axis=1, keepdims=True)
    aim = 0.32 * (rng.random((n, 3)) - 0.5)
    dd = aim - o
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    b = (o * dd).sum(1)
    disc = b * b - ((o * o).sum(1) - 0.09)
    hit = disc > 1e-3
    t_hit = -b - np.sqrt(np.where(hit, disc, 0.0))
    o_t, d_t = dev(o.astype(F)), dev(dd.astype(F))
    hits = ops.ray_aabb(o_t, d_t, 0.5)
    near, far = hits[:, 0], hits[:, 1]
    inside = (far > near) & (near >= 0)
    assert bool(inside[dev(hit)].all())
    step = ((far - near) / N).clamp_min(1e-4)
    ts = (near[:, None] + (torch.arange(N, device=DEV)[None, :] + 0.5) * step[:, None]).reshape(-1).contiguous()
    deltas = step[:, None].expand(n, N).reshape(-1).contiguous()
    rays_a = torch.stack([torch.arange(n), torch.arange(n) * N, torch.full((n,), N)], 1).to(DEV, torch.int32).contiguous()
    dirs = d_t[:, None, :].expand(n, N, 3).reshape(-1, 3).contiguous()
    xyzs = (o_t[:, None, :] + ts.view(n, N, 1) * d_t[:, None, :]).reshape(-1, 3).contiguous()
    _, _, ws = _sphere_pass(o_t, d_t, xyzs, dirs, deltas, ts, rays_a, 64.0)
    noise = dev(rng.random(n).astype(F))
    ra2, xyzs2, dirs2, deltas2, ts2, parent, total = ops.resample_rays(ws, deltas, ts, rays_a, o_t, d_t, noise, 32)
    assert int(total) > n * N and int(total) == ts2.shape[0]
    op_c, dep_c, _ = _sphere_pass(o_t, d_t, xyzs, dirs, deltas, ts, rays_a, 512.0)
    op_f, dep_f, _ = _sphere_pass(o_t, d_t, xyzs2, dirs2, deltas2, ts2, ra2, 512.0)
    m, want = dev(hit), dev(t_hit.astype(F))
    err_c = float((dep_c[m] - want[m]).abs().mean())
    err_f = float((dep_f[m] - want[m]).abs().mean())
    print("resample sphere: %d hit rays, mean |depth - t_hit| coarse %.3e refined %.3e (ratio %.3f), samples %d -> %d"
          % (int(hit.sum()), err_c, err_f, err_f / err_c, n * N, int(total)))
    assert int(hit.sum()) > 100 and err_f < err_c


def _small_model(seed=0):
    from ngp_hip.surface import SDFField
    torch.manual_seed(seed)
    return SDFField(scale=0.5, levels=8, log2_T=14, max_res=256).to(DEV)


def _rays(n, seed=3):
    from ngp_hip import synthetic
    o, d = synthetic.orbit_camera_rays(4, (32, 32), seed=seed)
    pick = np.random.default_rng(seed).permutation(o.shape[0])[:n]
    return dev(o[pick]), dev(d[pick])


def test_render_surface_with_importance_samples(hip_lib, monkeypatch):
    """n_importance = 16 on a fresh field: finite outputs, parent consistent with rm_samples_coarse, a backward that reaches the table,
    both MLPs and log_inv_s.  n_importance = 0 never calls ops.resample_rays (a counter on the operator) and returns today's keys."""
    from ngp_hip import ops
    from ngp_hip.surface import render_surface
    calls = []
    real = ops.resample_rays
    monkeypatch.setattr(ops, "resample_rays", lambda *a, **k: (calls.append(a[7]), real(*a, **k))[1])
    model = _small_model()
    model.update_density_grid(0.01 * 1024 / 3**0.5, warmup=True)
    o, d = _rays(256)
    base = render_surface(model, o, d, cos_anneal=0.5)
    with torch.no_grad():
        base_test = render_surface(model, o, d, test_time=True, cos_anneal=0.5)
    assert calls == [] and "parent" not in base and "rm_samples_coarse" not in base and "parent" not in base_test
    res = render_surface(model, o, d, cos_anneal=0.5, n_importance=16)
    assert calls == [16]
    S, Sc = res["ts"].shape[0], int(res["rm_samples_coarse"])
    par = res["parent"]
    assert int(res["rm_samples"]) == S and Sc < S <= Sc + 16 * 256 and par.shape == (S,) and par.dtype == torch.int32
    assert bool((par[1:] >= par[:-1]).all()) and torch.equal(torch.unique(par).cpu(), torch.arange(Sc, dtype=torch.int32))
    for k in ("rgb", "opacity", "depth", "normal", "ws", "grad_norm"):
        assert bool(torch.isfinite(res[k]).all()), k
    assert res["ws"].shape == (S,) and res["grad_norm"].shape == (S,) and not res["ts"].requires_grad
    ra = res["rays_a"].cpu().numpy()
    t_np = res["ts"].cpu().numpy()
    for _, s0, c in ra[:64]:
        assert np.all(np.diff(t_np[s0:s0 + c]) > 0)
    loss = torch.nn.functional.mse_loss(res["rgb"], torch.rand(256, 3, device=DEV)) + 0.1 * ((res["grad_norm"] - 1) ** 2).mean()
    loss.backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if not k.endswith("bias"):
            assert float(p.grad.abs().sum()) > 0, k
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        out = render_surface(model, o, d, test_time=True, cos_anneal=0.5, chunk=100, n_importance=16, importance_inv_s=64.0)
    assert calls == [16, 16, 16, 16] and out["rgb"].shape == (256, 3) and bool(torch.isfinite(out["rgb"]).all())
    assert int(out["rm_samples_coarse"]) < int(out["rm_samples"]) and all(p.grad is None for p in model.parameters())
