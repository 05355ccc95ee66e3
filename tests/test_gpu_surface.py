"""csrc/surface.hip -- ngp_surface_composite_fwd / _bwd -- element by element against the float64 model of tests/surface_reference.py on
its named sets (ray lengths around multiples of 64, a ray that dies in the last lane of a group or the first of the next, a 1 - a of
exactly zero, rays in front of / inside / facing away from the surface, s in {1, 64, 3000} x r in {0, 0.5, 1}, exp overflow, a NaN ray,
ragged blocks), through a buffer layout in which everything the kernels must not touch holds a sentinel; then the autograd node, the
SDFField model, render_surface and the example at a tiny size.

The yardstick is the module's: |gpu - f64| <= 4 E32 scale, E32 the error of the serial float32 evaluation on the same named set.  Live
counts are exact on decided rays and inside count_bounds otherwise; the float64 model is evaluated at the kernel's count.  Every test
prints the ratios it measured (pytest -s); profiles/PARITY_NOTES.md records them."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import surface_reference as sr
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENT = sr.SENTINEL
THR = sr.THR
SETS = list(sr.case_table())
# (name, cotangent switches, bg): g_ws / g_opacity / g_aux on and off, bg in {0, 0.5}
VARIANTS = [("all_bg", dict(g_aux=True, g_opacity=True, g_ws=True, g_depth=True), 0.5),
            ("rgb_only", dict(g_aux=False, g_opacity=False, g_ws=False, g_depth=False), 0.0),
            ("ws_aux", dict(g_aux=True, g_opacity=False, g_ws=True, g_depth=False), 0.0),
            ("op_bg", dict(g_aux=False, g_opacity=True, g_ws=False, g_depth=True), 0.5)]
ALL_VARIANT_SETS = ("lengths", "a_one", "s64_r0.5")
CASES = [(n, v[0]) for n in SETS for v in VARIANTS if v[0] in ("all_bg", "rgb_only") or n in ALL_VARIANT_SETS]
_cache = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent(shape, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), SENT, device=DEV, dtype=dtype)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


class Dev:
    """A named set (or a prefix of it) with its layout and device copies."""

    def __init__(self, case, seed):
        self.case, self.lay = case, sr.Layout(case.rays, seed)
        lay = self.lay
        assert lay.rays_a.min() >= 0 and lay.rays_a[:, 0].max() < lay.n_out and (lay.rays_a[:, 1] + lay.rays_a[:, 2]).max() <= lay.S - 64
        self.t = {k: dev(getattr(lay, k)) for k in ("sdf", "cosv", "rgbs", "aux", "deltas", "ts", "rays_a")}
        self.inv_s = torch.tensor([case.s], device=DEV, dtype=torch.float32)


def device_case(name):
    if name not in _cache:
        _cache[name] = Dev(sr.case_table()[name], sum(map(ord, name)))
    return _cache[name]


def _p(t):
    from ngp_hip import ops
    return ops._ptr(t)


def launch(d, cot=None, bg=0.0, use_aux=True, n_rays=None, tensors=None):
    """Both launches on sentinel-filled buffers.  -> (raw device buffers, the same in row order as numpy for sr.judge)."""
    from ngp_hip import ops
    L, lay, t = ops._lib(), d.lay, dict(d.t, **(tensors or {}))
    n = lay.n if n_rays is None else n_rays
    aux = t["aux"] if use_aux else None
    o = dict(tot=sent(lay.n_out, torch.int32), op=sent(lay.n_out), dep=sent(lay.n_out), rgb=sent((lay.n_out, 3)), out=sent((lay.n_out, 3)),
             aux_out=sent((lay.n_out, 3)), ws=sent(lay.S), alphas=sent(lay.S))
    rc = L.ngp_surface_composite_fwd(_p(t["sdf"]), _p(t["cosv"]), _p(t["rgbs"]), _p(aux), _p(t["deltas"]), _p(t["ts"]), _p(t["rays_a"]),
                                     _p(d.inv_s), d.case.r, THR, n, bg, _p(o["tot"]), _p(o["op"]), _p(o["dep"]), _p(o["rgb"]), _p(o["out"]),
                                     _p(o["aux_out"] if use_aux else None), _p(o["ws"]), _p(o["alphas"]), ops._stream())
    assert rc == 0
    if cot is not None:
        g = {k: dev(None if v is None else (lay.flat(v) if k == "g_ws" else lay.per_ray(v))) for k, v in cot.items()}
        o.update(d_sdf=sent(lay.S), d_cos=sent(lay.S), d_rgbs=sent((lay.S, 3)), d_aux=sent((lay.S, 3)), d_inv_s=sent(1), work=sent(lay.n + 3))
        rc = L.ngp_surface_composite_bwd(_p(g["g_opacity"]), _p(g["g_depth"]), _p(g["g_rgb"]), _p(g["g_aux"] if use_aux else None), _p(g["g_ws"]),
                                         _p(t["sdf"]), _p(t["cosv"]), _p(t["rgbs"]), _p(aux), _p(t["deltas"]), _p(t["ts"]), _p(t["rays_a"]),
                                         _p(d.inv_s), d.case.r, n, bg, _p(o["tot"]), _p(o["alphas"]), _p(o["d_sdf"]), _p(o["d_cos"]),
                                         _p(o["d_rgbs"]), _p(o["d_aux"] if use_aux else None), _p(o["d_inv_s"]), _p(o["work"]), ops._stream())
        assert rc == 0
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in o.items()}
    idx = lay.ray_idx
    got = dict(M=h["tot"][idx], O=h["op"][idx], D=h["dep"][idx], R=h["rgb"][idx], rgb_out=h["out"][idx], A=h["aux_out"][idx] if use_aux else None,
               w=lay.padded(h["ws"]), alphas=lay.padded(h["alphas"]))
    if cot is not None:
        got.update(d_sdf=lay.padded(h["d_sdf"]), d_cos=lay.padded(h["d_cos"]), d_rgbs=lay.padded(h["d_rgbs"]),
                   d_aux=lay.padded(h["d_aux"]) if use_aux else None, d_inv_s=h["d_inv_s"])
    return o, h, got


def assert_sentinels(lay, h, m=None, use_aux=True):
    """Everything outside the first m rays still holds the sentinel: unused samples, spare rows, output rows of no ray."""
    outside_s, outside_r = ~lay.sample_mask(m), ~lay.ray_mask(m)
    for k in ("ws", "alphas", "d_sdf", "d_cos", "d_rgbs", "d_aux"):
        if k in h:
            keep = outside_s if (use_aux or k != "d_aux") else np.ones(lay.S, bool)
            assert np.all(h[k][keep] == SENT), "%s was written outside the rays" % k
    for k in ("tot", "op", "dep", "rgb", "out", "aux_out"):
        keep = outside_r if (use_aux or k != "aux_out") else np.ones(lay.n_out, bool)
        assert np.all(h[k][keep] == SENT), "%s was written for a ray index of no ray" % k
    if "work" in h:
        assert np.all(h["work"][(lay.n if m is None else m):] == SENT)


@pytest.mark.parametrize("name,variant", CASES)
def test_forward_and_backward_against_float64(hip_lib, name, variant):
    _, switches, bg = next(v for v in VARIANTS if v[0] == variant)
    d = device_case(name)
    cot = sr.cotangents(d.case.rays, **switches)
    e32, _, _ = sr.case_e32(d.case, cot, bg=bg)
    _, h, got = launch(d, cot, bg)
    assert_sentinels(d.lay, h)
    v = sr.judge(d.case, got, e32, cot, bg=bg)
    print("surface %s %s bg=%g: %s" % (name, variant, bg, v))
    assert v.ok(), v.failures[:5]
    nan = d.case.nan_rows
    if nan.any():                                            # the NaN reaches the ray's own outputs and d_inv_s, nothing faults
        assert np.all(np.isnan(got["R"][nan])) and np.isnan(got["d_inv_s"][0])
    else:
        assert np.isfinite(got["d_inv_s"][0])


@pytest.mark.parametrize("m", sr.RAY_COUNTS)
def test_ragged_ray_counts(hip_lib, m):
    """The first m rays of the `counts` set (4 rays per block): judged with the whole set's E32; the other rays' buffers keep the sentinel."""
    full = sr.case_table()["counts"]
    d = device_case("counts")
    cot = sr.cotangents(full.rays)
    e32, _, _ = sr.case_e32(full, cot, bg=0.5)
    _, h, got = launch(d, cot, 0.5, n_rays=m)
    assert_sentinels(d.lay, h, m)
    sub = full.prefix(m)
    got_m = {k: (x if k == "d_inv_s" or x is None else x[:m]) for k, x in got.items()}
    v = sr.judge(sub, got_m, e32, {k: x[:m] for k, x in cot.items()}, bg=0.5)
    print("surface counts n_rays=%d: %s" % (m, v))
    assert v.ok(), v.failures[:5]


def test_two_launches_are_bit_identical_and_d_inv_s_is_the_ordered_sum(hip_lib):
    """1200 rays (the s64_r0.5 set 60 times over: the reduction's strided loop runs twice): every output of two launches has the same
    bits, d_inv_s included; copies of a ray give the same row; d_inv_s is the sum of the per-ray rows to float32 summation accuracy."""
    base = sr.case_table()["s64_r0.5"]
    rows = np.tile(np.arange(base.rays.n), 60)
    d = Dev(sr.Case(base.rays.take(rows), base.s, base.r), 77)
    cot = sr.cotangents(d.case.rays)
    o1, h1, _ = launch(d, cot, 0.5)
    o2, h2, _ = launch(d, cot, 0.5)
    for k in o1:
        assert same_bits(o1[k], o2[k]), k
    work = h1["work"][:d.lay.n].astype(np.float64)
    assert abs(h1["d_inv_s"][0] - work.sum()) <= 16 * 2.0**-24 * np.abs(work).sum()
    d2 = Dev(d.case, 78)                                      # another layout: the rows follow rays_a, bit for bit
    _, h3, _ = launch(d2, cot, 0.5)
    assert np.array_equal(h1["work"][:d.lay.n].view(np.uint32), h3["work"][:d.lay.n].view(np.uint32))
    assert h1["d_inv_s"].view(np.uint32)[0] == h3["d_inv_s"].view(np.uint32)[0]


def test_a_nan_ray_leaves_every_other_ray_unchanged(hip_lib):
    d = device_case("nan")
    lay, nan = d.lay, d.case.nan_rows
    cot = sr.cotangents(d.case.rays)
    _, h_nan, _ = launch(d, cot, 0.5)
    clean = {k: torch.where(torch.isnan(d.t[k]), torch.full_like(d.t[k], 0.3 if k == "sdf" else -0.5), d.t[k]) for k in ("sdf", "cosv")}
    _, h_ok, _ = launch(d, cot, 0.5, tensors=clean)
    others_s = np.zeros(lay.S, bool)
    for r in np.flatnonzero(~nan):
        others_s[lay.start[r]:lay.start[r] + lay.rays.N[r]] = True
    others_r = np.zeros(lay.n_out, bool)
    others_r[lay.ray_idx[~nan]] = True
    for k in ("ws", "alphas", "d_sdf", "d_cos", "d_rgbs", "d_aux"):
        assert np.array_equal(h_nan[k][others_s].view(np.uint32), h_ok[k][others_s].view(np.uint32)), k
    for k in ("tot", "op", "dep", "rgb", "out", "aux_out"):
        assert np.array_equal(h_nan[k][others_r].view(np.uint32), h_ok[k][others_r].view(np.uint32)), k
    assert np.array_equal(h_nan["work"][:lay.n][~nan].view(np.uint32), h_ok["work"][:lay.n][~nan].view(np.uint32))
    assert np.isfinite(h_ok["d_inv_s"][0]) and all(np.isnan(h_nan["rgb"][lay.ray_idx[r]]).all() for r in np.flatnonzero(nan))


def test_no_rays_empty_rays_and_no_aux(hip_lib):
    d = device_case("lengths")
    cot = sr.cotangents(d.case.rays)
    _, h, _ = launch(d, cot, 0.5, n_rays=0)                       # n_rays = 0: status 0, nothing launched, nothing written
    assert all(np.all(x == SENT) for x in h.values())
    _, h, got = launch(d, cot, 0.5)
    empty = d.case.rays.N == 0
    assert empty.sum() == 2
    assert np.all(got["M"][empty] == 0) and np.all(got["O"][empty] == 0) and np.all(got["D"][empty] == 0) and np.all(got["R"][empty] == 0)
    assert np.all(got["rgb_out"][empty] == F(0.5)) and np.all(got["A"][empty] == 0) and np.all(h["work"][:d.lay.n][empty] == 0)
    o_aux, _, _ = launch(d, cot, 0.5)
    cot_no = dict(cot, g_aux=None)
    o_ref, _, _ = launch(d, cot_no, 0.5)                          # aux present, no cotangent for it
    o_no, h_no, _ = launch(d, cot_no, 0.5, use_aux=False)         # aux = NULL: the same numbers, the aux buffers untouched
    assert_sentinels(d.lay, h_no, use_aux=False)
    for k in ("tot", "op", "dep", "rgb", "out", "ws", "alphas", "d_sdf", "d_cos", "d_rgbs", "d_inv_s", "work"):
        assert same_bits(o_ref[k], o_no[k]), k
    for k in ("tot", "op", "dep", "rgb", "out", "ws", "alphas", "d_rgbs"):
        assert same_bits(o_aux[k], o_no[k]), k


def test_ops_refuse_cpu_tensors_and_bad_shapes(hip_lib):
    from ngp_hip import ops
    z = torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.surface_composite_fwd(z, z, torch.zeros(4, 3), z, z, torch.zeros(1, 3, dtype=torch.int32), torch.ones(1))
    g = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    with pytest.raises(ValueError, match="rgbs"):
        ops.surface_composite_fwd(g(4), g(4), g(4, 4), g(4), g(4), g(1, 3, dtype=torch.int32), g(1))
    with pytest.raises(ValueError, match="one float"):
        ops.surface_composite_fwd(g(4), g(4), g(4, 3), g(4), g(4), g(1, 3, dtype=torch.int32), g(2))


def test_autograd_wiring_equals_the_operator(hip_lib):
    from ngp_hip import ops
    from ngp_hip.surface import surface_render_func
    d = device_case("s64_r0.5")
    lay, t = d.lay, d.t
    ra = lay.rays_a.copy()
    ra[:, 0] = np.random.default_rng(9).permutation(lay.n)               # the operator layer sizes the per-ray outputs by the ray count
    ra = dev(ra)
    live = torch.from_numpy(lay.sample_mask()).to(DEV)
    for shape in ((1,), ()):
        leaf = {k: t[k].clone().requires_grad_() for k in ("sdf", "cosv", "rgbs", "aux")}
        inv_s = torch.nn.Parameter(torch.full(shape, d.case.s, device=DEV))
        vr, op, dep, rgb, ws, aux_out = surface_render_func(leaf["sdf"], leaf["cosv"], leaf["rgbs"], t["deltas"], t["ts"], ra, inv_s,
                                                            cos_anneal=d.case.r, T_threshold=THR, aux=leaf["aux"], bg=0.5)
        gen = torch.Generator(DEV).manual_seed(5)
        g = {k: torch.randn(x.shape, device=DEV, generator=gen) for k, x in (("op", op), ("dep", dep), ("rgb", rgb), ("ws", ws), ("aux", aux_out))}
        g["ws"] = torch.where(live, g["ws"], torch.zeros_like(g["ws"]))
        ws_live = torch.where(live, ws, torch.zeros_like(ws))            # (samples of no ray are never written)
        ((op * g["op"]).sum() + (dep * g["dep"]).sum() + (rgb * g["rgb"]).sum() + (aux_out * g["aux"]).sum() + (ws_live * g["ws"]).sum()).backward()
        s1 = inv_s.detach().reshape(1)
        tot, op2, dep2, _rgb2, out2, aux2, ws2, alphas2 = ops.surface_composite_fwd(t["sdf"], t["cosv"], t["rgbs"], t["deltas"], t["ts"], ra, s1,
                                                                                   d.case.r, THR, t["aux"], 0.5)
        assert torch.equal(op, op2) and torch.equal(rgb, out2) and torch.equal(aux_out, aux2) and torch.equal(ws[live], ws2[live])
        assert int(vr) == int(tot.sum()) and not vr.requires_grad
        direct = ops.surface_composite_bwd(g["op"], g["dep"], g["rgb"], g["aux"], g["ws"], t["sdf"], t["cosv"], t["rgbs"], t["deltas"], t["ts"],
                                           ra, s1, tot, alphas2, d.case.r, t["aux"], 0.5)
        for k, ref in zip(("sdf", "cosv", "rgbs", "aux"), direct[:4]):
            assert torch.equal(leaf[k].grad[live], ref[live]), k
        assert inv_s.grad.shape == inv_s.shape and torch.equal(inv_s.grad.reshape(1), direct[4])
    # without aux: five outputs and a None
    out = surface_render_func(t["sdf"], t["cosv"], t["rgbs"], t["deltas"], t["ts"], ra, d.inv_s, cos_anneal=d.case.r)
    assert len(out) == 6 and out[5] is None


def _small_model(seed=0):
    from ngp_hip.surface import SDFField
    torch.manual_seed(seed)
    return SDFField(scale=0.5, levels=8, log2_T=14, max_res=256).to(DEV)


def _rays(n, seed=3):
    from ngp_hip import synthetic
    o, d = synthetic.orbit_camera_rays(4, (32, 32), seed=seed)
    pick = np.random.default_rng(seed).permutation(o.shape[0])[:n]
    return dev(o[pick]), dev(d[pick])


def test_sdf_field_trains_through_render_surface(hip_lib):
    """256 rays, a 2^14-entry table with 8 levels, one occupancy warm-up, one backward of MSE + eikonal: finite, non-zero gradients for the
    hash table (through the encoder's double backward), both MLPs and log_inv_s; then test_time=True under no_grad leaves no .grad."""
    from ngp_hip.mesh import extract_mesh, topology
    from ngp_hip.surface import render_surface
    model = _small_model()
    model.update_density_grid(0.01 * 1024 / 3**0.5, warmup=True)
    occupied = int(torch.count_nonzero(model.density_bitfield))
    assert 0 < occupied < model.density_bitfield.numel()
    o, d = _rays(256)
    res = render_surface(model, o, d, cos_anneal=0.5)
    S = res["ws"].shape[0]
    assert S > 0 and res["rgb"].shape == (256, 3) and res["normal"].shape == (256, 3) and res["grad_norm"].shape == (S,) and res["alphas"].shape == (S,)
    assert int(res["vr_samples"]) > 0 and float(res["opacity"].detach().max()) > 0.5
    hit = res["opacity"] > 0.9
    assert bool(hit.any()) and bool((torch.linalg.norm(res["normal"], dim=1) <= res["opacity"] + 1e-3).all())    # composited unit normals
    loss = torch.nn.functional.mse_loss(res["rgb"], torch.rand(256, 3, device=DEV)) + 0.1 * ((res["grad_norm"] - 1) ** 2).mean()
    loss.backward()
    named = dict(model.named_parameters())
    assert set(k.split(".")[0] for k in named) == {"pos_encoder", "geo_layers", "rgb_net", "log_inv_s"}
    for k, p in named.items():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
        if not k.endswith("bias"):
            assert float(p.grad.abs().sum()) > 0, k
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        out = render_surface(model, o, d, test_time=True, cos_anneal=0.5, chunk=100)                # three chunks
    assert out["rgb"].shape == (256, 3) and out["normal"].shape == (256, 3) and not out["rgb"].requires_grad
    assert all(p.grad is None for p in model.parameters())
    assert bool(torch.isfinite(out["rgb"]).all()) and float((out["opacity"] - res["opacity"].detach()).abs().mean()) < 0.1
    # the fresh field is roughly a sphere: its zero level set is ONE closed surface of genus 0 around the origin, inside the box
    mesh = extract_mesh(model.sdf, 32, 0.0, bounds=([-0.5] * 3, [0.5] * 3), sign=-1, device=DEV)
    topo = topology(mesh)
    assert topo["vertices"] > 100 and topo["euler"] == 2 and topo["boundary_edges"] == 0
    with torch.no_grad():
        assert float(model.sdf(torch.zeros(1, 3, device=DEV))) < 0 and float(mesh.vertices.abs().max()) < 0.5


def test_the_example_at_a_tiny_size(hip_lib):
    spec = importlib.util.spec_from_file_location("train_surface_example", os.path.join(ROOT, "examples", "train_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    info = mod.main(["--steps", "60", "--views", "4", "--test_views", "1", "--wh", "32", "--batch", "1024", "--log2_T", "14", "--levels", "8",
                     "--max_res", "256", "--mesh_res", "32", "--warmup_steps", "32"])
    print(info)
    assert all(np.isfinite(v) for v in info.values() if isinstance(v, float)), info
    assert info["loss_last"] < info["loss_first"]
    assert info["mesh_vertices"] > 0 and info["mesh_faces"] > 0 and info["untrained_mesh_vertices"] > 0
