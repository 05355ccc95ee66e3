"""The compositing kernels of csrc/composite.hip -- composite_fwd_kernel, composite_bwd_kernel, composite_train_fused_kernel<HALF, LIVE>,
composite_test_kernel -- element by element against the float64 model of tests/composite_reference.py, on the edges the kernels are
built around (ray lengths around multiples of 64, a ray that dies in the last lane of a group or the first of the next, a 1 - a of
exactly zero, all-zero density, transmittance hovering at the threshold, ragged 4-ray and 16-ray blocks, a NaN density), through a
buffer layout in which everything the kernels must not touch holds a sentinel.

The yardstick is the module's: |gpu - f64| <= K * E32 * scale, E32 the error of the serial float32 evaluation on the same named set
of rays (tests/test_composite_reference.py shows on the CPU that the bound is meetable by the kernels' summation order and that five
deliberate defects break it).  Live counts are exact on decided rays, between the module's count_bounds on undecided ones, and the
float64 model is then evaluated at the kernel's count, so that no value of any ray goes unchecked.  Every test prints the ratios
it measured (pytest -s); profiles/PARITY_NOTES.md records them."""
import numpy as np
import pytest
import torch

import composite_reference as cr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENT = cr.SENTINEL
SETS = ("lengths", "placed", "a_one", "hovering", "counts")
BWD_VARIANTS = [(gws, gop, bg) for gws in (False, True) for gop in (False, True) for bg in (0.0, 0.5)]
FUSED_VARIANTS = [(bg, ls) for bg in (0.0, 0.5, 1.0) for ls in (1.0, 2.0**14)]
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sent(shape, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), SENT, device=DEV, dtype=dtype)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


class Case:
    """One named set in one rgbs precision: the rays (fp16 colours widened), their layout, the device copies.  Built once."""

    def __init__(self, name, half, rays=None):
        rays = cr.case_table()[name] if rays is None else rays
        self.half = half
        self.rays = rays.with_rgb(rays.rgb.astype(np.float16).astype(F)) if half else rays
        self.lay = cr.Layout(self.rays, sum(map(ord, name)), half)
        lay = self.lay
        self.sig, self.rgbs, self.dl, self.ts, self.ra = dev(lay.sigmas), dev(lay.rgbs), dev(lay.deltas), dev(lay.ts), dev(lay.rays_a)
        # every index in rays_a lies inside its buffer
        assert lay.rays_a[:, 0].max() < lay.n_out and (lay.rays_a[:, 1] + lay.rays_a[:, 2]).max() <= lay.S - 64 and lay.rays_a.min() >= 0
        self._prefix = {}

    def prefix(self, m):
        if m not in self._prefix:
            self._prefix[m] = self.rays.take(np.arange(m))
        return self._prefix[m]


def case(name, half):
    if (name, half) not in _cache:
        _cache[name, half] = Case(name, half)
    return _cache[name, half]


def _ptr(t):
    from ngp_hip import ops
    return ops._ptr(t)


def _stream():
    from ngp_hip import ops
    return ops._stream()


def run_forward(L, c, m, bg=None):
    lay = c.lay
    o = dict(tot=sent(lay.n_out, torch.int32), op=sent(lay.n_out), dep=sent(lay.n_out), rgb=sent((lay.n_out, 3)), ws=sent(lay.S))
    head = (_ptr(c.sig), _ptr(c.rgbs), int(c.half), _ptr(c.dl), _ptr(c.ts), _ptr(c.ra), cr.THR, m, _ptr(o["tot"]), _ptr(o["op"]),
            _ptr(o["dep"]), _ptr(o["rgb"]), _ptr(o["ws"]))
    if bg is None:
        assert L.ngp_composite_train_fwd(*head, _stream()) == 0
    else:
        o["out"] = sent((lay.n_out, 3))
        assert L.ngp_composite_train_fwd_bg(*head, _ptr(o["out"]), bg, _stream()) == 0
    torch.cuda.synchronize()
    return o


def forward_result(c, m, o):
    """Device outputs -> the padded row-order dict the module judges; everything outside the first m rays must hold the sentinel."""
    lay, idx = c.lay, c.lay.ray_idx[:m]
    keep_s, keep_r = ~lay.sample_mask(m), ~lay.ray_mask(m)
    ws = o["ws"].cpu().numpy()
    assert np.all(ws[keep_s] == SENT), "ws written outside the rays"
    got = dict(w=lay.padded(ws, m))
    for k, name in (("tot", "M"), ("op", "O"), ("dep", "D"), ("rgb", "R"), ("out", "rgb_out")):
        if k in o:
            a = o[k].cpu().numpy()
            assert np.all(a[keep_r] == SENT), "%s written for a ray index that is not present" % k
            got[name] = a[idx]
    return got


def run_backward(L, c, m, fwd, g_rgb, g_dep, g_op, g_ws, bg):
    lay = c.lay
    ds, dc = sent(lay.S), sent((lay.S, 3), torch.float16 if c.half else torch.float32)
    t = [None if g is None else dev(lay.per_ray(g)) for g in (g_op, g_dep, g_rgb)] + [None if g_ws is None else dev(lay.flat(g_ws))]
    args = (_ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(t[3]), _ptr(c.sig), _ptr(c.rgbs), int(c.half), _ptr(c.dl), _ptr(c.ts), _ptr(c.ra),
            _ptr(fwd["op"]), _ptr(fwd["dep"]), _ptr(fwd["rgb"]), _ptr(fwd["ws"]), cr.THR, m, _ptr(ds), _ptr(dc))
    if bg == 0.0:
        assert L.ngp_composite_train_bwd(*args, _stream()) == 0
    else:
        assert L.ngp_composite_train_bwd_bg(*args, bg, _stream()) == 0
    torch.cuda.synchronize()
    return ds, dc


def backward_result(c, m, ds, dc):
    lay = c.lay
    keep = ~lay.sample_mask(m)
    ds, dc = ds.cpu().numpy(), dc.float().cpu().numpy()
    assert np.all(ds[keep] == SENT) and np.all(dc[keep] == SENT), "gradients written outside the rays"
    return lay.padded(ds, m), lay.padded(dc, m)


def run_fused(L, c, m, target, bg, loss_scale, live, live_total0=0):
    lay = c.lay
    o = dict(tot=sent(lay.n_out, torch.int32), op=sent(lay.n_out), dep=sent(lay.n_out), rgb=sent((lay.n_out, 3)), ws=sent(lay.S),
             ds=sent(lay.S), dc=sent((lay.S, 3), torch.float16 if c.half else torch.float32), sq=sent(lay.n_out))
    tgt, ls = dev(lay.per_ray(target)), torch.tensor([loss_scale], device=DEV, dtype=torch.float32)
    if live:
        o["list"] = sent(lay.S + 64, torch.int32)
        o["total"] = torch.tensor([live_total0], device=DEV, dtype=torch.int32)
        o["zero"] = torch.tensor([123], device=DEV, dtype=torch.int32)
    assert L.ngp_composite_train_fused_live(_ptr(c.sig), _ptr(c.rgbs), int(c.half), _ptr(c.dl), _ptr(c.ts), _ptr(c.ra), _ptr(tgt), bg, _ptr(ls),
                                            cr.THR, m, _ptr(o["tot"]), _ptr(o["op"]), _ptr(o["dep"]), _ptr(o["rgb"]), _ptr(o["ws"]),
                                            _ptr(o["ds"]), _ptr(o["dc"]), _ptr(o["sq"]), _ptr(o.get("list")), _ptr(o.get("total")),
                                            _ptr(o.get("zero")), _stream()) == 0
    torch.cuda.synchronize()
    return o


def check_live_list(c, m, o):
    """live_total == sum vr; the list holds exactly start_r .. start_r + vr_r - 1 of every ray, each ray contiguous and ascending; the
    tail keeps its sentinel; live_zero is cleared."""
    lay = c.lay
    vr = o["tot"].cpu().numpy()[lay.ray_idx[:m]]
    total, lst = int(o["total"][0]), o["list"].cpu().numpy()
    assert total == int(vr.sum()) and int(o["zero"][0]) == 0
    assert np.all(lst[total:] == int(SENT))
    want = np.concatenate([np.arange(lay.start[r], lay.start[r] + vr[r]) for r in range(m)] + [np.zeros(0, np.int64)])
    assert np.array_equal(np.sort(lst[:total]), np.sort(want))
    pos = {int(s): p for p, s in enumerate(lst[:total])}
    for r in range(m):
        if vr[r]:
            p = pos[int(lay.start[r])]
            assert np.array_equal(lst[p:p + vr[r]], lay.start[r] + np.arange(vr[r])), "ray %s is not contiguous in the list" % c.rays.names[r]


def _note(worst, v):
    for q, r in v.ratios.items():
        worst[q] = max(worst.get(q, 0.0), r)


def _fmt(worst):
    return ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))


def _e32(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _counts_of(name, c):
    return cr.RAY_COUNTS if name == "counts" else (c.rays.n,)


# ------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", SETS)
def test_forward(hip_lib, name, half):
    c = case(name, half)
    worst = {}
    for bg in (None, 0.5, 1.0):
        e32, _ = _e32(("fwd", name, half, bg), lambda: cr.forward_e32(c.rays, bg))
        for m in _counts_of(name, c):
            o = run_forward(hip_lib, c, m, bg)
            v, _ = cr.judge_forward(c.prefix(m), forward_result(c, m, o), e32, bg=bg)
            assert v.ok(), (name, bg, m, v.failures[:5])
            _note(worst, v)
            if bg is not None:                              # the unblended outputs are the plain entry's, bit for bit
                p = run_forward(hip_lib, c, m, None)
                assert all(same_bits(o[k], p[k]) for k in ("tot", "op", "dep", "rgb", "ws"))
    print("composite fwd %s/%s: |gpu - f64| / (E32 scale): %s (bound %d)" % (name, "f16" if half else "f32", _fmt(worst), cr.K))


# ------------------------------------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", SETS)
def test_backward(hip_lib, name, half):
    c = case(name, half)
    g_rgb, g_dep, g_op, g_ws = cr.gradients(c.rays, 21)
    worst = {}
    for m in _counts_of(name, c):
        fwd = run_forward(hip_lib, c, m)
        M = forward_result(c, m, fwd)["M"]
        for gws, gop, bg in (BWD_VARIANTS if m == c.rays.n else [(True, True, 0.5)]):
            a = (g_rgb, g_dep if gop else None, g_op if gop else None, g_ws if gws else None)
            e32 = _e32(("bwd", name, half, gws, gop, bg), lambda: cr.backward_e32(c.rays, *a, bg=bg))
            ds, dc = backward_result(c, m, *run_backward(hip_lib, c, m, fwd, *a, bg))
            v = cr.judge_backward(c.prefix(m), ds, dc, M, e32, *[None if x is None else x[:m] for x in a], bg=bg, dc_half=half)
            assert v.ok(), (name, (gws, gop, bg), m, v.failures[:5])
            _note(worst, v)
    print("composite bwd %s/%s: |gpu - f64| / (E32 scale): %s (bound %d)" % (name, "f16" if half else "f32", _fmt(worst), cr.K))


# ------------------------------------------------------------------------------------------------ 3. fused
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", SETS)
def test_fused(hip_lib, name, half):
    c = case(name, half)
    worst = {}
    for m in _counts_of(name, c):
        fwd = run_forward(hip_lib, c, m)
        for bg, ls in (FUSED_VARIANTS if m == c.rays.n else [(0.5, 1.0)]):
            tgt = _e32(("tgt", name, half, bg), lambda: cr.targets(c.rays, bg, 31))
            e32 = _e32(("fused", name, half, bg, ls, m), lambda: cr.fused_e32(c.rays, tgt, bg, ls, m))
            plain, live = run_fused(hip_lib, c, m, tgt, bg, ls, False), run_fused(hip_lib, c, m, tgt, bg, ls, True)
            for k in ("tot", "op", "dep", "rgb", "ws"):      # "same arithmetic as composite_fwd_kernel"
                assert same_bits(plain[k], fwd[k]), (name, bg, ls, m, k)
            for k in ("tot", "op", "dep", "rgb", "ws", "ds", "dc", "sq"):
                assert same_bits(plain[k], live[k]), (name, bg, ls, m, k)
            check_live_list(c, m, live)
            got = forward_result(c, m, plain)
            got["d_sigma"], got["d_rgbs"] = backward_result(c, m, plain["ds"], plain["dc"])
            sq = plain["sq"].cpu().numpy()
            assert np.all(sq[~c.lay.ray_mask(m)] == SENT)
            got["sq_err"] = sq[c.lay.ray_idx[:m]]
            v = cr.judge_fused(c.prefix(m), got, tgt[:m], bg, ls, m, e32, dc_half=half)
            assert v.ok(), (name, bg, ls, m, v.failures[:5])
            _note(worst, v)
    print("composite fused %s/%s: |gpu - f64| / (E32 scale): %s (bound %d)" % (name, "f16" if half else "f32", _fmt(worst), cr.K))


def test_fused_live_total_untouched_when_every_ray_is_empty(hip_lib):
    rng = np.random.default_rng(1)
    rays = cr.make_rays([cr._ray(rng, "empty%d" % i, 0, np.zeros(0)) for i in range(5)])
    c = Case("empty", True, rays)
    o = run_fused(hip_lib, c, 5, np.zeros((5, 3), F), 1.0, 1.0, True, live_total0=77)
    assert int(o["total"][0]) == 77 and int(o["zero"][0]) == 0
    assert np.all(o["list"].cpu().numpy() == int(SENT)) and np.all(o["ws"].cpu().numpy() == SENT)
    assert np.array_equal(o["tot"].cpu().numpy()[c.lay.ray_idx], np.zeros(5, np.int32))
    # an empty ray composites to nothing: the loss sees the background
    assert np.array_equal(o["sq"].cpu().numpy()[c.lay.ray_idx], np.full(5, 3.0, F))


# ------------------------------------------------------------------------------------------------ 4. poisoned ray
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_poisoned_ray(hip_lib, half):
    """A NaN density at sample 10 of one ray among 16 healthy ones: its own outputs are NaN, its count is 11 (every kernel stops at
    the NaN), and every other ray has the bits it has without it."""
    t = cr.case_table()["counts"]
    rows = list(range(16))
    victim = next(i for i in range(16, t.n) if t.N[i] >= 65)
    rows.insert(5, victim)                                  # row 5: inside the first 16-ray block, among healthy rays
    healthy = t.take(rows)
    sig = healthy.sigma.copy()
    sig[5, 10] = np.nan
    poisoned = cr.Rays(sig, healthy.delta, healthy.t, healthy.rgb, healthy.N, healthy.names[:5] + ["poisoned"] + healthy.names[6:])
    a, b = Case("poison", half, poisoned), Case("poison", half, healthy)
    assert np.array_equal(a.lay.rays_a, b.lay.rays_a)
    lay, n = a.lay, 17
    others_r = np.delete(lay.ray_idx, 5)
    others_s = lay.sample_mask() & ~np.isin(np.arange(lay.S), np.arange(lay.start[5], lay.start[5] + lay.rays.N[5]))
    own = slice(lay.start[5], lay.start[5] + lay.rays.N[5])
    g_rgb, g_dep, g_op, g_ws = cr.gradients(poisoned, 5)
    tgt = cr.targets(healthy, 0.5, 6)
    outs = []
    for c in (a, b):
        fwd = run_forward(hip_lib, c, n)
        ds, dc = run_backward(hip_lib, c, n, fwd, g_rgb, g_dep, g_op, g_ws, 0.5)
        fused = [run_fused(hip_lib, c, n, tgt, 0.5, 1.0, live) for live in (False, True)]
        outs.append((fwd, ds, dc, fused))
    (fa, dsa, dca, fua), (fb, dsb, dcb, fub) = outs
    ridx = int(lay.ray_idx[5])
    for o in [fa] + fua:
        assert int(o["tot"][ridx]) == 11
        assert bool(torch.isnan(o["op"][ridx])) and bool(torch.isnan(o["dep"][ridx])) and bool(torch.isnan(o["rgb"][ridx]).all())
        w = o["ws"][own].cpu().numpy()
        assert np.isnan(w[10]) and np.all(np.isfinite(w[:10])) and np.all(w[11:] == 0)
    for o in fua:
        assert bool(torch.isnan(o["sq"][ridx])) and bool(torch.isnan(o["ds"][own][:11]).all()) and bool((o["ds"][own][11:] == 0).all())
    check_live_list(a, n, fua[1])
    assert bool(torch.isnan(dsa[own][:11]).all()) and bool((dsa[own][11:] == 0).all()) and bool((dca[own][11:] == 0).all())
    ro, so = torch.from_numpy(others_r.astype(np.int64)).to(DEV), torch.from_numpy(np.flatnonzero(others_s)).to(DEV)
    for x, y in [(fa, fb), (fua[0], fub[0]), (fua[1], fub[1])]:
        for k in ("tot", "op", "dep", "rgb") + (("sq",) if "sq" in x else ()):
            assert same_bits(x[k][ro], y[k][ro]), k
        for k in ("ws",) + (("ds", "dc") if "ds" in x else ()):
            assert same_bits(x[k][so], y[k][so]), k
    assert same_bits(dsa[so], dsb[so]) and same_bits(dca[so], dcb[so])


# ------------------------------------------------------------------------------------------------ 5. test-time composite
def _test_time_rays():
    """steps in {0, 1, 8, 70}: thin rays (stay alive), medium rays, a placed opaque sample (sigma delta = 12: the ray dies AT that
    sample and includes it), and starting opacities that put T = 1 - opacity_in one float32 step above / below thr in front of a
    zero-density sample (T is unchanged by it: alive / dead exactly)."""
    rng = np.random.default_rng(41)
    lst, op_in = [], []
    for steps in (0, 1, 8, 70):
        for rep in range(3):
            lst.append(cr._ray(rng, "thin_steps%d_%d" % (steps, rep), steps, cr._thin(rng, steps))); op_in.append(0.5 * rng.random())
            lst.append(cr._ray(rng, "medium_steps%d_%d" % (steps, rep), steps, 9.21 / max(steps, 1) * 3 * rng.random(steps))); op_in.append(0.5 * rng.random())
        for k in sorted({1, max(1, steps // 2), steps} - {0}) if steps else ():
            sd = cr._thin(rng, steps)
            sd[k - 1] = 12.0
            lst.append(cr._ray(rng, "placed_k%d_steps%d" % (k, steps), steps, sd)); op_in.append(0.5 * rng.random())
        if steps:
            for tag, ticks in (("above", 1678), ("below", 1677)):            # thr = 1677.7 * 2^-24
                sd = cr._thin(rng, steps)
                sd[0] = 0.0
                lst.append(cr._ray(rng, "start_%s_steps%d" % (tag, steps), steps, sd)); op_in.append(1.0 - ticks * 2.0**-24)
    return cr.make_rays(lst), np.asarray(op_in, F)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_composite_test_kernel(hip_lib, half):
    rays, op_in = _test_time_rays()
    if half:
        rays = rays.with_rgb(rays.rgb.astype(np.float16).astype(F))
    n = rays.n
    T0 = 1.0 - op_in.astype(np.float64)
    assert not cr.undecided(rays, T0=T0, extra_rel=2.0**-24).any()          # every ray of this table is decided
    lay = cr.Layout(rays, 77, half)
    rng = np.random.default_rng(43)
    n_total = n + 9                                                       # nine rays that are not in `alive`
    slot = rng.permutation(n_total)[:n].astype(np.int64)                  # alive[i]: the ray of pack_info row i
    op0, dep0, rgb0 = np.full(n_total, 0.25, F), rng.random(n_total).astype(F), rng.random((n_total, 3)).astype(F)
    op0[slot] = op_in
    pack = np.stack([lay.start.astype(np.int64), rays.N], 1)
    alive, op, dep, rgb = dev(slot.copy()), dev(op0), dev(dep0), dev(rgb0)
    assert hip_lib.ngp_composite_test(_ptr(dev(lay.sigmas)), _ptr(dev(lay.rgbs)), int(half), _ptr(dev(lay.deltas)), _ptr(dev(lay.ts)),
                                      _ptr(dev(pack)), _ptr(alive), cr.THR, n, _ptr(op), _ptr(dep), _ptr(rgb), _stream()) == 0
    torch.cuda.synchronize()
    alive, op, dep, rgb = alive.cpu().numpy(), op.cpu().numpy(), dep.cpu().numpy(), rgb.cpu().numpy()
    ref, s32 = cr.test64(rays, op_in), cr.serial32_test(rays, op_in)
    assert np.array_equal(s32["dead"], ref["dead"]) and np.array_equal(s32["steps"], ref["steps"])
    assert np.array_equal(alive, np.where(ref["dead"], -1, slot))
    for i, nm in enumerate(rays.names):                    # above: the zero-density sample leaves the ray alive, the next one ends it
        if nm.startswith("start_"):
            above = nm.startswith("start_above")
            assert ref["steps"][i] == (min(2, rays.N[i]) if above else 1) and ref["dead"][i] == (not above or rays.N[i] > 1)
    rest = np.setdiff1d(np.arange(n_total), slot)
    assert np.array_equal(op[rest], op0[rest]) and np.array_equal(dep[rest], dep0[rest]) and np.array_equal(rgb[rest], rgb0[rest])
    empty = slot[rays.N == 0]
    assert np.array_equal(op[empty], op0[empty]) and np.array_equal(rgb[empty], rgb0[empty])
    v = cr.Verdict()
    wt = np.sum(ref["w"] * rays.t, 1)
    quantities = {"O": (op[slot], op0[slot], s32["O"], ref["O"], ref["O"]), "D": (dep[slot], dep0[slot], s32["D"], ref["D"], wt),
                  "R": (rgb[slot], rgb0[slot], s32["R"], ref["R"], np.broadcast_to(ref["O"][:, None], (n, 3)))}
    for q, (got, init, inc32, inc64, mag) in quantities.items():
        init64 = init.astype(np.float64)
        want, scale = init64 + inc64, np.abs(init64) + mag                # final accumulator = initial + increment, one float32 add
        e32 = cr._e32(np.abs((init + inc32).astype(np.float64) - want), scale)
        assert e32 > 0
        cr._judge(v, rays, q, got, want, scale, e32, cr.K)
    assert v.ok(), v.failures[:5]
    print("composite test-time %s: |gpu - f64| / (E32 scale): %s (bound %d)" % ("f16" if half else "f32", v, cr.K))


# ------------------------------------------------------------------------------------------------ 6. distortion on the same layout
@pytest.mark.parametrize("name", ["lengths", "placed"])
def test_distortion_on_composited_weights(hip_lib, oracle, name):
    """ngp_distortion_fwd / _bwd on the ws the forward kernel produced, judged as test_distortion_golden_and_oracle judges them: both
    float32 evaluations against the float64 restatement, the kernel's error at most 3x the oracle's + 1e-6."""
    c = case(name, False)
    lay, n = c.lay, c.rays.n
    fwd = run_forward(hip_lib, c, n)
    ws = fwd["ws"].clone()
    loss, wi, wti = sent(lay.n_out), sent(lay.S), sent(lay.S)
    assert hip_lib.ngp_distortion_fwd(_ptr(ws), _ptr(c.dl), _ptr(c.ts), _ptr(c.ra), n, _ptr(loss), _ptr(wi), _ptr(wti), _stream()) == 0
    gl = np.random.default_rng(9).standard_normal(n).astype(F)
    dws = sent(lay.S)
    assert hip_lib.ngp_distortion_bwd(_ptr(dev(lay.per_ray(gl))), _ptr(ws), _ptr(c.dl), _ptr(c.ts), _ptr(wi), _ptr(wti), _ptr(c.ra), n,
                                      _ptr(dws), _stream()) == 0
    torch.cuda.synchronize()
    ws_h, loss, dws = ws.cpu().numpy(), loss.cpu().numpy(), dws.cpu().numpy()
    keep = ~lay.sample_mask()
    assert np.all(dws[keep] == SENT) and np.all(wi.cpu().numpy()[keep] == SENT) and np.all(loss[~lay.ray_mask()] == SENT)
    rays_a = lay.rays_a.copy()
    rays_a[:, 0] = np.arange(n)                             # (the oracle sizes its per-ray outputs by the row count)
    ref_loss, ref_wi, ref_wti = oracle.distortion_fwd(ws_h, lay.deltas, lay.ts, rays_a)
    ref_dws = oracle.distortion_bwd(gl, lay.deltas, ws_h, lay.ts, ref_wi, ref_wti, rays_a)
    f64, d64 = np.zeros(n), np.zeros(lay.S)
    used = np.zeros(lay.S, bool)
    for r, (_, s0, cnt) in enumerate(rays_a):
        sl = slice(s0, s0 + cnt)
        f64[r] = cr.distortion_loss64(ws_h[sl], lay.ts[sl], lay.deltas[sl])
        if cnt:
            d64[sl] = cr.distortion_grad64(gl[r], ws_h[sl], lay.ts[sl], lay.deltas[sl])
            used[sl] = True
    err_hip, err_ora = np.abs(loss[lay.ray_idx] - f64).max(), np.abs(ref_loss - f64).max()
    assert err_hip <= 3 * err_ora + 1e-6, (err_hip, err_ora)
    g_hip, g_ora = np.abs(dws[used] - d64[used]).max(), np.abs(ref_dws[used] - d64[used]).max()
    assert g_hip <= 3 * g_ora + 1e-6 * np.abs(d64).max(), (g_hip, g_ora)
    print("distortion on %s: loss error %.3g (oracle %.3g), gradient error %.3g (oracle %.3g)" % (name, err_hip, err_ora, g_hip, g_ora))
