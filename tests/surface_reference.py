"""Float64 model of the SDF surface compositor (NeuS opacity), its serial float32 evaluation, and the yardstick the kernels of
csrc/surface.hip are held to (tests/test_surface_reference.py on the CPU, tests/test_gpu_surface.py on the GPU).  numpy only.

The contract, per ray (include/ngp_hip.h, "surface rendering"):

    ic = -( relu(-c/2 + 1/2) (1 - r) + relu(-c) r );  h = ic delta / 2
    p  = sigmoid((f - h) s),  n = sigmoid((f + h) s);  a = clip( (p - n + 1e-5) / (p + 1e-5), 0, 1 )
    T = 1;  for j < N:  stop at the first !(T > thr);  w_j = a T;  R += w rgb;  A += w aux;  D += w t;  O += w;  T <- T (1 - a);  M += 1

  forward64 / backward64       the contract in float64.  backward64 is a REVERSE SWEEP of the loop (the adjoint X of the transmittance
                               behind a sample: X_{j-1} = G_j a_j + (1 - a_j) X_j, dL/da_j = T_j (G_j - X_j)); it also returns the
                               magnitude sums S: the same sweep with every term's absolute value.
  serial32_forward / _backward the same serial loops with every rounding a separate numpy float32 operation (no contraction: the
                               library is built with -ffp-contract=off); expf is numpy's float32 exp.  `alter` switches on one of three
                               deliberate defects (ALTERATIONS); tests/test_surface_reference.py shows the yardstick catches each.

The two share their loop bodies (one function, parametrised by the number format): what separates them is the arithmetic alone.  The
float64 backward is checked against central differences of the float64 forward.

The yardstick is composite_reference's.  For a named set, E32 = max |serial32 - f64| / scale and a result passes when
|got - f64| <= K E32 scale + TINY (K = 4), with the scales
    ws: T_j     alphas: 1 on the live samples (= T_j for alphas T_j)     R, aux_out: O     rgb_out: O + |bg| (1 + O)     D: sum w |t|
    d_sdf, d_cos, d_inv_s: the magnitude sums S     d_rgbs: |g_rgb| T_j     d_aux: |g_aux| T_j
serial32 runs at the float64 model's live counts.  d_inv_s is one number per launch: its E32 is taken over the per-ray sums of the set
as well as their total, so that it does not hang on the luck of one rounding.

Decidability of the live count: composite_reference.count_bounds' rule, U_j = W sum_{i<j} T_j / (1 - a_i), with the absolute error W
of a float32 `1 - a_i` widened from 2^-22 to 2^-22 + alpha_width(): the largest |a32 - a64| serial32 makes on the named sets, rounded
up to a power of two (the NeuS opacity is a quotient of differences of sigmoids, not one expf)."""
import numpy as np

from composite_reference import F, K, SENTINEL, THR, THR32, TINY, WAVE, Verdict, _e32, _judge, _judge_zeros  # noqa: F401

EPS = 1e-5
ALTERATIONS = {
    "eps": "the 1e-5 terms of the opacity are dropped",
    "one_minus_a": "da/df omits the (1 - a) factor on p'",
    "anneal": "da/dc ignores the anneal branch (uses [-c > 0] alone, as if r = 1)",
}


class SRays:
    """A padded batch: f, c, delta, t [n, L], rgb, aux [n, L, 3] (float32 unless dtype is given), N [n], names [n]."""

    def __init__(self, f, c, delta, t, rgb, aux, N, names, dtype=F):
        self.f, self.c, self.delta, self.t, self.rgb, self.aux = (np.ascontiguousarray(x, dtype) for x in (f, c, delta, t, rgb, aux))
        self.N, self.names = np.asarray(N, np.int64), list(names)
        self.n, self.L = self.f.shape
        assert self.L % WAVE == 0 and self.N.max(initial=0) <= self.L and len(self.names) == self.n
        self.valid = np.arange(self.L)[None, :] < self.N[:, None]

    def take(self, rows):
        rows = np.asarray(rows)
        return SRays(self.f[rows], self.c[rows], self.delta[rows], self.t[rows], self.rgb[rows], self.aux[rows], self.N[rows],
                     [self.names[i] for i in rows], self.f.dtype)

    def replace(self, dtype=None, **kw):
        d = dict(f=self.f, c=self.c, delta=self.delta, t=self.t, rgb=self.rgb, aux=self.aux)
        d.update(kw)
        return SRays(d["f"], d["c"], d["delta"], d["t"], d["rgb"], d["aux"], self.N, self.names, dtype or self.f.dtype)


def make_rays(ray_list):
    """ray_list: [(name, f [N], c [N], delta [N], t [N], rgb [N,3], aux [N,3])] -> SRays."""
    n = len(ray_list)
    L = max(WAVE, -(-max(len(r[1]) for r in ray_list) // WAVE) * WAVE)
    f, c, dl, t = np.ones((n, L), F), np.zeros((n, L), F), np.ones((n, L), F), np.ones((n, L), F)
    rgb, aux = np.zeros((n, L, 3), F), np.zeros((n, L, 3), F)
    for i, (_, ff, cc, dd, tt, col, ax) in enumerate(ray_list):
        m = len(ff)
        f[i, :m], c[i, :m], dl[i, :m], t[i, :m], rgb[i, :m], aux[i, :m] = ff, cc, dd, tt, col, ax
    return SRays(f, c, dl, t, rgb, aux, [len(r[1]) for r in ray_list], [r[0] for r in ray_list])


# ------------------------------------------------------------------------------------------------------------------ the loops
def _relu(x):
    return np.where(x < 0, x.dtype.type(0), x)              # (lets a NaN through, like the kernel's)


def _sigmoid(x):
    one = x.dtype.type(1)
    return one / (one + np.exp(-x))


def opacity(rays, s, r, dt, alter=""):
    """Every per-sample quantity of the opacity and of its derivatives, in the number format dt, one numpy operation per rounding.
    -> dict a, q = 1 - a, p, n, h, v (before the clip), dadf, dadc, dads and their magnitude sums mf, mc, ms."""
    f, c, dl = rays.f.astype(dt), rays.c.astype(dt), rays.delta.astype(dt)
    s, r, one, half, zero = dt(s), dt(r), dt(1), dt(0.5), dt(0)
    eps = dt(0.0 if "eps" in alter else EPS)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        u1, u2 = -c * half + half, -c
        ic = -(_relu(u1) * (one - r) + _relu(u2) * r)
        h = ic * dl * half
        p, n = _sigmoid((f - h) * s), _sigmoid((f + h) * s)
        den = p + eps
        v = (p - n + eps) / den
        a = np.where(v < 0, zero, np.where(v > 1, one, v))
        free = ~(v < 0) & ~(v > 1)
        pp, nn = p * (one - p), n * (one - n)
        ppa = pp if "one_minus_a" in alter else pp * (one - a)
        dadf = np.where(free, s * (ppa - nn) / den, zero)
        dadh = np.where(free, -s * (pp * (one - a) + nn) / den, zero)
        ind = (u2 > 0).astype(dt) if "anneal" in alter else (one - r) * half * (u1 > 0).astype(dt) + r * (u2 > 0).astype(dt)
        dadc = dadh * (dl * half) * ind
        dads = np.where(free, ((f - h) * (pp * (one - a)) - (f + h) * nn) / den, zero)
        mh = np.where(free, s * (pp * (one - a) + nn) / den, zero)
        ms = np.where(free, (np.abs(f - h) * (pp * (one - a)) + np.abs(f + h) * nn) / den, zero)
    return dict(a=a, q=one - a, p=p, n=n, h=h, v=v, dadf=dadf, dadc=dadc, dads=dads, mf=mh, mc=mh * (dl * half) * ind, ms=ms)


def _forward(rays, s, r, dt, thr, force_M, alter=""):
    n, L = rays.n, rays.L
    op = opacity(rays, s, r, dt, alter)
    a, q = op["a"], op["q"]
    t, rgb, aux = rays.t.astype(dt), rays.rgb.astype(dt), rays.aux.astype(dt)
    thr, zero = dt(thr), dt(0)
    T, alive = np.ones(n, dt), np.ones(n, bool)
    R, A, D, O, M = np.zeros((n, 3), dt), np.zeros((n, 3), dt), np.zeros(n, dt), np.zeros(n, dt), np.zeros(n, np.int64)
    w, Ts = np.zeros((n, L), dt), np.zeros((n, L), dt)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(int(rays.N.max(initial=0))):
            live = (alive & (j < rays.N) & (T > thr)) if force_M is None else (j < np.asarray(force_M))
            alive = live
            wj = np.where(live, a[:, j] * T, zero)
            w[:, j], Ts[:, j] = wj, np.where(live, T, zero)
            for k in range(3):
                R[:, k] = np.where(live, R[:, k] + wj * rgb[:, j, k], R[:, k])
                A[:, k] = np.where(live, A[:, k] + wj * aux[:, j, k], A[:, k])
            D = np.where(live, D + wj * t[:, j], D)
            O = np.where(live, O + wj, O)
            T = np.where(live, T * q[:, j], T)
            M += live
    live = np.arange(L)[None, :] < M[:, None]
    return dict(op, M=M, T=Ts, w=w, alphas=np.where(live, a, zero), R=R, A=A, D=D, O=O)


def _cotangents(n, L, dt, g_rgb, g_aux, g_depth, g_opacity, g_ws, bg):
    z = lambda x, shape: np.zeros(shape, dt) if x is None else np.asarray(x, dt)
    g_rgb, g_aux, gd, go, gw = z(g_rgb, (n, 3)), z(g_aux, (n, 3)), z(g_depth, n), z(g_opacity, n), z(g_ws, (n, L))
    go_mag = np.abs(go)
    if bg != 0.0:                        # g_rgb is the gradient of the blended colour: the blend's share of d opacity
        go = go + -dt(bg) * ((g_rgb[:, 0] + g_rgb[:, 1]) + g_rgb[:, 2])
        go_mag = go_mag + abs(dt(bg)) * ((np.abs(g_rgb[:, 0]) + np.abs(g_rgb[:, 1])) + np.abs(g_rgb[:, 2]))
    return g_rgb, g_aux, gd, go, go_mag, gw


def _backward(rays, fwd, dt, g_rgb, g_aux, g_depth, g_opacity, g_ws, bg):
    """Reverse sweep on the live samples of `fwd` (its T, a, q, M and the opacity derivatives).  -> dict d_sdf, d_cos [n, L], d_rgbs,
    d_aux [n, L, 3], ds_ray [n], d_inv_s (their sum in row order) and the magnitude sums S_sdf, S_cos [n, L], S_ray [n], S_inv_s."""
    n, L = rays.n, rays.L
    g_rgb, g_aux, gd, go, go_mag, gw = _cotangents(n, L, dt, g_rgb, g_aux, g_depth, g_opacity, g_ws, bg)
    t, rgb, aux = rays.t.astype(dt), rays.rgb.astype(dt), rays.aux.astype(dt)
    T, a, q, M = fwd["T"], fwd["a"], fwd["q"], fwd["M"]
    zero = dt(0)
    X, Xabs = np.zeros(n, dt), np.zeros(n, dt)
    out = {k: np.zeros((n, L), dt) for k in ("d_sdf", "d_cos", "S_sdf", "S_cos")}
    ds, ds_abs = np.zeros(n, dt), np.zeros(n, dt)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(int(M.max(initial=0)) - 1, -1, -1):
            live = j < M
            G = (g_rgb[:, 0] * rgb[:, j, 0] + g_rgb[:, 1] * rgb[:, j, 1]) + g_rgb[:, 2] * rgb[:, j, 2]
            G = G + ((g_aux[:, 0] * aux[:, j, 0] + g_aux[:, 1] * aux[:, j, 1]) + g_aux[:, 2] * aux[:, j, 2])
            G = ((G + gd * t[:, j]) + go) + gw[:, j]
            Gabs = np.abs(g_rgb * rgb[:, j]).sum(1) + np.abs(g_aux * aux[:, j]).sum(1) + np.abs(gd * t[:, j]) + go_mag + np.abs(gw[:, j])
            da, da_abs = T[:, j] * (G - X), T[:, j] * (Gabs + Xabs)
            out["d_sdf"][:, j] = np.where(live, da * fwd["dadf"][:, j], zero)
            out["d_cos"][:, j] = np.where(live, da * fwd["dadc"][:, j], zero)
            out["S_sdf"][:, j] = np.where(live, da_abs * fwd["mf"][:, j], zero)
            out["S_cos"][:, j] = np.where(live, da_abs * fwd["mc"][:, j], zero)
            ds = np.where(live, ds + da * fwd["dads"][:, j], ds)
            ds_abs = np.where(live, ds_abs + da_abs * fwd["ms"][:, j], ds_abs)
            X = np.where(live, G * a[:, j] + q[:, j] * X, X)
            Xabs = np.where(live, Gabs * a[:, j] + q[:, j] * Xabs, Xabs)
        total, total_abs = zero, zero
        for i in range(n):
            total, total_abs = total + ds[i], total_abs + ds_abs[i]
    live = (np.arange(L)[None, :] < M[:, None])[:, :, None]                              # (exact +0, not g * 0 = -0, behind the live count)
    out.update(d_rgbs=np.where(live, g_rgb[:, None, :] * fwd["w"][:, :, None], zero),
               d_aux=np.where(live, g_aux[:, None, :] * fwd["w"][:, :, None], zero), ds_ray=ds, S_ray=ds_abs, d_inv_s=total, S_inv_s=total_abs)
    return out


def forward64(rays, s, r, thr=THR, force_M=None):
    return _forward(rays, s, r, np.float64, thr, force_M)


def backward64(rays, fwd, g_rgb, g_aux=None, g_depth=None, g_opacity=None, g_ws=None, bg=0.0):
    return _backward(rays, fwd, np.float64, g_rgb, g_aux, g_depth, g_opacity, g_ws, bg)


def serial32_forward(rays, s, r, thr=THR32, force_M=None, alter=""):
    return _forward(rays, s, r, F, thr, force_M, alter)


def serial32_backward(rays, fwd, g_rgb, g_aux=None, g_depth=None, g_opacity=None, g_ws=None, bg=0.0):
    return _backward(rays, fwd, F, g_rgb, g_aux, g_depth, g_opacity, g_ws, bg)


# ------------------------------------------------------------------------------------------------------------------ decidability
def alpha_width():
    """The largest |a32 - a64| of serial32 over the named sets (NaN rays apart), rounded up to a power of two."""
    if "w" not in _WIDTH:
        worst = 0.0
        for case in case_table().values():
            rows = [i for i, nm in enumerate(case.rays.names) if not nm.startswith("nan")]
            rays = case.rays.take(rows)
            a64, a32 = opacity(rays, case.s, case.r, np.float64)["a"], opacity(rays, case.s, case.r, F)["a"]
            worst = max(worst, float(np.max(np.abs(a32.astype(np.float64) - a64)[rays.valid], initial=0.0)))
        _WIDTH["raw"] = worst
        _WIDTH["w"] = 2.0 ** int(np.ceil(np.log2(worst)))
    return _WIDTH["w"]


_WIDTH = {}


def transmittance64(case):
    """T_j after j samples, j = 0 .. L, never stopped: [n, L + 1], and U_j of the decidability rule."""
    rays = case.rays
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.where(rays.valid, opacity(rays, case.s, case.r, np.float64)["q"], 1.0)
        P = np.concatenate([np.ones((rays.n, 1)), np.cumprod(q, 1)], 1)
        E = np.zeros_like(P)                                 # E_j = sum_{i<j} prod_{l<j, l != i} q_l, without a division
        for j in range(rays.L):
            E[:, j + 1] = E[:, j] * q[:, j] + P[:, j]
    return P, (2.0**-22 + alpha_width()) * E


def undecided(case, thr=THR):
    """[n] bool: some T_j, 1 <= j <= N, within U_j of thr.  NaN rays are decided (every evaluation stops at the NaN)."""
    T, U = transmittance64(case)
    j = np.arange(case.rays.L + 1)[None, :]
    with np.errstate(invalid="ignore"):
        return ((np.abs(T - thr) <= U) & (j >= 1) & (j <= case.rays.N[:, None])).any(1)


def count_bounds(case, thr=THR):
    """(M_lo, M_hi): the samples live beyond doubt and those that can be live; equal to the float64 count on a decided ray."""
    T, U = transmittance64(case)
    with np.errstate(invalid="ignore"):
        sure, maybe = case.rays.valid & (T[:, :-1] > thr + U[:, :-1]), case.rays.valid & (T[:, :-1] > thr - U[:, :-1])
    return np.cumprod(sure, 1).sum(1), np.cumprod(maybe, 1).sum(1)


# ------------------------------------------------------------------------------------------------------------------ the yardstick
FWD_QUANTITIES = ("w", "alphas", "R", "A", "D", "O", "rgb_out")
BWD_QUANTITIES = ("d_sdf", "d_cos", "d_rgbs", "d_aux", "d_inv_s")


def _bc(x, like):
    return np.broadcast_to(x, like.shape)


def forward_scales(rays, ref, bg):
    live = (np.arange(rays.L)[None, :] < ref["M"][:, None]).astype(np.float64)
    O = ref["O"]
    return {"w": (ref["w"], ref["T"]), "alphas": (ref["alphas"], live), "R": (ref["R"], _bc(O[:, None], ref["R"])),
            "A": (ref["A"], _bc(O[:, None], ref["A"])), "D": (ref["D"], np.sum(ref["w"] * np.abs(rays.t), 1)), "O": (O, O),
            "rgb_out": (ref["R"] + bg * (1 - O)[:, None], _bc((O + abs(bg) * (1 + O))[:, None], ref["R"]))}


def backward_scales(ref, bwd, g_rgb, g_aux):
    n = ref["T"].shape[0]
    g = np.abs(np.asarray(g_rgb, np.float64))
    ga = np.zeros((n, 3)) if g_aux is None else np.abs(np.asarray(g_aux, np.float64))
    return {"d_sdf": (bwd["d_sdf"], bwd["S_sdf"]), "d_cos": (bwd["d_cos"], bwd["S_cos"]),
            "d_rgbs": (bwd["d_rgbs"], g[:, None, :] * ref["T"][:, :, None]), "d_aux": (bwd["d_aux"], ga[:, None, :] * ref["T"][:, :, None]),
            "ds_ray": (bwd["ds_ray"], bwd["S_ray"]),
            "d_inv_s": (np.reshape(bwd["d_inv_s"], (1,)), np.reshape(bwd["S_inv_s"], (1,)))}


def rgb_out32(fwd, bg):
    return fwd["R"] + (F(bg) * (F(1) - fwd["O"]))[:, None]


def case_e32(case, cot=None, bg=0.0, alter=""):
    """E32 of every quantity of the named set under the cotangents `cot` (dict g_rgb, g_aux, g_depth, g_opacity, g_ws; default: all
    of cotangents(case)) and the background bg -> (e32 dict, float64 forward, float64 backward).  NaN rays take no part."""
    rays = case.clean
    cot = cotangents(case.rays) if cot is None else cot
    if case.clean_rows is not None:
        cot = {k: (None if x is None else x[case.clean_rows]) for k, x in cot.items()}
    ref = forward64(rays, case.s, case.r)
    bwd = backward64(rays, ref, bg=bg, **cot)
    s32 = serial32_forward(rays, case.s, case.r, force_M=ref["M"], alter=alter)
    b32 = serial32_backward(rays, s32, bg=bg, **cot)
    got = dict(s32, rgb_out=rgb_out32(s32, bg), **{k: b32[k] for k in ("d_sdf", "d_cos", "d_rgbs", "d_aux", "ds_ray")})
    got["d_inv_s"] = np.reshape(b32["d_inv_s"], (1,))
    scales = dict(forward_scales(rays, ref, bg), **backward_scales(ref, bwd, cot["g_rgb"], cot["g_aux"]))
    with np.errstate(invalid="ignore"):
        e = {k: _e32(np.abs(np.asarray(got[k], np.float64) - v), np.asarray(sc, np.float64)) for k, (v, sc) in scales.items()}
    e["d_inv_s"] = max(e["d_inv_s"], e.pop("ds_ray"))
    return e, ref, bwd


def judge_counts(v, case, got_M):
    got_M = np.asarray(got_M, np.int64)
    lo, hi = count_bounds(case)
    M = forward64(case.rays, case.s, case.r)["M"]
    for i in np.flatnonzero(((got_M < lo) | (got_M > hi)) & ~case.nan_rows):
        v.failures.append("live count: ray %s has %d, the float64 model %d (admissible %d .. %d)" % (case.rays.names[i], got_M[i], M[i], lo[i], hi[i]))


def judge(case, got, e32, cot, bg=0.0, k=K, v=None):
    """got: dict M, w, alphas [n, L], R, A, D, O, rgb_out and (optionally) d_sdf, d_cos, d_rgbs, d_aux, d_inv_s of a float32 evaluation,
    in row order (all rows of the set).  The float64 model is re-run at got's live counts; rays named nan* are skipped."""
    v = Verdict() if v is None else v
    sel = np.flatnonzero(~case.nan_rows)
    judge_counts(v, case, got["M"])
    rays = case.rays.take(sel)
    M = np.clip(np.asarray(got["M"], np.int64)[sel], 0, rays.N)
    cot = {k_: (None if x is None else np.asarray(x)[sel]) for k_, x in cot.items()}
    ref = forward64(rays, case.s, case.r, force_M=M)
    live = np.arange(rays.L)[None, :] < M[:, None]
    scales = forward_scales(rays, ref, bg)
    has_bwd = "d_sdf" in got
    if has_bwd:
        bwd = backward64(rays, ref, bg=bg, **cot)
        scales.update(backward_scales(ref, bwd, cot["g_rgb"], cot["g_aux"]))
        scales.pop("ds_ray")
    for q, (val, scale) in scales.items():
        if q not in got or got[q] is None:
            continue
        g = np.asarray(got[q], np.float64)
        if q == "d_inv_s":
            if case.nan_rows.any():
                continue                                     # the sum over the launch holds the NaN ray's share
            _judge(v, _Named(["launch"]), q, g.reshape(1), val, scale, e32[q], k)
            continue
        g = g[sel]
        if g.ndim >= 2 and g.shape[1] == rays.L:             # per-sample: exact +0 behind the live count
            _judge_zeros(v, rays, q, np.asarray(got[q])[sel], M)
            g = np.where(live if g.ndim == 2 else live[:, :, None], g, 0.0)
        _judge(v, rays, q, g, val, np.asarray(scale, np.float64), e32[q], k)
    return v


class _Named:
    def __init__(self, names):
        self.names = names


# ------------------------------------------------------------------------------------------------------------------ the case table
class Case:
    """A named set: rays, the launch's s and r, and which rows hold a NaN."""

    def __init__(self, rays, s, r):
        self.rays, self.s, self.r = rays, float(F(s)), float(r)
        self.nan_rows = np.array([nm.startswith("nan") for nm in rays.names])
        self.clean_rows = np.flatnonzero(~self.nan_rows) if self.nan_rows.any() else None
        self.clean = rays.take(self.clean_rows) if self.nan_rows.any() else rays

    def prefix(self, m):
        return Case(self.rays.take(np.arange(m)), self.s, self.r)


def _track(rng, n):
    t, dl = np.zeros(n), np.zeros(n)
    pos = 0.05 + 0.45 * rng.random()
    for j in range(n):
        dl[j] = pos / 256 + 1.7e-3
        t[j] = pos + 0.5 * dl[j]
        pos += dl[j]
    return t.astype(F), dl.astype(F)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _ray(rng, name, f, c):
    n = len(f)
    t, dl = _track(rng, n)
    return (name, np.asarray(f, F), np.asarray(c, F), dl, t, rng.random((n, 3)).astype(F), _unit(rng, n))


def _crossing(rng, name, n, hit=None, back=False):
    """A ray that meets a surface after a fraction `hit` of its samples: f falls linearly (slope = the cosine), plus a little noise."""
    hit = (0.2 + 0.6 * rng.random()) if hit is None else hit
    cos = -(0.25 + 0.7 * rng.random())
    j0 = hit * n
    f = -cos * 2e-3 * (j0 - np.arange(n)) + 2e-4 * rng.standard_normal(n)
    c = np.clip(cos + 0.05 * rng.standard_normal(n), -0.95, -0.05)
    return _ray(rng, name, f, -c if back else c)


def _front(rng, name, n):
    return _ray(rng, name, 0.2 + 0.2 * rng.random(n), -(0.1 + 0.8 * rng.random(n)))


def _lengths(rng):
    rays = []
    for n in (0, 1, 2, 63, 64, 65, 128, 129, 300):
        rays.append(_front(rng, "front_N%d" % n, n))
        rays.append(_crossing(rng, "cross_N%d" % n, n))
    return rays


def _placed(rng, depth, tag):
    """Samples in front of the surface (a ~ 1e-5), then one far inside at sample k - 1: exactly k live samples."""
    rays = []
    for k in (1, 2, 63, 64, 65, 127, 128):
        for n in (k, k + 1, k + 70):
            name, f, c, dl, t, col, ax = _front(rng, "%s_k%d_N%d" % (tag, k, n), n)
            f[k - 1:] = -depth
            rays.append((name, f, c, dl, t, col, ax))
    return rays


def _inside(rng):
    rays = []
    for n in (1, 5, 64, 70, 129):
        rays.append(_ray(rng, "inside_N%d" % n, -(0.2 + 0.2 * rng.random(n)), -(0.1 + 0.8 * rng.random(n))))
    return rays + [_crossing(rng, "cross%d" % i, 150) for i in range(6)]


def _backfacing(rng):
    rays = [_ray(rng, "back_front_N%d" % n, 0.2 + 0.2 * rng.random(n), 0.1 + 0.8 * rng.random(n)) for n in (1, 64, 129)]
    rays += [_crossing(rng, "back_cross%d" % i, 200, back=True) for i in range(6)]
    return rays + [_crossing(rng, "cross%d" % i, 200) for i in range(4)]


def _mixed(rng, n_rays, tag="mix"):
    rays = []
    for i in range(n_rays):
        n = int(rng.integers(1, 300))
        kind = i % 4
        if kind == 0:
            rays.append(_front(rng, "%s%d_front_N%d" % (tag, i, n), n))
        elif kind == 3:
            rays.append(_crossing(rng, "%s%d_back_N%d" % (tag, i, n), n, back=True))
        else:
            rays.append(_crossing(rng, "%s%d_cross_N%d" % (tag, i, n), n))
    return rays


def _hovering(rng, s, r):
    """Crossing rays whose float64 T_j is tuned to thr (1 + a few 1e-8) at one sample by bisection on that sample's f: the class a
    float32 evaluation may count one sample off.  The rest of the set is ordinary."""
    rays = _mixed(rng, 12, "hov_plain")
    for i, j in enumerate((5, 40, 64, 130)):
        name, f, c, dl, t, col, ax = _front(rng, "hover%d_j%d" % (i, j), j + 40)
        f[:j - 1] = 0.004 - 0.008 * np.arange(j - 1) / max(j - 1, 1)            # a gentle crossing: T stays well above thr
        f[j:] = -0.05
        one = make_rays([(name, f, c, dl, t, col, ax)])
        T_before = float(np.prod(opacity(one, s, r, np.float64)["q"][0, :j - 1]))
        target = THR * (1.0 + 3e-8 * rng.standard_normal()) / T_before            # 1 - a of sample j - 1
        lo, hi = -1.0, 1.0                                                       # q grows with f
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            f[j - 1] = mid
            qm = float(opacity(make_rays([(name, f, c, dl, t, col, ax)]), s, r, np.float64)["q"][0, j - 1])
            lo, hi = (mid, hi) if qm < target else (lo, mid)
        f[j - 1] = F(lo)
        rays.append((name, f, c, dl, t, col, ax))
    return rays


def case_table():
    """name -> Case.  Every ray is generated once from a fixed seed."""
    if _TABLE:
        return _TABLE
    T = _TABLE
    T["lengths"] = Case(make_rays(_lengths(np.random.default_rng(201))), 64.0, 0.5)
    T["placed"] = Case(make_rays(_placed(np.random.default_rng(202), 0.1, "placed") + _mixed(np.random.default_rng(242), 4)), 400.0, 1.0)        # dies in lane 63 / lane 0 ...
    T["a_one"] = Case(make_rays(_placed(np.random.default_rng(203), 0.3, "a_one") + _mixed(np.random.default_rng(243), 4)), 3000.0, 0.0)         # ... with 1 - a exactly 0
    T["front"] = Case(make_rays([_front(np.random.default_rng(204 + n), "front_N%d" % n, n) for n in (1, 7, 64, 100, 129, 257)]), 64.0, 1.0)
    T["inside"] = Case(make_rays(_inside(np.random.default_rng(205))), 64.0, 0.5)
    T["backfacing"] = Case(make_rays(_backfacing(np.random.default_rng(206))), 64.0, 1.0)
    for s in (1.0, 64.0, 3000.0):
        for r in (0.0, 0.5, 1.0):
            T["s%g_r%g" % (s, r)] = Case(make_rays(_mixed(np.random.default_rng(int(210 + s + 10 * r)), 20)), s, r)
    # |f s| = 0.5 * 3000: exp overflows in float32 on both sides of the surface
    far = [_ray(np.random.default_rng(230 + i), "far%d" % i, sign * np.full(n, 0.5), -np.full(n, 0.5)) for i, (sign, n) in
           enumerate(((1, 3), (1, 70), (-1, 3), (-1, 70)))]
    T["overflow"] = Case(make_rays(far + _mixed(np.random.default_rng(231), 8)), 3000.0, 0.5)
    nan = _mixed(np.random.default_rng(232), 9)
    name, f, c, dl, t, col, ax = _crossing(np.random.default_rng(233), "nan_f_N100", 100, hit=0.9)
    f[17] = np.nan
    nan.insert(4, (name, f, c, dl, t, col, ax))
    name, f, c, dl, t, col, ax = _crossing(np.random.default_rng(234), "nan_c_N70", 70, hit=0.9)
    c[3] = np.nan
    nan.insert(8, (name, f, c, dl, t, col, ax))
    T["nan"] = Case(make_rays(nan), 64.0, 0.5)
    T["counts"] = Case(make_rays(_mixed(np.random.default_rng(235), 17, "cnt")), 200.0, 0.5)
    T["hovering"] = Case(make_rays(_hovering(np.random.default_rng(236), float(F(64.0)), 0.5)), 64.0, 0.5)
    return T


_TABLE = {}
RAY_COUNTS = (1, 3, 4, 5, 17)
HOVERING = "hovering"


def cotangents(rays, seed=7, g_aux=True, g_opacity=True, g_ws=True, g_depth=True):
    """Seeded upstream gradients for a set: dict g_rgb [n, 3], g_aux [n, 3], g_depth, g_opacity [n], g_ws [n, L] (float32 or None)."""
    rng = np.random.default_rng(seed)
    full = dict(g_rgb=rng.standard_normal((rays.n, 3)).astype(F), g_aux=rng.standard_normal((rays.n, 3)).astype(F),
                g_depth=rng.standard_normal(rays.n).astype(F), g_opacity=rng.standard_normal(rays.n).astype(F),
                g_ws=rng.standard_normal((rays.n, rays.L)).astype(F))
    for key, on in (("g_aux", g_aux), ("g_opacity", g_opacity), ("g_ws", g_ws), ("g_depth", g_depth)):
        if not on:
            full[key] = None
    return full


# ------------------------------------------------------------------------------------------------------------------ the buffer layout
class Layout:
    """Sample buffers and rays_a for an SRays batch the way the kernels see them: row r of rays_a is ray r with ray index ray_idx[r] (a
    permutation sample of range(n + 5): some output rows belong to no ray), sample ranges allocated in yet another order with 0-5
    unused samples between them, 64 spare rows at the end.  Unused samples hold finite junk."""

    def __init__(self, rays, seed):
        rng = np.random.default_rng(seed)
        n = rays.n
        self.rays, self.n, self.n_out = rays, n, n + 5
        self.ray_idx = rng.permutation(self.n_out)[:n].astype(np.int32)
        start, pos = np.zeros(n, np.int32), 0
        for r in rng.permutation(n):
            pos += int(rng.integers(0, 6))
            start[r] = pos
            pos += int(rays.N[r])
        self.S, self.start = pos + 64, start
        self.rays_a = np.stack([self.ray_idx, start, rays.N.astype(np.int32)], 1).astype(np.int32)
        self.sdf, self.cosv = self.flat(rays.f, 0.3), self.flat(rays.c, -0.5)
        self.deltas, self.ts = self.flat(rays.delta, 0.01), self.flat(rays.t, 1.0)
        self.rgbs, self.aux = self.flat(rays.rgb, 0.5), self.flat(rays.aux, 0.5)

    def flat(self, padded, fill=0.0):
        """[n, L, ...] -> [S, ...]."""
        out = np.full((self.S,) + padded.shape[2:], fill, padded.dtype)
        for r in range(self.n):
            out[self.start[r]:self.start[r] + self.rays.N[r]] = padded[r, :self.rays.N[r]]
        return out

    def per_ray(self, rows_values, fill=0.0):
        """[n, ...] in row order -> [n_out, ...] indexed by ray index."""
        out = np.full((self.n_out,) + rows_values.shape[1:], fill, rows_values.dtype)
        out[self.ray_idx] = rows_values
        return out

    def padded(self, flat):
        """[S, ...] kernel output -> [n, L, ...] in row order (0 outside the rays)."""
        out = np.zeros((self.n, self.rays.L) + flat.shape[1:], flat.dtype)
        for r in range(self.n):
            out[r, :self.rays.N[r]] = flat[self.start[r]:self.start[r] + self.rays.N[r]]
        return out

    def sample_mask(self, m=None):
        mask = np.zeros(self.S, bool)
        for r in range(self.n if m is None else m):
            mask[self.start[r]:self.start[r] + self.rays.N[r]] = True
        return mask

    def ray_mask(self, m=None):
        mask = np.zeros(self.n_out, bool)
        mask[self.ray_idx[:self.n if m is None else m]] = True
        return mask
