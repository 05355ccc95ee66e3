"""Float64 model of volume-render compositing, its two float32 evaluations, and the yardstick the compositing kernels are held to
(tests/test_composite_reference.py on the CPU, tests/test_gpu_composite_exact.py on the GPU).  numpy only: no GPU, no oracle.

The contract, per ray (the reference's serial loops volume_train.py:22-48 and volume_render_test.py:18-54):

    T = 1;  for j < N:  stop at the first !(T > thr);  a = 1 - exp(-sigma_j delta_j);  w_j = a T;  R += w_j c_j;  D += w_j t_j;
                        O += w_j;  T <- T (1 - a);  M += 1

Every function here works on a padded batch (`Rays`: [n, L] arrays, L a multiple of 64, ray i has N[i] samples) and is serial along
the ray; the batch axis only saves interpreter time.

  forward64 / backward64 / fused64 / test64   the contract in float64.  backward64 is a REVERSE SWEEP of the loop above (adjoint of T
                                              carried from the last live sample to the first); the closed form of SURVEY A.5 does not
                                              appear in it.  It also returns S, the same sweep with every term's absolute value.
  serial32_*                                  float32, the reference's serial order; the backward is the closed form of SURVEY A.5
                                              evaluated serially (the formula composite.hip commits to, with its `R - prefix`
                                              differences).
  wave32_*                                    float32 in composite.hip's order: Kogge-Stone inclusive scans over 64 lanes, per-lane
                                              partial sums across groups, a butterfly reduction, liveness as a prefix, carries
                                              between groups, a group skipped when T <= thr at its start.  `alter` switches on one of
                                              five deliberate defects; tests/test_composite_reference.py shows the yardstick
                                              catches each.

Every float32 rounding is a numpy float32 operation (multiply and add are separate calls: no contraction, as the library is built
with -ffp-contract=off); expf is numpy's float32 exp.

The yardstick (the one of tests/test_gpu_hash_input_grad.py).  For a named set of rays, E32 = max |serial32 - f64| / scale, with
    w_s: scale T_s (the absolute error of 1 - expf is an ulp of 1, not of a)     R, O, rgb_out: O, O, O + bg (1 + O)     D: sum w t
    d_sigma: the magnitude sum of the closed form's terms (closed_form_scale64)    d_rgbs: |g_rgb| T_s    sq_err: sq_err
and a result passes when |got - f64| <= K E32 scale + TINY.  serial32 is run with the float64 model's live counts, so that E32
measures arithmetic and not a different decision.

Decidability of the live count M.  A ray is UNDECIDED when some float64 T_j (1 <= j <= N) lies within U_j of thr,
    U_j = 2^-22 sum_{i<j} T_j / (1 - a_i)        (= thr sum_{i<j} 2^-22 / (1 - a_i) at T_j = thr:
the absolute error of a float32 `1 - a_i` is a few 2^-24, i.e. 2^-22 / (1 - a_i) relative, and it reaches T_j multiplied by the other
factors).  Written with T_j / (1 - a_i) = prod_{l<j, l != i} (1 - a_l) <= 1 it stays finite when a float32 1 - a_i is exactly zero
(sigma delta = 100: T is then exactly 0 on every side, nothing is undecided about it).  count_bounds turns the same U_j into the
interval a float32 count must lie in: the samples live beyond doubt (T_j > thr + U_j) .. the samples that can be live (T_j > thr - U_j).
On a decided ray that is M exactly; on a ray that crosses thr in one step M +- 1; only on a plateau (zero-density samples AT the
threshold, the case the kernels' prefix ballot exists for) is it wider.  The model is re-run with force_M set to the count under test,
so that no value of any ray goes unchecked."""
import numpy as np

F = np.float32
THR32 = F(1e-4)
THR = float(THR32)
TINY = 1e-30
K = 4                       # a tree order against a serial order: the factor of both hash-gradient suites (see PARITY_NOTES)
WAVE = 64
SENTINEL = -7.0             # pre-fill of every output buffer


class Rays:
    """A padded batch: sigma, delta, t [n, L] float32, rgb [n, L, 3] float32 (fp16 inputs widened), N [n], names [n]."""

    def __init__(self, sigma, delta, t, rgb, N, names):
        self.sigma, self.delta, self.t, self.rgb = (np.ascontiguousarray(x, F) for x in (sigma, delta, t, rgb))
        self.N, self.names = np.asarray(N, np.int64), list(names)
        self.n, self.L = self.sigma.shape
        assert self.L % WAVE == 0 and self.N.max(initial=0) <= self.L and len(self.names) == self.n
        self.valid = np.arange(self.L)[None, :] < self.N[:, None]

    def take(self, rows):
        rows = np.asarray(rows)
        return Rays(self.sigma[rows], self.delta[rows], self.t[rows], self.rgb[rows], self.N[rows], [self.names[i] for i in rows])

    def with_rgb(self, rgb):
        return Rays(self.sigma, self.delta, self.t, rgb, self.N, self.names)


def make_rays(ray_list):
    """ray_list: [(name, sigma [N], delta [N], t [N], rgb [N, 3])] -> Rays."""
    n = len(ray_list)
    L = max(WAVE, -(-max(len(r[1]) for r in ray_list) // WAVE) * WAVE)
    sigma, delta, t, rgb = np.zeros((n, L), F), np.ones((n, L), F), np.ones((n, L), F), np.zeros((n, L, 3), F)
    for i, (_, s, d, tt, c) in enumerate(ray_list):
        m = len(s)
        sigma[i, :m], delta[i, :m], t[i, :m], rgb[i, :m] = s, d, tt, c
    return Rays(sigma, delta, t, rgb, [len(r[1]) for r in ray_list], [r[0] for r in ray_list])


# ------------------------------------------------------------------------------------------------------------------ float64
def forward64(rays, thr=THR, force_M=None):
    """-> dict M [n], T [n, L] (transmittance BEFORE sample j; 0 where the sample is not live), a, q = 1 - a, w [n, L], R [n, 3], D, O."""
    n, L = rays.n, rays.L
    with np.errstate(invalid="ignore", over="ignore"):
        sd = rays.sigma.astype(np.float64) * rays.delta.astype(np.float64)
        a, q = -np.expm1(-sd), np.exp(-sd)
        T, alive = np.ones(n), np.ones(n, bool)
        Ts, w, M = np.zeros((n, L)), np.zeros((n, L)), np.zeros(n, np.int64)
        for j in range(L):
            live = (alive & (j < rays.N) & (T > thr)) if force_M is None else (j < np.asarray(force_M))
            alive = live
            Ts[:, j] = np.where(live, T, 0.0)
            w[:, j] = np.where(live, a[:, j] * T, 0.0)
            T = np.where(live, T * q[:, j], T)
            M += live
        c = rays.rgb.astype(np.float64)
        return dict(M=M, T=Ts, a=a, q=q, w=w, R=np.einsum("nj,njc->nc", w, c), D=np.sum(w * rays.t, 1), O=np.sum(w, 1))


def backward64(rays, fwd, g_rgb, g_depth=None, g_opacity=None, g_ws=None):
    """Reverse sweep of the serial loop on the live samples of `fwd`.  -> d_sigma [n, L], d_rgbs [n, L, 3], S [n, L]."""
    n, L = rays.n, rays.L
    g_rgb = np.asarray(g_rgb, np.float64)
    g_depth = np.zeros(n) if g_depth is None else np.asarray(g_depth, np.float64)
    g_opacity = np.zeros(n) if g_opacity is None else np.asarray(g_opacity, np.float64)
    g_ws = np.zeros((n, L)) if g_ws is None else np.asarray(g_ws, np.float64)
    c, t, dl = rays.rgb.astype(np.float64), rays.t.astype(np.float64), rays.delta.astype(np.float64)
    T, a, q, M = fwd["T"], fwd["a"], fwd["q"], fwd["M"]
    Tbar, Tabs = np.zeros(n), np.zeros(n)                  # adjoint of the transmittance AFTER sample j, and its magnitude sum
    d_sigma, S = np.zeros((n, L)), np.zeros((n, L))
    with np.errstate(invalid="ignore"):
        for j in range(L - 1, -1, -1):
            live = j < M
            wbar = np.sum(g_rgb * c[:, j], 1) + g_depth * t[:, j] + g_opacity + g_ws[:, j]                # adjoint of w_j
            wabs = np.sum(np.abs(g_rgb * c[:, j]), 1) + np.abs(g_depth * t[:, j]) + np.abs(g_opacity) + np.abs(g_ws[:, j])
            abar = wbar * T[:, j] - Tbar * T[:, j]                                                        # w = a T;  T+ = T (1 - a)
            aabs = wabs * T[:, j] + Tabs * T[:, j]
            dadsig = dl[:, j] * q[:, j]                                                                   # a = 1 - exp(-sigma delta)
            d_sigma[:, j] = np.where(live, abar * dadsig, 0.0)
            S[:, j] = np.where(live, aabs * dadsig, 0.0)
            Tbar = np.where(live, wbar * a[:, j] + Tbar * q[:, j], Tbar)
            Tabs = np.where(live, wabs * a[:, j] + Tabs * q[:, j], Tabs)
    return d_sigma, g_rgb[:, None, :] * fwd["w"][:, :, None], S


def closed_form_scale64(rays, fwd, g_rgb, g_depth=None, g_opacity_mag=None, g_ws=None):
    """Magnitude sum of the terms of SURVEY A.5's closed form, per sample: the scale of d_sigma's yardstick (the float32 evaluations
    form R - prefix, D - prefix, 1 - O, W - prefix, whose rounding is an ulp of R, D, 1, W and not of the difference).
    g_opacity_mag: the magnitude of the opacity gradient's terms (|g_opacity| + |bg| sum_c |g_rgb_c| under a background blend)."""
    n, L = rays.n, rays.L
    ag = np.abs(np.asarray(g_rgb, np.float64))
    agd = np.zeros(n) if g_depth is None else np.abs(np.asarray(g_depth, np.float64))
    ago = np.zeros(n) if g_opacity_mag is None else np.abs(np.asarray(g_opacity_mag, np.float64))
    agw = np.zeros((n, L)) if g_ws is None else np.abs(np.asarray(g_ws, np.float64))
    c, t, dl = np.abs(rays.rgb.astype(np.float64)), np.abs(rays.t.astype(np.float64)), rays.delta.astype(np.float64)
    w = fwd["w"]
    Tp = fwd["T"] * fwd["q"]
    wc = w[:, :, None] * c
    pr, pd, pw = np.cumsum(wc, 1), np.cumsum(w * t, 1), np.cumsum(agw * w, 1)
    acc = np.sum(ag[:, None, :] * (c * Tp[:, :, None] + pr[:, -1:, :] + pr), 2)
    acc += agd[:, None] * (t * Tp + pd[:, -1:] + pd) + (ago * (1 + fwd["O"]))[:, None] + agw * Tp + pw[:, -1:] + pw
    return np.where(np.arange(L)[None, :] < fwd["M"][:, None], dl * acc, 0.0)


def fused64(rays, target, bg, loss_scale, n_rays, thr=THR, force_M=None):
    """The trainer's fused contract: composite, MSE gradient of the blended colour, backward with g_depth = g_ws = 0."""
    fwd = forward64(rays, thr, force_M)
    err = fwd["R"] + bg * (1 - fwd["O"])[:, None] - np.asarray(target, np.float64)
    g_rgb = 2.0 / (3.0 * n_rays) * loss_scale * err
    g_op = -bg * g_rgb.sum(1)
    d_sigma, d_rgbs, S = backward64(rays, fwd, g_rgb, None, g_op, None)
    scale = closed_form_scale64(rays, fwd, g_rgb, None, abs(bg) * np.abs(g_rgb).sum(1), None)
    return dict(fwd, sq_err=np.sum(err * err, 1), g_rgb=g_rgb, d_sigma=d_sigma, d_rgbs=d_rgbs, S=S, ds_scale=scale)


def transmittance64(rays, T0=None):
    """T_j after j samples, j = 0 .. L, never stopped: [n, L + 1], and U_j of the decidability rule."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.exp(-(rays.sigma.astype(np.float64) * rays.delta.astype(np.float64)))
        q = np.where(rays.valid, q, 1.0)
        T0 = np.ones(rays.n) if T0 is None else np.asarray(T0, np.float64)
        P = np.concatenate([np.ones((rays.n, 1)), np.cumprod(q, 1)], 1)
        E = np.zeros_like(P)                                 # E_j = sum_{i<j} prod_{l<j, l != i} q_l, without a division:
        for j in range(rays.L):                              # E_{j+1} = E_j q_j + P_j
            E[:, j + 1] = E[:, j] * q[:, j] + P[:, j]
    return T0[:, None] * P, 2.0**-22 * T0[:, None] * E


def undecided(rays, thr=THR, T0=None, extra_rel=0.0):
    """[n] bool: some T_j, 1 <= j <= N, within U_j (+ extra_rel T_j: a rounded starting value) of thr.  NaN rays are decided (every
    evaluation stops at the NaN)."""
    T, U = transmittance64(rays, T0)
    j = np.arange(rays.L + 1)[None, :]
    with np.errstate(invalid="ignore"):
        near = (np.abs(T - thr) <= U + extra_rel * T) & (j >= 1) & (j <= rays.N[:, None])
    return near.any(1)


def count_bounds(rays, thr=THR):
    """(M_lo, M_hi): the samples that are live beyond doubt (T_j > thr + U_j on the whole prefix) and those that can be live
    (T_j > thr - U_j).  Equal to the float64 live count on a decided ray; M +- 1 on a ray that crosses thr in one step; a whole
    stretch on a PLATEAU (samples of zero density at T = thr: every one of them is at the threshold, in any arithmetic)."""
    T, U = transmittance64(rays)
    inray = np.arange(rays.L)[None, :] < rays.N[:, None]
    with np.errstate(invalid="ignore"):
        sure, maybe = inray & (T[:, :-1] > thr + U[:, :-1]), inray & (T[:, :-1] > thr - U[:, :-1])
    return np.cumprod(sure, 1).sum(1), np.cumprod(maybe, 1).sum(1)


def test64(rays, opacity_in, thr=THR, force_steps=None):
    """Test-time composite of one march round (volume_render_test.py:18-54): starts from T = 1 - opacity_in, includes the sample that
    brings T to <= thr, then stops.  -> dict steps [n] (samples composited), dead [n] (alive <- -1), R, D, O (the increments)."""
    n, L = rays.n, rays.L
    sd = rays.sigma.astype(np.float64) * rays.delta.astype(np.float64)
    a, q = -np.expm1(-sd), np.exp(-sd)
    T = 1.0 - np.asarray(opacity_in, np.float64)
    run = rays.N > 0
    dead = rays.N == 0
    w, steps = np.zeros((n, L)), np.zeros(n, np.int64)
    for j in range(L):
        go = (run & (j < rays.N)) if force_steps is None else (j < np.asarray(force_steps))
        w[:, j] = np.where(go, a[:, j] * T, 0.0)
        T = np.where(go, T * q[:, j], T)
        steps += go
        stop = go & (T <= thr)
        dead |= stop
        run = go & ~stop
    if force_steps is not None:
        dead = (rays.N == 0) | (np.asarray(force_steps) < rays.N)
    return dict(steps=steps, dead=dead, w=w, R=np.einsum("nj,njc->nc", w, rays.rgb.astype(np.float64)), D=np.sum(w * rays.t, 1),
                O=np.sum(w, 1))


def distortion_loss64(ws, ts, deltas):
    """One ray of the distortion loss (modules/distortion.py:15-84) in float64."""
    wv, tv = np.asarray(ws, np.float64), np.asarray(ts, np.float64)
    wi, wti = np.cumsum(wv), np.cumsum(wv * tv)
    return np.sum(2 * (wti * (wi - wv) - wi * (wti - wv * tv)) + wv * wv * deltas / 3)


def distortion_grad64(g, ws, ts, deltas):
    """d(g * loss) / d ws of one ray (modules/distortion.py:86-119) in float64; at least one sample."""
    wv, tv, dv = np.asarray(ws, np.float64), np.asarray(ts, np.float64), np.asarray(deltas, np.float64)
    wi, wti = np.cumsum(wv), np.cumsum(wv * tv)
    sel = np.concatenate([[0.0], tv[1:] * wi[:-1] - wti[:-1]])
    return g * 2 * (sel + (wti[-1] - wti - tv * (wi[-1] - wi))) + g * (2.0 / 3.0) * wv * dv


# ------------------------------------------------------------------------------------------------------------------ float32, serial
def _alpha32(rays, j):
    return F(1) - np.exp(-rays.sigma[:, j] * rays.delta[:, j])


def serial32_forward(rays, thr=THR32, force_M=None):
    n, L = rays.n, rays.L
    T, alive = np.ones(n, F), np.ones(n, bool)
    R, D, O, M = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.int64)
    w, Ts = np.zeros((n, L), F), np.zeros((n, L), F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(L):
            live = (alive & (j < rays.N) & (T > thr)) if force_M is None else (j < np.asarray(force_M))
            alive = live
            a = _alpha32(rays, j)
            wj = np.where(live, a * T, F(0))
            w[:, j], Ts[:, j] = wj, np.where(live, T, F(0))
            for k in range(3):
                R[:, k] = np.where(live, R[:, k] + wj * rays.rgb[:, j, k], R[:, k])
            D = np.where(live, D + wj * rays.t[:, j], D)
            O = np.where(live, O + wj, O)
            T = np.where(live, T * (F(1) - a), T)
            M += live
    return dict(M=M, w=w, T=Ts, R=R, D=D, O=O)


def serial32_backward(rays, fwd, g_rgb, g_depth=None, g_opacity=None, g_ws=None):
    """SURVEY A.5's closed form, serially in float32, on the float32 forward `fwd` (its w, T, R, D, O, M)."""
    n, L = rays.n, rays.L
    g_rgb = np.asarray(g_rgb, F)
    gd = np.zeros(n, F) if g_depth is None else np.asarray(g_depth, F)
    go = np.zeros(n, F) if g_opacity is None else np.asarray(g_opacity, F)
    R, D, O, M = fwd["R"], fwd["D"], fwd["O"], fwd["M"]
    W = np.zeros(n, F)
    if g_ws is not None:
        g_ws = np.asarray(g_ws, F)
        for j in range(L):
            W = np.where(j < M, W + g_ws[:, j] * fwd["w"][:, j], W)
    pr, pd, pw = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F)
    d_sigma, d_rgbs = np.zeros((n, L), F), np.zeros((n, L, 3), F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(L):
            live = j < M
            a = _alpha32(rays, j)
            w, Tp = fwd["w"][:, j], fwd["T"][:, j] * (F(1) - a)
            acc = np.zeros(n, F)
            for k in range(3):
                pr[:, k] = np.where(live, pr[:, k] + w * rays.rgb[:, j, k], pr[:, k])
                acc = acc + g_rgb[:, k] * (rays.rgb[:, j, k] * Tp - (R[:, k] - pr[:, k]))
                d_rgbs[:, j, k] = np.where(live, g_rgb[:, k] * w, F(0))
            pd = np.where(live, pd + w * rays.t[:, j], pd)
            acc = acc + gd * (rays.t[:, j] * Tp - (D - pd))
            acc = acc + go * (F(1) - O)
            if g_ws is not None:
                pw = np.where(live, pw + g_ws[:, j] * w, pw)
                acc = acc + (g_ws[:, j] * Tp - (W - pw))
            d_sigma[:, j] = np.where(live, rays.delta[:, j] * acc, F(0))
    return d_sigma, d_rgbs


def _mse_grad32(R, O, target, bg, loss_scale, n_rays):
    """The float32 operations of the fused kernel between its two passes."""
    k = F(2) / (F(3) * F(n_rays)) * F(loss_scale)
    b = F(bg) * (F(1) - O)
    err = (R + b[:, None]) - np.asarray(target, F)
    g_rgb = k * err
    g_op = -F(bg) * ((g_rgb[:, 0] + g_rgb[:, 1]) + g_rgb[:, 2])
    return (err[:, 0] * err[:, 0] + err[:, 1] * err[:, 1]) + err[:, 2] * err[:, 2], g_rgb, g_op


def serial32_fused(rays, target, bg, loss_scale, n_rays, thr=THR32, force_M=None):
    fwd = serial32_forward(rays, thr, force_M)
    sq, g_rgb, g_op = _mse_grad32(fwd["R"], fwd["O"], target, bg, loss_scale, n_rays)
    d_sigma, d_rgbs = serial32_backward(rays, fwd, g_rgb, None, g_op, None)
    return dict(fwd, sq_err=sq, d_sigma=d_sigma, d_rgbs=d_rgbs)


def serial32_test(rays, opacity_in, thr=THR32, force_steps=None):
    """composite_test_kernel's own order (it is serial): -> dict steps, dead, and the FINAL accumulators given the initial ones."""
    n, L = rays.n, rays.L
    T = F(1) - np.asarray(opacity_in, F)
    run, dead = rays.N > 0, rays.N == 0
    R, D, O, steps = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.int64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(L):
            go = (run & (j < rays.N)) if force_steps is None else (j < np.asarray(force_steps))
            a = _alpha32(rays, j)
            w = a * T
            for k in range(3):
                R[:, k] = np.where(go, R[:, k] + w * rays.rgb[:, j, k], R[:, k])
            D = np.where(go, D + w * rays.t[:, j], D)
            O = np.where(go, O + w, O)
            T = np.where(go, T * (F(1) - a), T)
            steps += go
            stop = go & (T <= thr)
            dead = dead | stop
            run = go & ~stop
    return dict(steps=steps, dead=dead, R=R, D=D, O=O)


# ------------------------------------------------------------------------------------------------------------------ float32, wave order
ALTERATIONS = {
    "a": "the prefix-sum carry cr* is not passed to the next 64-sample group",
    "b": "the transmittance carry uses lane 62 instead of lane 63",
    "c": "liveness is the raw per-lane Ts > thr (no prefix ballot), and a dead group does not zero T",
    "d": "g_opacity omits the -bg sum g_rgb share",
    "e": "the skipped-group branch leaves ws / d_sigmas unwritten",
}


def _scan(v, mul):
    """Kogge-Stone inclusive scan along the 64 lanes (ngp_device.h wave_scan_mul / wave_scan_add)."""
    v = v.copy()
    d = 1
    while d < WAVE:
        o = v[:, :-d].copy()
        v[:, d:] = v[:, d:] * o if mul else v[:, d:] + o
        d <<= 1
    return v


def _butterfly(v):
    """wave_sum: every lane ends with the total; lane 0's is taken."""
    lanes = np.arange(WAVE)
    d = 32
    while d >= 1:
        v = v + v[:, lanes ^ d]
        d >>= 1
    return v[:, 0]


def _wave_group(rays, base, T, thr, alter):
    """One 64-sample group of every ray, the part all three kernels share: -> run, skip (per ray), valid, live (per lane), a, Ts, w, T'."""
    n = rays.n
    sl = slice(base, base + WAVE)
    active = base < rays.N
    valid = rays.valid[:, sl] & active[:, None]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        run = active & (T > thr)
        skip = active & ~run
        a = np.where(valid, F(1) - np.exp(-rays.sigma[:, sl] * rays.delta[:, sl]), F(0))
        incl = _scan(F(1) - a, True)
        excl = np.concatenate([np.ones((n, 1), F), incl[:, :-1]], 1)
        Ts = T[:, None] * excl
        dead = valid & ~(Ts > thr)
        if "c" in alter:
            live = valid & ~dead
        else:
            first = np.where(dead.any(1), dead.argmax(1), WAVE)
            live = valid & (np.arange(WAVE)[None, :] < first[:, None])
        live = live & run[:, None]
        w = np.where(live, a * Ts, F(0))
        last = incl[:, WAVE - 2] if "b" in alter else incl[:, WAVE - 1]
        Tn = T * last if "c" in alter else np.where(dead.any(1), F(0), T * last)
        Tn = np.where(run, Tn, T)
    return run, skip, valid, live, a, Ts, w, Tn.astype(F)


def wave32_forward(rays, thr=THR32, alter=""):
    """composite_fwd_kernel / pass 1 of the fused kernel.  ws starts as SENTINEL: what the kernel does not write stays."""
    n, L = rays.n, rays.L
    T = np.ones(n, F)
    part = np.zeros((5, n, WAVE), F)                        # per-lane partial sums r0 r1 r2 dep op
    cnt = np.zeros(n, np.int64)
    ws = np.full((n, L), SENTINEL, F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for base in range(0, L, WAVE):
            sl = slice(base, base + WAVE)
            run, skip, valid, live, a, Ts, w, T = _wave_group(rays, base, T, thr, alter)
            if "e" not in alter:
                ws[:, sl] = np.where(valid & skip[:, None], F(0), ws[:, sl])
            ws[:, sl] = np.where(valid & run[:, None], w, ws[:, sl])
            for k in range(3):
                part[k] = part[k] + w * rays.rgb[:, sl, k]
            part[3] = part[3] + w * rays.t[:, sl]
            part[4] = part[4] + w
            cnt += live.sum(1)
        R = np.stack([_butterfly(part[k]) for k in range(3)], 1)
    return dict(M=cnt, w=ws, R=R, D=_butterfly(part[3]), O=_butterfly(part[4]))


def wave32_backward(rays, fwd, g_rgb, g_depth=None, g_opacity=None, g_ws=None, bg=0.0, thr=THR32, alter=""):
    """composite_bwd_kernel / pass 2 of the fused kernel, on the forward outputs `fwd` (R, D, O, w as the forward kernel stored
    them).  g_rgb is the gradient of the blended colour when bg != 0.  -> d_sigma [n, L], d_rgbs [n, L, 3] (SENTINEL where unwritten)."""
    n, L = rays.n, rays.L
    g_rgb = np.asarray(g_rgb, F)
    gd = np.zeros(n, F) if g_depth is None else np.asarray(g_depth, F)
    go = np.zeros(n, F) if g_opacity is None else np.asarray(g_opacity, F)
    if bg != 0.0 and "d" not in alter:
        go = go + -F(bg) * ((g_rgb[:, 0] + g_rgb[:, 1]) + g_rgb[:, 2])
    R, D, O = fwd["R"], fwd["D"], fwd["O"]
    d_sigma, d_rgbs = np.full((n, L), SENTINEL, F), np.full((n, L, 3), SENTINEL, F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        W = np.zeros(n, F)
        if g_ws is not None:
            g_ws = np.asarray(g_ws, F)
            part = np.zeros((n, WAVE), F)
            for base in range(0, L, WAVE):
                sl = slice(base, base + WAVE)
                part = np.where(rays.valid[:, sl], part + g_ws[:, sl] * fwd["w"][:, sl], part)
            W = _butterfly(part)
        T = np.ones(n, F)
        carry = np.zeros((5, n), F)                         # cr0 cr1 cr2 cd cw
        for base in range(0, L, WAVE):
            sl = slice(base, base + WAVE)
            run, skip, valid, live, a, Ts, w, T = _wave_group(rays, base, T, thr, alter)
            Tp = Ts * (F(1) - a)
            c, tm, dl = rays.rgb[:, sl], np.where(valid, rays.t[:, sl], F(0)), np.where(valid, rays.delta[:, sl], F(0))
            c = np.where(valid[:, :, None], c, F(0))
            p = [carry[k][:, None] + _scan(w * c[:, :, k], False) for k in range(3)]
            pd = carry[3][:, None] + _scan(w * tm, False)
            acc = (g_rgb[:, 0:1] * (c[:, :, 0] * Tp - (R[:, 0:1] - p[0])) + g_rgb[:, 1:2] * (c[:, :, 1] * Tp - (R[:, 1:2] - p[1]))) \
                + g_rgb[:, 2:3] * (c[:, :, 2] * Tp - (R[:, 2:3] - p[2]))
            acc = acc + gd[:, None] * (tm * Tp - (D[:, None] - pd))
            acc = acc + (go * (F(1) - O))[:, None]
            if g_ws is not None:
                gw = np.where(valid, g_ws[:, sl], F(0))
                pw = carry[4][:, None] + _scan(gw * w, False)
                acc = acc + (gw * Tp - (W[:, None] - pw))
            ds = np.where(live, dl * acc, F(0))
            dc = np.where(live[:, :, None], g_rgb[:, None, :] * w[:, :, None], F(0))
            wr = valid & run[:, None]
            zero = valid & skip[:, None] if "e" not in alter else np.zeros_like(valid)
            d_sigma[:, sl] = np.where(wr, ds, np.where(zero, F(0), d_sigma[:, sl]))
            d_rgbs[:, sl] = np.where(wr[:, :, None], dc, np.where(zero[:, :, None], F(0), d_rgbs[:, sl]))
            if "a" not in alter:
                for k in range(3):
                    carry[k] = np.where(run, p[k][:, WAVE - 1], carry[k])
                carry[3] = np.where(run, pd[:, WAVE - 1], carry[3])
                if g_ws is not None:
                    carry[4] = np.where(run, pw[:, WAVE - 1], carry[4])
    return d_sigma, d_rgbs


def wave32_fused(rays, target, bg, loss_scale, n_rays, thr=THR32, alter=""):
    """composite_train_fused_kernel: pass 1, the MSE gradient, pass 2 with g_depth = g_ws = 0 (its go = -bg sum g_rgb always)."""
    fwd = wave32_forward(rays, thr, alter)
    sq, g_rgb, g_op = _mse_grad32(fwd["R"], fwd["O"], target, bg, loss_scale, n_rays)
    if "d" in alter:
        g_op = np.zeros_like(g_op)
    d_sigma, d_rgbs = wave32_backward(rays, fwd, g_rgb, None, g_op, None, 0.0, thr, alter)
    return dict(fwd, sq_err=sq, d_sigma=d_sigma, d_rgbs=d_rgbs)


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def _e32(err, scale):
    m = scale > 0
    assert np.all(err[~m] == 0), "a float32 error where the scale is zero"
    return float(np.max(err[m] / scale[m])) if m.any() else 0.0


def _bcast(x, like):
    return np.broadcast_to(x, like.shape)


def forward_scales(ref, rays, bg):
    """quantity -> (float64 value, scale) of the forward outputs."""
    out = {"w": (ref["w"], ref["T"]), "R": (ref["R"], _bcast(ref["O"][:, None], ref["R"])), "D": (ref["D"], np.sum(ref["w"] * np.abs(rays.t), 1)),
           "O": (ref["O"], ref["O"])}
    if bg is not None:
        out["rgb_out"] = (ref["R"] + bg * (1 - ref["O"])[:, None], _bcast((ref["O"] + abs(bg) * (1 + ref["O"]))[:, None], ref["R"]))
    return out


def forward_e32(rays, bg=None):
    """E32 of the forward quantities on this set: quantity -> float; and the float64 model (decided counts)."""
    ref = forward64(rays)
    s32 = serial32_forward(rays, force_M=ref["M"])
    got = dict(s32)
    if bg is not None:
        got["rgb_out"] = s32["R"] + (F(bg) * (F(1) - s32["O"]))[:, None]
    return {q: _e32(np.abs(got[q].astype(np.float64) - v), s) for q, (v, s) in forward_scales(ref, rays, bg).items()}, ref


def backward_scales(rays, ref, d_sigma, d_rgbs, g_rgb, g_depth, g_op_mag, g_ws):
    g = np.abs(np.asarray(g_rgb, np.float64))
    return {"d_sigma": (d_sigma, closed_form_scale64(rays, ref, g_rgb, g_depth, g_op_mag, g_ws)),
            "d_rgbs": (d_rgbs, g[:, None, :] * ref["T"][:, :, None])}


def _go_parts(n, g_rgb, g_opacity, bg):
    go = np.zeros(n) if g_opacity is None else np.asarray(g_opacity, np.float64)
    g = np.asarray(g_rgb, np.float64)
    return go - bg * g.sum(1), np.abs(go) + abs(bg) * np.abs(g).sum(1)


def backward_e32(rays, g_rgb, g_depth=None, g_opacity=None, g_ws=None, bg=0.0):
    ref = forward64(rays)
    go, go_mag = _go_parts(rays.n, g_rgb, g_opacity, bg)
    ds, dc, _ = backward64(rays, ref, g_rgb, g_depth, go, g_ws)
    s32 = serial32_forward(rays, force_M=ref["M"])
    go32 = (np.zeros(rays.n, F) if g_opacity is None else np.asarray(g_opacity, F))
    if bg != 0.0:
        g = np.asarray(g_rgb, F)
        go32 = go32 + -F(bg) * ((g[:, 0] + g[:, 1]) + g[:, 2])
    ds32, dc32 = serial32_backward(rays, s32, g_rgb, g_depth, go32, g_ws)
    got = {"d_sigma": ds32, "d_rgbs": dc32}
    return {q: _e32(np.abs(got[q].astype(np.float64) - v), s)
            for q, (v, s) in backward_scales(rays, ref, ds, dc, g_rgb, g_depth, go_mag, g_ws).items()}


def fused_scales(rays, ref):
    out = forward_scales(ref, rays, None)
    out.update(backward_scales(rays, ref, ref["d_sigma"], ref["d_rgbs"], ref["g_rgb"], None, None, None))
    out["d_sigma"] = (ref["d_sigma"], ref["ds_scale"])
    out["sq_err"] = (ref["sq_err"], ref["sq_err"])
    return out


def fused_e32(rays, target, bg, loss_scale, n_rays):
    ref = fused64(rays, target, bg, loss_scale, n_rays)
    s32 = serial32_fused(rays, target, bg, loss_scale, n_rays, force_M=ref["M"])
    return {q: _e32(np.abs(s32[q].astype(np.float64) - v), s) for q, (v, s) in fused_scales(rays, ref).items()}


class Verdict:
    """What a judged result measured: ratios[quantity] = max |got - f64| / (E32 scale), failures = [text naming the ray]."""

    def __init__(self):
        self.ratios, self.failures = {}, []

    def ok(self):
        return not self.failures

    def __str__(self):
        return ", ".join("%s %.2f" % kv for kv in sorted(self.ratios.items()))


def _judge(v, rays, name, got, ref, scale, e32, k, extra=None):
    """|got - ref| <= k e32 scale + extra + TINY element-wise; records the worst ratio and names the worst offending ray."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    tol = k * e32 * scale + TINY + (0.0 if extra is None else extra)
    with np.errstate(invalid="ignore", divide="ignore"):
        over = err - (0.0 if extra is None else extra)
        ratio = np.where(scale > 0, np.maximum(over, 0.0) / (e32 * scale), 0.0) if e32 > 0 else np.zeros_like(err)
    v.ratios[name] = max(v.ratios.get(name, 0.0), float(np.max(ratio, initial=0.0)))
    bad = ~(err <= tol)                                     # (NaN in `got` fails)
    if bad.any():
        worst = np.unravel_index(np.argmax(np.where(bad, np.where(np.isnan(err), np.inf, err / tol), 0)), err.shape)
        v.failures.append("%s: ray %s element %s: |got - f64| = %.3g, allowed %.3g (E32 %.3g)"
                          % (name, rays.names[worst[0]], worst[1:], err[worst], tol[worst], e32))


def judge_counts(v, rays, got_M, what="live count"):
    """The count lies between count_bounds: exact on a decided ray.  Within one of the float64 model's on every ray but the plateau
    class (named plateau*), where a float32 evaluation may stop at any sample of the plateau."""
    got_M = np.asarray(got_M, np.int64)
    lo, hi = count_bounds(rays)
    M = forward64(rays)["M"]
    for i in np.flatnonzero((got_M < lo) | (got_M > hi)):
        v.failures.append("%s: ray %s has %d, the float64 model %d (admissible %d .. %d)" % (what, rays.names[i], got_M[i], M[i], lo[i], hi[i]))
    for i in np.flatnonzero(np.abs(got_M - M) > 1):
        if not rays.names[i].startswith("plateau"):
            v.failures.append("%s: ray %s has %d, more than one from the float64 model's %d" % (what, rays.names[i], got_M[i], M[i]))


def _judge_zeros(v, rays, name, got, M):
    """Exact +0 (no sentinel, no -0, no NaN) at every sample of the ray at or behind its live count."""
    got = np.asarray(got)
    behind = rays.valid & (np.arange(rays.L)[None, :] >= np.asarray(M)[:, None])
    if got.ndim == 3:
        behind = np.broadcast_to(behind[:, :, None], got.shape)
    bad = behind & ~((got == 0) & ~np.signbit(got))
    if bad.any():
        i = np.argwhere(bad)[0]
        v.failures.append("%s: ray %s sample %d behind the live count %d holds %r, not +0" % (name, rays.names[i[0]], i[1], M[i[0]], got[tuple(i)]))


def judge_forward(rays, got, e32, k=K, bg=None, v=None):
    """got: dict M, w [n, L], R, D, O (+ rgb_out when bg is given), as a float32 evaluation produced them."""
    v = Verdict() if v is None else v
    judge_counts(v, rays, got["M"])
    M = np.clip(np.asarray(got["M"], np.int64), 0, rays.N)
    ref = forward64(rays, force_M=M)
    _judge_zeros(v, rays, "w", got["w"], M)
    live = np.arange(rays.L)[None, :] < M[:, None]
    for q, (val, scale) in forward_scales(ref, rays, bg).items():
        g = np.where(live, got[q], 0.0) if q == "w" else got[q]
        _judge(v, rays, q, g, val, scale, e32[q], k)
    return v, ref


def judge_backward(rays, got_ds, got_dc, M, e32, g_rgb, g_depth=None, g_opacity=None, g_ws=None, bg=0.0, k=K, dc_half=False, v=None):
    """d_sigma / d_rgbs of a float32 evaluation whose forward found the live counts M (already judged)."""
    v = Verdict() if v is None else v
    M = np.clip(np.asarray(M, np.int64), 0, rays.N)
    ref = forward64(rays, force_M=M)
    go, go_mag = _go_parts(rays.n, g_rgb, g_opacity, bg)
    ds, dc, _ = backward64(rays, ref, g_rgb, g_depth, go, g_ws)
    _judge_values_backward(v, rays, got_ds, got_dc, M, ref, ds, dc, backward_scales(rays, ref, ds, dc, g_rgb, g_depth, go_mag, g_ws), e32, k, dc_half)
    return v


def _judge_values_backward(v, rays, got_ds, got_dc, M, ref, ds, dc, scales, e32, k, dc_half):
    _judge_zeros(v, rays, "d_sigma", got_ds, M)
    _judge_zeros(v, rays, "d_rgbs", got_dc, M)
    live = np.arange(rays.L)[None, :] < M[:, None]
    _judge(v, rays, "d_sigma", np.where(live, got_ds, 0.0), ds, scales["d_sigma"][1], e32["d_sigma"], k)
    # fp16 d_rgbs: one rounding of the float32 value on top (2^-11 relative, half the smallest subnormal 2^-25 absolute)
    extra = (2.0**-11 * (np.abs(dc) + k * e32["d_rgbs"] * scales["d_rgbs"][1]) + 2.0**-25) if dc_half else None
    _judge(v, rays, "d_rgbs", np.where(live[:, :, None], got_dc, 0.0), dc, scales["d_rgbs"][1], e32["d_rgbs"], k, extra)


def judge_fused(rays, got, target, bg, loss_scale, n_rays, e32, k=K, dc_half=False, v=None):
    """got: dict M, w, R, D, O, sq_err, d_sigma, d_rgbs of the fused kernel (or its emulation)."""
    v = Verdict() if v is None else v
    judge_counts(v, rays, got["M"])
    M = np.clip(np.asarray(got["M"], np.int64), 0, rays.N)
    ref = fused64(rays, target, bg, loss_scale, n_rays, force_M=M)
    _judge_zeros(v, rays, "w", got["w"], M)
    live = np.arange(rays.L)[None, :] < M[:, None]
    sc = fused_scales(rays, ref)
    for q in ("w", "R", "D", "O", "sq_err"):
        g = np.where(live, got[q], 0.0) if q == "w" else got[q]
        _judge(v, rays, q, g, sc[q][0], sc[q][1], e32[q], k)
    _judge_values_backward(v, rays, got["d_sigma"], got["d_rgbs"], M, ref, ref["d_sigma"], ref["d_rgbs"], sc, e32, k, dc_half)
    return v


# ------------------------------------------------------------------------------------------------------------------ the case table
def _track(rng, n):
    """Sample positions and step lengths that grow along the ray, as under exp_step_factor > 0."""
    t, dl = np.zeros(n), np.zeros(n)
    pos = 0.05 + 0.45 * rng.random()
    for j in range(n):
        dl[j] = pos / 256 + 1.7e-3
        t[j] = pos + 0.5 * dl[j]
        pos += dl[j]
    return t.astype(F), dl.astype(F)


def _ray(rng, name, n, sd):
    """A ray whose sample j has sigma_j delta_j ~ sd[j] (sigma is rounded to float32)."""
    t, dl = _track(rng, n)
    return (name, (np.asarray(sd, np.float64)[:n] / dl).astype(F), dl, t, rng.random((n, 3)).astype(F))


def _thin(rng, n):
    return 0.01 * (0.5 + rng.random(n))


def _lengths(rng):
    rays = []
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 300):
        rays.append(_ray(rng, "thin_N%d" % n, n, _thin(rng, n)))
        # medium: the optical depth -ln(thr) = 9.2 is reached after a fraction 0.3 .. 0.9 of the ray
        per = 9.21 / (max(n, 1) * (0.3 + 0.6 * rng.random()))
        rays.append(_ray(rng, "medium_N%d" % n, n, per * 2 * rng.random(n)))
    for n in (1, 64, 129):                                  # all-zero sigma: every sample live, w = 0, d_sigma != 0
        rays.append(_ray(rng, "zero_sigma_N%d" % n, n, np.zeros(n)))
    return rays


def _placed(rng, opaque, tag):
    rays = []
    for k in (1, 2, 63, 64, 65, 127, 128):
        for n in (k, k + 1, k + 70):
            sd = _thin(rng, n)
            sd[k - 1] = opaque                              # T falls below thr behind sample k - 1: exactly k live samples
            rays.append(_ray(rng, "%s_k%d_N%d" % (tag, k, n), n, sd))
    return rays


def _tuned(rng, name, n, j, plateau):
    """A ray whose float64 T_j is thr (1 +- few 1e-8): samples 0 .. j-2 carry an optical depth of -ln(thr) - 0.05, sample j-1 the rest.
    plateau: T_j = thr (1 + 1.2e-6) instead, j is lane 20 .. 40 of its 64-sample group, and the samples up to the group's end have sigma
    delta = 2^-24 (1 - a is one ulp below 1): T sinks through thr by 0.8 ulp per sample, while the Kogge-Stone products of the group's
    first factors differ from lane to lane by more than that.  The rest of the ray is dense."""
    _, _, dl, t, c = _ray(rng, name, n, np.ones(n))
    sd = (0.5 + rng.random(n)) * 0.05
    sd[:j - 1] *= (9.21 - 0.05) / sd[:j - 1].sum()
    if plateau:
        sd[j:-(-j // WAVE) * WAVE] = 2.0**-24
    sig = (sd / dl).astype(F)
    done = float(np.sum(sig[:j - 1].astype(np.float64) * dl[:j - 1].astype(np.float64)))
    off = -1.2e-6 if plateau else 3e-8 * rng.standard_normal()
    sig[j - 1] = F((-np.log(THR) - done + off) / float(dl[j - 1]))
    return (name, sig, dl, t, c)


def _hovering(rng, n_rays=300):
    """A random set (lengths 1 .. 299, termination anywhere or not at all) with the undecided class in it, 2 % of the rays: two rays
    that cross thr within a few 1e-8 and go on falling (a float32 evaluation may be one sample off), four PLATEAU rays (see
    count_bounds; the case liveness-as-a-prefix exists for: a Kogge-Stone product is not monotone to the last ulp there)."""
    rays = []
    special = {7: ("hover", 98, 162, False), 57: ("hover", 5, 39, False), 107: ("plateau", 20, 100, True), 157: ("plateau", 158, 260, True),
               207: ("plateau", 104, 200, True), 257: ("plateau", 217, 299, True)}
    for i in range(n_rays):
        n = int(rng.integers(1, 300))
        per = 9.21 / (n * (0.2 + 1.2 * rng.random()))
        ray = _ray(rng, "random%d_N%d" % (i, n), n, per * 2 * rng.random(n))
        if i in special:
            tag, j, n, plateau = special[i]
            ray = _tuned(rng, "%s%d_j%d_N%d" % (tag, i, j, n), n, j, plateau)
        rays.append(ray)
    return rays


def case_table():
    """name -> Rays.  Every ray is generated once from a fixed seed.  `counts` is the table the ray-count prefixes are taken from:
    its first rows mix every class so that the 4-ray blocks and the 16-ray LIVE blocks have full and ragged tails."""
    if _TABLE:
        return _TABLE
    lengths = _lengths(np.random.default_rng(101))
    placed = _placed(np.random.default_rng(102), 12.0, "placed")
    a_one = _placed(np.random.default_rng(103), 100.0, "a_one")
    hovering = _hovering(np.random.default_rng(104))
    rng = np.random.default_rng(105)
    pool = lengths + placed + a_one + hovering[:30] + hovering[107:108]
    counts = [pool[i] for i in rng.permutation(len(pool))[:67]]
    for name, lst in (("lengths", lengths), ("placed", placed), ("a_one", a_one), ("hovering", hovering), ("counts", counts)):
        _TABLE[name] = make_rays(lst)
    return _TABLE


_TABLE = {}
RAY_COUNTS = (1, 3, 4, 5, 15, 16, 17, 67)


def gradients(rays, seed):
    """Seeded upstream gradients for a set: g_rgb [n, 3], g_depth, g_opacity [n], g_ws [n, L] (float32)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rays.n, 3)).astype(F), rng.standard_normal(rays.n).astype(F), rng.standard_normal(rays.n).astype(F),
            rng.standard_normal((rays.n, rays.L)).astype(F))


def targets(rays, bg, seed):
    """Target colours at 0.1 .. 0.6 from the float64 blended colour, either side, per channel: the MSE residual is then known to a
    relative 2^-24 / 0.1 in float32 and |g_rgb| T_s is a meaningful scale for d_rgbs (a residual that cancels to nothing has no
    float32 digits at all, in any order)."""
    rng = np.random.default_rng(seed)
    ref = forward64(rays)
    blended = ref["R"] + bg * (1 - ref["O"])[:, None]
    off = (0.1 + 0.5 * rng.random((rays.n, 3))) * np.where(rng.random((rays.n, 3)) < 0.5, -1.0, 1.0)
    return (blended + off).astype(F)


# ------------------------------------------------------------------------------------------------------------------ the buffer layout
class Layout:
    """Sample buffers and rays_a for a Rays batch the way the kernels see them: row r of rays_a is ray r of `rays` with ray index
    ray_idx[r] (a permutation sample of range(n_out), n_out > n: some output rows belong to no ray), sample ranges allocated in yet
    another order with 0-5 unused samples between them, 64 spare rows at the end.  Unused samples hold finite junk."""

    def __init__(self, rays, seed, half=False):
        rng = np.random.default_rng(seed)
        n = rays.n
        self.rays, self.n, self.n_out = rays, n, n + 5
        self.ray_idx = rng.permutation(self.n_out)[:n].astype(np.int32)
        start, pos = np.zeros(n, np.int32), 0
        for r in rng.permutation(n):
            pos += int(rng.integers(0, 6))
            start[r] = pos
            pos += int(rays.N[r])
        self.S = pos + 64
        self.rays_a = np.stack([self.ray_idx, start, rays.N.astype(np.int32)], 1).astype(np.int32)
        self.start = start
        self.sigmas, self.deltas, self.ts = np.full(self.S, 3.0, F), np.full(self.S, 0.01, F), np.ones(self.S, F)
        self.rgbs = np.full((self.S, 3), 0.5, np.float16 if half else F)
        for r in range(n):
            sl, m = slice(start[r], start[r] + rays.N[r]), rays.N[r]
            self.sigmas[sl], self.deltas[sl], self.ts[sl], self.rgbs[sl] = rays.sigma[r, :m], rays.delta[r, :m], rays.t[r, :m], rays.rgb[r, :m]

    def flat(self, padded, fill=0.0):
        """[n, L, ...] -> [S, ...] (per-sample input such as g_ws)."""
        out = np.full((self.S,) + padded.shape[2:], fill, padded.dtype)
        for r in range(self.n):
            out[self.start[r]:self.start[r] + self.rays.N[r]] = padded[r, :self.rays.N[r]]
        return out

    def per_ray(self, rows_values, fill=0.0):
        """[n, ...] in row order -> [n_out, ...] indexed by ray index."""
        out = np.full((self.n_out,) + rows_values.shape[1:], fill, rows_values.dtype)
        out[self.ray_idx] = rows_values
        return out

    def padded(self, flat, m=None):
        """[S, ...] kernel output -> [m, L, ...] in row order (0 outside the rays)."""
        m = self.n if m is None else m
        out = np.zeros((m, self.rays.L) + flat.shape[1:], flat.dtype)
        for r in range(m):
            out[r, :self.rays.N[r]] = flat[self.start[r]:self.start[r] + self.rays.N[r]]
        return out

    def sample_mask(self, m=None):
        """[S] bool: samples that belong to one of the first m rays."""
        mask = np.zeros(self.S, bool)
        for r in range(self.n if m is None else m):
            mask[self.start[r]:self.start[r] + self.rays.N[r]] = True
        return mask

    def ray_mask(self, m=None):
        mask = np.zeros(self.n_out, bool)
        mask[self.ray_idx[:self.n if m is None else m]] = True
        return mask
