"""Float64 reference of the training step's epilogue (include/ngp_hip.h f-2: the scalar bookkeeping of GradScaler.step / update and
CosineAnnealingLR, Adam(eps) with its 16-bit storage copies, the MSE loss and its gradient, the slab sum of the MLP weight gradient)
-- the CPU side of tests/test_optim_reference.py and tests/test_gpu_optim_exact.py.  numpy only.

Three layers, as for compositing, the MLP and the scatter-add: a float64 contract (prologue64, amp_prologue64, adam64, mse64,
dw_reduce64), a float32 restatement with every rounding a separate numpy float32 operation (adam32, mse32, bf16_rne, f16_rne), and
the kernels held to both: bit for bit to the float32 form (the library is built with -ffp-contract=off and without fast-math;
float32 divide and square root are correctly rounded), within the bounds below to the float64 form.

Hyperparameters (lr0, eta_min, beta1, beta2, eps, growth, backoff, lr) are THE FLOAT32 VALUES THAT CROSS THE C ABI, widened: every
function here rounds them to float32 first (hyper()).  torch.optim.Adam with Python-double betas is a slightly different
optimizer; test_optim_reference.py records the distance.

State layout (include/ngp_hip.h): sf = [loss scale, 1/scale of this step, lr, 1 - beta1^t, sqrt(1 - beta2^t), last loss, -, -],
si = [iteration, optimizer steps taken, growth tracker, found_inf, skip flag of this step, skipped steps so far, -, -].

Scalar contract (one step).
    skip       = found_inf != 0, and found_inf is consumed (cleared)
    inv_scale  = 1 / scale, the scale BEFORE growth or backoff (GradScaler.unscale_ runs before GradScaler.update)
    lr         = eta_min + (lr0 - eta_min)(1 + cos(pi min(iter, t_max) / t_max)) / 2   from the iteration counter BEFORE it advances;
                 the schedule advances on skipped steps too (scheduler.step() is unconditional) and stays at eta_min from t_max on
    not skipped: opt_step += 1, bc1 = 1 - beta1^opt_step, bc2_sqrt = sqrt(1 - beta2^opt_step); growth tracker += 1 and, when it
                 reaches growth_interval, scale *= growth and the tracker returns to 0
    skipped:     scale *= backoff, tracker = 0, skipped_total += 1; opt_step and the bias corrections keep their values
    AMP form (amp_prologue64): lr, the scale and the flag come from outside (None: scale 1 / never skip); it touches neither the
                 loss scale, the iteration nor the growth tracker.

Adam contract (adam64), per element, torch.optim.Adam's algebra:
    gr = g inv_scale;  m' = beta1 m + (1 - beta1) gr;  v' = beta2 v + (1 - beta2) gr^2
    p' = p - (lr / bc1) m' / (sqrt(v') / bc2_sqrt + eps)
and the step's outcome (adam_step32): g is zero afterwards; a skipped step leaves p, m, v and the storage copy bitwise untouched
and still clears g; the copy is bf16_rne(p') / f16_rne(p') wherever it is written, and the caller keeps copy == round(p) elsewhere;
g = m = v = 0 is an exact fixed point; an f16 gradient is widened exactly.

adam32, the float32 order (u = 2^-24, fl = one float32 rounding):
    gr = fl(g inv);  d = fl(gr - m);  c1 = fl(1 - beta1);  m' = fl(m + fl(d c1))
    c2 = fl(1 - beta2);  v' = fl(fl(v beta2) + fl(fl(gr gr) c2))
    den = fl(fl(sqrt(v') / bc2_sqrt) + eps)   (sqrt one rounding of its own);  step = fl(lr / bc1);  p' = fl(p - fl(step fl(m' / den)))

Bounds of adam32 against adam64 on the SAME constants (adam_bounds; first order in u, times 1 + 2^-10 for the higher orders;
valid while every intermediate is a normal float32 -- the `denormal` set adds an absolute floor of 8 * 2^-149 to each of Bm, Bv, Bdp
instead: at most 5 roundings of at most 2^-150 each; the floor on v' reaches dp through the root, |dp| floor / v', and v' is kept normal):
    m':  5 roundings (gr, gr - m, 1 - beta1, the product, the sum).  The error of gr enters d absolutely, so the cancellation in
         gr - m does not help:   |m'32 - m'64| <= u (c1 |gr| + 3 c1 |gr - m| + |m'|)                                  =: Bm
    v':  gr^2 carries 3 (gr twice, the square), 1 - beta2 and the product one each, v beta2 one, the sum one; all terms are >= 0:
         |v'32 - v'64| <= u (5 c2 gr^2 + beta2 v + v')  <=  6 u v'                                                      =: Bv
    dp = p - p' before the last subtraction:  v' is off by at most 6 u relatively, its root by 3 u, plus the root's own rounding
         (1), the divide by bc2_sqrt (1), the add of eps (1): den within 6 u; the quotient m' / den (1), lr / bc1 (1), the product (1):
         |dp32 - dp64| <= (lr / bc1) Bm / den + 9 u |dp|                                                                =: Bdp
    p':  |p'32 - p'64| <= Bdp + u |p'|
When the float64 side is driven by prologue64 instead of the device's own state, lr, bc1 and bc2_sqrt differ by the scalar
bounds below; dp is homogeneous of degree 1 in lr, -1 in bc1 and at most 1 in bc2_sqrt, so Bdp grows by |dp| (e_lr / lr + e_bc1 / bc1
+ e_bc2 / bc2_sqrt) (adam_bounds(rel_consts=...)); m' and v' do not depend on them.

Scalar bounds.  powf and cosf on the device are not correctly rounded; POW_ULPS and COS_ULPS are the only measured numbers in
this file (profiles/PARITY_NOTES.md: twice the measured maximum, never below 1).
    1 - beta^t:  pow < 1, so its ulp is at most 2^-24: |pow32 - pow| <= POW_ULPS u; the subtraction rounds a result < 1: u / 2.
         |bc1_32 - bc1| <= (POW_ULPS + 1) u  ABSOLUTELY (bc_abs_bound).  At t = 1, 1 - beta2^t is 1e-3: RELATIVELY that allows 1.7e-4
         (about 1e-5 is what a well-rounded pow leaves) -- a consequence of forming 1 - beta^t in float32, not a tolerance chosen here.
    sqrt(1 - beta2^t) = sqrt(y):  |sqrt(y32) - sqrt(y)| <= e_y / (2 sqrt(y - e_y)), plus the root's rounding u / 2 (result < 1)
         (bc2_sqrt_abs_bound).
    lr:  x = fl(fl(pi32 k) / T) is within 3 u of pi k / T relatively (pi32, product, quotient), so cos moves by at most 3 pi u k / T;
         cosf adds COS_ULPS u (|cos| <= 1: ulp <= 2^-24 below 1).  With A = (lr0 - eta_min) / 2 and w = 1 + cos:
         |lr32 - lr| <= A (3 pi k / T + COS_ULPS) u + u (3 A w + lr)   (the add 1 + c, lr0 - eta_min, the product, the final add)
         (lr_abs_bound).  In float64 lr at iter >= t_max is exactly eta_min: cos(pi) is exactly -1.

Sums.  The reduced loss and the slab sum use the project's usual bound for a float32 sum of n terms in any order,
(n + 16) u sum|terms| (sum_bound) -- 16 stands for the fixed number of extra roundings around the sum (the divide by 3 n, the add
onto dW).  For the loss the terms themselves are float32 squares of float32 differences: diff32 = fl(fl(rgb + b) - target) with
b = fl(bg fl(1 - opacity)) is within e = u (2 |b| + |rgb + b| + |diff|) of the float64 difference, so a term is within
e (2 |diff| + e) + u diff^2 of its float64 value (mse_loss_bound); that matters where rgb + b - target cancels.

`alter=` switches on ONE deliberate defect (ALTERS); test_optim_reference.py shows that each one fails the assertion below that
tests/test_gpu_optim_exact.py applies to the kernels."""
import math

import numpy as np

f16, f32, f64, u16, u32 = np.float16, np.float32, np.float64, np.uint16, np.uint32
U = 2.0**-24
SLACK = 1.0 + 2.0**-10
TINY = 2.0**-149
DENORMAL_FLOOR = 8 * TINY                   # up to 5 roundings of at most 2^-150 each in m' / v' where intermediates leave the normal range
# measured on gfx950 (profiles/PARITY_NOTES.md, "Training-step epilogue"): powf(beta, t) for beta = 0.9f, 0.999f and t = 1 .. 64 is off by at
# most 0.92 ulp, cosf(pi32 k / T) for T = 8, 24, 40 and k = 0 .. T by at most 0.88 x 2^-24; the allowance is twice that
POW_ULPS = 1.84
COS_ULPS = 1.76
NW = 9408                                   # flat MLP weights W1 | W2 | W3 | W4 | W5

SF_SCALE, SF_INV, SF_LR, SF_BC1, SF_BC2S, SF_LOSS = range(6)
SI_ITER, SI_OPT, SI_GROWTH, SI_FOUND, SI_SKIP, SI_SKIPPED = range(6)

ALTERS = ("bc2_for_bc2_sqrt", "eps_before_divide", "lr_at_iter_plus_1", "growth_not_reset_on_skip", "opt_step_on_skip",
          "inv_scale_after_growth", "bf16_truncated", "grad_not_cleared", "copy_on_skip")


def hyper(x):
    """The value a `float` argument of the C ABI has, widened to float64."""
    return float(f32(x))


# ------------------------------------------------------------------------------------------------ scalar state machine
def cosine_lr64(lr0, eta_min, t_max, it):
    lr0, eta_min = hyper(lr0), hyper(eta_min)
    return eta_min + (lr0 - eta_min) * (1.0 + math.cos(math.pi * min(it, t_max) / t_max)) / 2.0


def prologue64(sf, si, lr0, eta_min, t_max, beta1, beta2, growth, backoff, growth_interval, alter=None):
    """One step of ngp_train_prologue's contract: (sf', si') as lists of Python floats (float64) and ints."""
    beta1, beta2, growth, backoff = hyper(beta1), hyper(beta2), hyper(growth), hyper(backoff)
    sf, si = [float(x) for x in sf], [int(x) for x in si]
    it, scale, skip = si[SI_ITER], sf[SF_SCALE], si[SI_FOUND] != 0
    new_scale, tracker = scale, si[SI_GROWTH]
    if skip:
        new_scale = scale * backoff
        tracker = tracker if alter == "growth_not_reset_on_skip" else 0
        si[SI_SKIPPED] += 1
    else:
        tracker += 1
        if tracker >= growth_interval:
            new_scale, tracker = scale * growth, 0
    if not skip or alter == "opt_step_on_skip":
        si[SI_OPT] += 1
        sf[SF_BC1] = 1.0 - beta1 ** si[SI_OPT]
        sf[SF_BC2S] = math.sqrt(1.0 - beta2 ** si[SI_OPT])
    sf[SF_INV] = 1.0 / (new_scale if alter == "inv_scale_after_growth" else scale)
    sf[SF_LR] = cosine_lr64(lr0, eta_min, t_max, it + 1 if alter == "lr_at_iter_plus_1" else it)
    sf[SF_SCALE] = new_scale
    si[SI_GROWTH], si[SI_FOUND], si[SI_SKIP], si[SI_ITER] = tracker, 0, int(skip), it + 1
    return sf, si


def amp_prologue64(sf, si, grad_scale, found_inf, lr, beta1, beta2, alter=None):
    """ngp_adam_amp_prologue's contract: grad_scale / found_inf are the scaler's values or None (scale 1 / never skip)."""
    beta1, beta2 = hyper(beta1), hyper(beta2)
    sf, si = [float(x) for x in sf], [int(x) for x in si]
    skip = found_inf is not None and float(found_inf) != 0.0
    sf[SF_INV] = 1.0 / float(grad_scale) if grad_scale is not None else 1.0
    sf[SF_LR] = hyper(lr)
    si[SI_SKIP] = int(skip)
    if skip:
        si[SI_SKIPPED] += 1
    if not skip or alter == "opt_step_on_skip":
        si[SI_OPT] += 1
        sf[SF_BC1] = 1.0 - beta1 ** si[SI_OPT]
        sf[SF_BC2S] = math.sqrt(1.0 - beta2 ** si[SI_OPT])
    return sf, si


def bc_abs_bound(pow_ulps=None):
    return ((POW_ULPS if pow_ulps is None else pow_ulps) + 1.0) * U


def bc2_sqrt_abs_bound(beta2, t, pow_ulps=None):
    y = 1.0 - hyper(beta2) ** t
    e = bc_abs_bound(pow_ulps)
    return e / (2.0 * math.sqrt(y - e)) + U / 2


def lr_abs_bound(lr0, eta_min, t_max, it, cos_ulps=None):
    lr0, eta_min, k = hyper(lr0), hyper(eta_min), min(it, t_max)
    A = abs(lr0 - eta_min) / 2.0
    w = 1.0 + math.cos(math.pi * k / t_max)
    cu = COS_ULPS if cos_ulps is None else cos_ulps
    return (A * (3.0 * math.pi * k / t_max + cu) * U + U * (3.0 * A * w + abs(cosine_lr64(lr0, eta_min, t_max, it)))) * SLACK


def scalar_bounds(sf64, si64, lr0, eta_min, t_max, beta2, it):
    """Absolute bounds on the device's (lr, bc1, bc2_sqrt) after the step that left (sf64, si64); it = the iteration it ran at.
    lr0 None: the AMP form, lr is handed over and exact."""
    t = si64[SI_OPT]
    e_lr = 0.0 if lr0 is None else lr_abs_bound(lr0, eta_min, t_max, it)
    if t == 0:
        return e_lr, 0.0, 0.0                       # no step taken yet: the corrections still hold their initial value
    return e_lr, bc_abs_bound(), bc2_sqrt_abs_bound(beta2, t)


def assert_scalar_state(got_sf, got_si, want_sf, want_si, e_lr, e_bc1, e_bc2s, what=""):
    """The comparison the GPU test makes after every prologue launch: integers, the loss scale and 1/scale exact, lr and the bias
    corrections within the scalar bounds of float64."""
    got_i, want_i = [int(x) for x in got_si[:6]], [int(x) for x in want_si[:6]]
    assert got_i == want_i, "%s state_i %s != %s (iter, opt_step, growth, found_inf, skip, skipped_total)" % (what, got_i, want_i)
    assert float(got_sf[SF_SCALE]) == want_sf[SF_SCALE], "%s loss scale %r != %r" % (what, float(got_sf[SF_SCALE]), want_sf[SF_SCALE])
    assert float(got_sf[SF_INV]) == want_sf[SF_INV], "%s inv_scale %r != %r" % (what, float(got_sf[SF_INV]), want_sf[SF_INV])
    for k, e, name in ((SF_LR, e_lr, "lr"), (SF_BC1, e_bc1, "bc1"), (SF_BC2S, e_bc2s, "bc2_sqrt")):
        err = abs(float(got_sf[k]) - want_sf[k])
        assert err <= e, "%s %s %r vs %r: error %.3g > bound %.3g" % (what, name, float(got_sf[k]), want_sf[k], err, e)


# ------------------------------------------------------------------------------------------------ 16-bit storage formats
def bf16_rne(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even; overflow rounds to inf; NaN stays NaN (quiet bit set)."""
    b = np.ascontiguousarray(x, dtype=f32).view(u32).astype(np.uint64)
    r = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    nan = (b & 0x7fffffff) > 0x7f800000
    return np.where(nan, (b >> 16) | 0x40, r).astype(u16)


def bf16_trunc(x):
    return (np.ascontiguousarray(x, dtype=f32).view(u32) >> 16).astype(u16)


def f16_rne(x):
    """float32 -> IEEE binary16 bit patterns (uint16), round to nearest even, from the bits: normal numbers by rounding the 13
    dropped mantissa bits (the carry runs into the exponent, 65520 and above reach inf), subnormals as multiples of 2^-24."""
    x = np.ascontiguousarray(x, dtype=f32)
    b = x.view(u32).astype(np.int64)
    sign, a = (b >> 16) & 0x8000, b & 0x7fffffff
    r = a - (112 << 23)                                                     # exponent bias 127 -> 15
    normal = np.minimum((r + 0xfff + ((r >> 13) & 1)) >> 13, 0x7c00)
    small = a < 0x38800000                                                  # below 2^-14
    sub = np.rint(np.where(small, np.abs(x), 0).astype(f64) * 2.0**24).astype(np.int64)       # exact product; rint rounds half to even
    out = np.where(small, sub, normal)
    out = np.where(a > 0x7f800000, 0x7e00 | ((a >> 13) & 0x3ff), out)
    return (sign | out).astype(u16)


def is_nan16(bits, kind):
    bits = np.asarray(bits).astype(np.int64) & 0x7fff
    return bits > (0x7f80 if kind == 1 else 0x7c00)


def round16(x, kind, alter=None):
    if kind == 1:
        return bf16_trunc(x) if alter == "bf16_truncated" else bf16_rne(x)
    return f16_rne(x)


# ------------------------------------------------------------------------------------------------ Adam
def consts64(inv_scale, lr, bc1, bc2_sqrt, beta1, beta2, eps):
    return dict(inv_scale=float(inv_scale), lr=float(lr), bc1=float(bc1), bc2_sqrt=float(bc2_sqrt), beta1=hyper(beta1),
                beta2=hyper(beta2), eps=hyper(eps))


def consts_from_state(sf, beta1, beta2, eps):
    """Adam's constants from a state vector: the device's float32 one (bit-exact tests) or prologue64's."""
    return consts64(sf[SF_INV], sf[SF_LR], sf[SF_BC1], sf[SF_BC2S], beta1, beta2, eps)


def adam64(p, g, m, v, c, alter=None):
    p, g, m, v = (np.asarray(a).astype(f64) for a in (p, g, m, v))
    gr = g * c["inv_scale"]
    m1 = c["beta1"] * m + (1.0 - c["beta1"]) * gr
    v1 = c["beta2"] * v + (1.0 - c["beta2"]) * gr * gr
    b2 = c["bc2_sqrt"] ** 2 if alter == "bc2_for_bc2_sqrt" else c["bc2_sqrt"]
    den = (np.sqrt(v1) + c["eps"]) / b2 if alter == "eps_before_divide" else np.sqrt(v1) / b2 + c["eps"]
    dp = (c["lr"] / c["bc1"]) * m1 / den
    return p - dp, m1, v1, dp


def adam32(p, g, m, v, c, alter=None):
    """Float32 restatement; c holds float32-representable constants (consts_from_state of a float32 state).  Returns p', m', v' and the update dp (p' = fl(p - dp))."""
    p, g, m, v = (np.asarray(a, dtype=f32) for a in (p, g, m, v))
    k = {n: f32(x) for n, x in c.items()}
    one = f32(1.0)
    with np.errstate(all="ignore"):
        gr = g * k["inv_scale"]
        m1 = m + (gr - m) * (one - k["beta1"])
        v1 = v * k["beta2"] + (gr * gr) * (one - k["beta2"])
        b2 = k["bc2_sqrt"] * k["bc2_sqrt"] if alter == "bc2_for_bc2_sqrt" else k["bc2_sqrt"]
        den = (np.sqrt(v1) + k["eps"]) / b2 if alter == "eps_before_divide" else np.sqrt(v1) / b2 + k["eps"]
        dp = (k["lr"] / k["bc1"]) * (m1 / den)
        p1 = p - dp
    for a in (gr, m1, v1, den, dp, p1):
        assert a.dtype == f32
    return p1, m1, v1, dp


def adam_bounds(p, g, m, v, c, rel_consts=0.0, floor=0.0):
    """(Bp, Bm, Bv, Bdp): the docstring's bounds of adam32 against adam64(p, g, m, v, c).  rel_consts: the summed relative
    uncertainty of lr, bc1 and bc2_sqrt when c is not the device's own state; floor: absolute allowance per quantity where
    intermediates are denormal."""
    p1, m1, v1, dp = adam64(p, g, m, v, c)
    m, v = np.asarray(m).astype(f64), np.asarray(v).astype(f64)
    gr = np.asarray(g).astype(f64) * c["inv_scale"]
    c1, c2 = 1.0 - c["beta1"], 1.0 - c["beta2"]
    Bm = U * (c1 * np.abs(gr) + 3 * c1 * np.abs(gr - m) + np.abs(m1)) * SLACK + floor
    Bv = U * (5 * c2 * gr * gr + c["beta2"] * v + v1) * SLACK + floor
    den = np.sqrt(v1) / c["bc2_sqrt"] + c["eps"]
    Bdp = ((c["lr"] / c["bc1"]) * Bm / den + (9 * U + rel_consts) * np.abs(dp)) * SLACK + floor
    if floor:
        Bdp = Bdp + np.abs(dp) * floor / np.maximum(v1, TINY)               # the floor on v' reaches dp through the root: <= floor / v' relatively
    Bp = Bdp + U * np.abs(p1) * SLACK
    return Bp, Bm, Bv, Bdp


def trajectory_error_step(s32, s64, c_dev, c64, err, e_g, rel_consts):
    """Accumulated bound of a float32 trajectory against the float64 one over ONE more step.  s32 / s64: dict(p, g, m, v) of
    either trajectory before the step; err: dict(p, m, v) bounds on their distance; e_g: bound on |g32 - g64|; c_dev the float32
    trajectory's constants, c64 the float64 one's, rel_consts their summed relative distance.  Three legs:
      adam32(s32, c_dev) to adam64(s32, c64):  adam_bounds(s32, c_dev, rel_consts)
      adam64(s32, c64) to adam64(s64, c64), with I = inv_scale, c1 = 1 - beta1, c2 = 1 - beta2:
        m':  beta1 e_m + c1 I e_g                                    (linear)
        v':  beta2 e_v + c2 I^2 e_g (2 |g64| + e_g)                  (|a^2 - b^2| <= e (2 |b| + e))
        dp:  with rho = e_v' / v'64 < 1 the root moves by at most r = rho / (1 + sqrt(1 - rho)) relatively (eps only lessens that):
             |dp - dp64| <= (lr / bc1) (e_m' + |m'64| r) / (den64 (1 - r))
        p':  e_p + the bound on dp."""
    Bp, Bm, Bv, Bdp = adam_bounds(s32["p"], s32["g"], s32["m"], s32["v"], c_dev, rel_consts)
    p1, m1, v1, dp = adam64(s64["p"], s64["g"], s64["m"], s64["v"], c64)
    I, c1, c2 = c64["inv_scale"], 1.0 - c64["beta1"], 1.0 - c64["beta2"]
    e_m = c64["beta1"] * err["m"] + c1 * I * e_g
    e_v = c64["beta2"] * err["v"] + c2 * I * I * e_g * (2 * np.abs(np.asarray(s64["g"]).astype(f64)) + e_g)
    rho = e_v / v1
    assert (rho < 0.5).all(), "trajectory_error_step: v' is not known well enough (max rho %.3g)" % float(rho.max())
    r = rho / (1.0 + np.sqrt(1.0 - rho))
    den = np.sqrt(v1) / c64["bc2_sqrt"] + c64["eps"]
    e_dp = (c64["lr"] / c64["bc1"]) * (e_m + np.abs(m1) * r) / (den * (1.0 - r))
    return dict(p=err["p"] + e_dp + Bdp + U * np.abs(p1) * SLACK, m=e_m + Bm, v=e_v + Bv)


def adam_step32(p, g, m, v, c, skip=False, copy=None, copy_kind=0, alter=None):
    """The whole step's outcome in float32: dict(p, m, v, g, copy).  g may be float16 (widened exactly); copy is the uint16 storage
    copy as it stood before the step (copy_kind 1 bf16, 2 f16)."""
    g = np.asarray(g)
    g_out = g.copy() if alter == "grad_not_cleared" else np.zeros_like(g)
    p, m, v = (np.asarray(a, dtype=f32) for a in (p, m, v))
    if skip:
        out = dict(p=p.copy(), m=m.copy(), v=v.copy(), g=g_out, copy=None if copy is None else np.asarray(copy, dtype=u16).copy())
        if alter == "copy_on_skip" and copy_kind:
            out["copy"] = round16(p, copy_kind)
        return out
    p1, m1, v1, _ = adam32(p, g.astype(f32), m, v, c, alter)
    return dict(p=p1, m=m1, v=v1, g=g_out, copy=round16(p1, copy_kind, alter) if copy_kind else None)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: u16, 4: u32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d: got %r, want %r" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def assert_step_exact(got, want, what=""):
    """got / want: dicts as adam_step32 returns.  p, m, v and the storage copy bit for bit; g numerically zero (a -0.0 that was
    never rewritten is a zero)."""
    for k in ("p", "m", "v"):
        assert_bits_equal(got[k], want[k], "%s %s'" % (what, k))
    nz = np.flatnonzero(np.asarray(got["g"]).astype(f32) != 0)
    assert nz.size == 0, "%s gradient not cleared at %d of %d elements, first %d" % (what, nz.size, np.asarray(got["g"]).size, nz[0])
    if want.get("copy") is not None:
        assert_bits_equal(got["copy"], want["copy"], "%s storage copy" % what)


def assert_step_within(got, before, c, what="", rel_consts=0.0, floor=0.0):
    """got: the step's p, m, v; before: dict(p, g, m, v) as they stood; c: float64 constants.  dp, m', v' within adam_bounds."""
    p1, m1, v1, dp = adam64(before["p"], before["g"], before["m"], before["v"], c)
    Bp, Bm, Bv, Bdp = adam_bounds(before["p"], before["g"], before["m"], before["v"], c, rel_consts, floor)
    worst = {}
    for name, a, ref, B in (("m'", got["m"], m1, Bm), ("v'", got["v"], v1, Bv), ("p'", got["p"], p1, Bp)):
        err = np.abs(np.asarray(a).astype(f64) - ref)
        bad = np.flatnonzero(~(err <= B))
        assert bad.size == 0, "%s %s: %d elements outside the bound, first %d: got %r, float64 %r, bound %.3g" % (
            what, name, bad.size, bad[0], np.asarray(a).ravel()[bad[0]], ref[bad[0]], B[bad[0]])
        worst[name] = float(np.max(err / np.maximum(B, TINY)))
    return worst


# ------------------------------------------------------------------------------------------------ MSE loss and its gradient
def mse64(rgb, opacity, target, bg, n, scale):
    """(loss, sq_err [n], g_rgb [n, 3], g_opacity [n]): loss = mean((rgb + bg (1 - opacity) - target)^2) over 3 n values, the
    gradients of scale * loss with respect to rgb and opacity."""
    rgb, target = np.asarray(rgb).astype(f64).reshape(n, 3), np.asarray(target).astype(f64).reshape(n, 3)
    op, bg = np.asarray(opacity).astype(f64).reshape(n), hyper(bg)
    diff = rgb + (bg * (1.0 - op))[:, None] - target
    g_rgb = 2.0 / (3.0 * n) * float(scale) * diff
    return float(np.sum(diff * diff) / (3.0 * n)), np.sum(diff * diff, axis=1), g_rgb, -bg * np.sum(g_rgb, axis=1)


def mse32(rgb, opacity, target, bg, n, scale):
    """(sq_err, g_rgb, g_opacity) in the kernels' float32 association: k = 2 / (3 n) * scale left to right, go -= bg * gr over
    c = 0, 1, 2 starting from -0.0 (so a zero result carries the sign of -bg * gr: with bg = 0 g_opacity may be -0.0), sq_err += diff^2
    in the same order from +0.0.  (The reduced loss has no fixed order: mse_loss_bound.)"""
    rgb, target = np.asarray(rgb, dtype=f32).reshape(n, 3), np.asarray(target, dtype=f32).reshape(n, 3)
    op, bg, one = np.asarray(opacity, dtype=f32).reshape(n), f32(bg), f32(1.0)
    k = f32(2.0) / (f32(3.0) * f32(n)) * f32(scale)
    b = bg * (one - op)
    go, se = np.full(n, -0.0, f32), np.zeros(n, f32)                        # -0.0 - x is -x exactly, zeros included: go = -bg sum(gr)
    g_rgb = np.empty((n, 3), f32)
    for c in range(3):
        diff = (rgb[:, c] + b) - target[:, c]
        se = se + diff * diff
        g_rgb[:, c] = k * diff
        go = go - bg * g_rgb[:, c]
    assert k.dtype == f32 and go.dtype == f32 and se.dtype == f32
    return se, g_rgb, go


def sum_bound(n_terms, abs_sum, const=16):
    return (n_terms + const) * U * abs_sum


def mse_loss_bound(rgb, opacity, target, bg, n):
    rgb, target = np.asarray(rgb).astype(f64).reshape(n, 3), np.asarray(target).astype(f64).reshape(n, 3)
    b = (hyper(bg) * (1.0 - np.asarray(opacity).astype(f64).reshape(n)))[:, None]
    diff = np.abs(rgb + b - target)
    e = U * (2 * np.abs(b) + np.abs(rgb + b) + diff) * SLACK
    terms = float(np.sum(diff * diff))
    forming = float(np.sum(e * (2 * diff + e) + U * diff * diff))
    return (sum_bound(3 * n, terms + forming) + forming) / (3.0 * n)


# ------------------------------------------------------------------------------------------------ slab sum
def dw_reduce64(parts, n_parts):
    """(sum, sum |part|) over the first n_parts slabs of parts [>= n_parts, NW]."""
    a = np.asarray(parts).astype(f64).reshape(-1, NW)[:n_parts]
    return a.sum(axis=0), np.abs(a).sum(axis=0)


def dw_bound(n_parts, dW0, abs_sum):
    return sum_bound(n_parts, np.abs(np.asarray(dW0).astype(f64)) + abs_sum)


# ------------------------------------------------------------------------------------------------ named input sets
SETS = ("typical", "first_step", "fixed_point", "cancel", "tiny_v", "huge", "neg_zero", "f16_edges", "bf16_ties", "denormal")
EXACT_SETS = tuple(s for s in SETS if s != "denormal")          # every intermediate normal (or exactly zero): bit-exact
SCALE = 2.0**15                                                  # loss scale of the sets: g holds SCALE x the gradient
F16_EDGE_VALUES = (65504.0, 65519.0, 65520.0, 65521.0, 65536.0, 1e5, 2.0**-14, 2.0**-14 * (1 - 2.0**-11), 2.0**-14 * (1 - 2.0**-12),
                   2.0**-24, 2.0**-25, 2.0**-25 * (1 + 2.0**-20), 3 * 2.0**-25, 2.0**-26, 1 + 2.0**-11, 1 + 3 * 2.0**-11,
                   1 + 2.0**-11 + 2.0**-23, 1 + 2.0**-11 - 2.0**-23, 2047 * 2.0**-24 + 2.0**-25)
BF16_EDGE_BITS = (0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x3f80ffff, 0x3fff8000, 0x3fffffff, 0x7f7f8000, 0x7f7f7fff,
                  0x00008000, 0x00018000, 0x00007fff, 0x007f8000, 0x00800000)


def input_set(name, n=4096, seed=0):
    """dict(p, g, m, v: float32 [n], eps: the eps values the set is meant for).  n % 4 == 0.  Deterministic in (name, n, seed)."""
    assert n % 4 == 0 and name in SETS
    rng = np.random.default_rng([SETS.index(name), n, seed])
    sgn = lambda: rng.choice([-1.0, 1.0], n)
    p = sgn() * 10.0 ** rng.uniform(-4, 0, n)
    gr = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -2, n)
    m = rng.standard_normal(n) * 1e-3
    v = rng.uniform(0, 1, n) * 1e-5 + 1e-9
    eps = (1e-15,)
    lane, grp = np.arange(n) % 4, np.arange(n) // 4
    if name == "typical":
        gr[grp % 4 == 1] = 0.0                                              # groups that received no gradient this step
    elif name == "first_step":
        m[:] = 0.0; v[:] = 0.0
    elif name == "fixed_point":
        whole = grp % 3 == 0                                                # whole float4 groups ...
        single = (grp % 3 == 1) & (lane == grp % 4)                         # ... and single lanes of a group
        for a in (gr, m, v):
            a[whole | single] = 0.0
    elif name == "cancel":
        m = rng.standard_normal(n) * 10.0 ** rng.uniform(-5, -1, n)
        gr = f32(m).astype(f64) * (1.0 + rng.integers(-8, 9, n) * 2.0**-22)
    elif name == "tiny_v":
        eps = (1e-15, 1e-8)
        e = np.where(grp % 2 == 0, 1e-8, 1e-15)                             # sqrt(v') / bc2_sqrt comparable with either eps
        gr = sgn() * e * 10.0 ** rng.uniform(-1.5, 1.5, n)
        m = rng.standard_normal(n) * e
        v = (e * 10.0 ** rng.uniform(-1.5, 1.5, n)) ** 2
    elif name == "huge":
        gr = sgn() * 1e18 * rng.uniform(0.5, 2.0, n)
        m = rng.standard_normal(n) * 1e17
        v = rng.uniform(0.1, 1, n) * 1e35
    elif name == "neg_zero":
        z = (grp % 3 == 0) | ((grp % 3 == 1) & (lane == grp % 4))
        gr[z] = -0.0
        fresh = z & (grp % 6 == 0)                                          # -0.0 onto m = v = +0: the fixed point, whole groups
        m[fresh] = 0.0; v[fresh] = 0.0
    elif name in ("f16_edges", "bf16_ties"):
        if name == "f16_edges":
            edge = np.array(F16_EDGE_VALUES, dtype=f32)
        else:
            edge = np.array(BF16_EDGE_BITS, dtype=u32).view(f32)
        edge = np.concatenate([edge, -edge])
        k = np.arange(n // 2)
        p[: n // 2] = edge[k % edge.size]
        gr[: n // 2] = 0.0; m[: n // 2] = 0.0; v[: n // 2] = 1.0           # m' = 0: the update is exactly 0 and p' = p, the edge value
        if name == "f16_edges":
            p[n // 2:] = sgn()[n // 2:] * 10.0 ** rng.uniform(-8, 4.8, n - n // 2)     # updated values across f16's whole range
    elif name == "denormal":
        gr = sgn() * 10.0 ** rng.uniform(-44, -36, n)                       # gr, gr - m, their products: below 2^-126
        m = rng.standard_normal(n) * 10.0 ** rng.uniform(-44, -38, n)
        v = 10.0 ** rng.uniform(-14, -10, n)                                # v' itself stays normal: its root must stay well conditioned
        p = np.where(lane == 3, sgn() * 10.0 ** rng.uniform(-44, -38, n), p)
    g = f32(gr) * f32(SCALE)
    if name == "neg_zero":
        assert np.signbit(g[gr == 0]).all()
    m = f32(m)
    m[m == 0] = 0.0                                                         # (an underflow to -0.0: the sets keep zero moments at +0)
    out = dict(p=f32(p), g=g.astype(f32), m=m, v=f32(v), eps=eps)
    assert np.isfinite(out["g"]).all() and np.isfinite(out["p"]).all() and (out["v"] >= 0).all()
    assert not np.signbit(out["m"][out["m"] == 0]).any()
    return out


def mlp_from_flat(w):
    """The five weight matrices W1 [64,32], W2 [16,64], W3 [64,32], W4 [64,64], W5 [3,64] of a flat [NW] vector."""
    shapes, out, o = ((64, 32), (16, 64), (64, 32), (64, 64), (3, 64)), [], 0
    for s in shapes:
        out.append(w[o:o + s[0] * s[1]].reshape(s))
        o += s[0] * s[1]
    assert o == NW
    return out
