"""CPU checks of tests/optim_reference.py: the float32 restatement of Adam stays within the derived bounds of the float64 contract
on every named input set and the bounds are not vacuous; the scalar state machine reproduces a hand-written table; every
deliberate defect (`alter=`) fails the assertion tests/test_gpu_optim_exact.py applies to the kernels; the 16-bit roundings agree
with independent statements; and the distance between the C ABI's float32 hyperparameters and torch's doubles is what
profiles/PARITY_NOTES.md says."""
import math

import numpy as np
import pytest

import optim_reference as R

f32, f64 = np.float32, np.float64
B1, B2 = 0.9, 0.999


def _state32(t, lr=1e-2, scale=R.SCALE):
    """A float32 state vector as a prologue leaves it at optimizer step t (every value rounded once from float64)."""
    sf = np.zeros(8, f32)
    sf[R.SF_SCALE], sf[R.SF_INV], sf[R.SF_LR] = scale, 1.0 / scale, lr
    sf[R.SF_BC1], sf[R.SF_BC2S] = 1.0 - R.hyper(B1) ** t, math.sqrt(1.0 - R.hyper(B2) ** t)
    return sf


CASES = [(name, eps, t) for name in R.SETS for eps in R.input_set(name, 8)["eps"] for t in (1, 7, 1000)]


def test_adam32_within_the_derived_bounds_of_adam64_and_the_bounds_are_not_vacuous():
    worst = {"m'": 0.0, "v'": 0.0, "p'": 0.0, "dp": 0.0}
    for name, eps, t in CASES:
        s = R.input_set(name, 4096)
        c = R.consts_from_state(_state32(t), B1, B2, eps)
        floor = R.DENORMAL_FLOOR if name == "denormal" else 0.0
        p1, m1, v1, dp = R.adam32(s["p"], s["g"], s["m"], s["v"], c)
        w = R.assert_step_within(dict(p=p1, m=m1, v=v1), s, c, "%s eps=%g t=%d" % (name, eps, t), floor=floor)
        dp64 = R.adam64(s["p"], s["g"], s["m"], s["v"], c)[3]
        Bdp = R.adam_bounds(s["p"], s["g"], s["m"], s["v"], c, floor=floor)[3]
        err = np.abs(dp.astype(f64) - dp64)
        assert (err <= Bdp).all(), (name, eps, t, float(np.max(err / np.maximum(Bdp, R.TINY))))
        if name != "denormal":
            w["dp"] = float(np.max(err / np.maximum(Bdp, R.TINY)))
            for k in worst:
                worst[k] = max(worst[k], w[k])
    print("worst error / bound:", worst)
    for k, r in worst.items():
        assert 1.0 / 64 <= r <= 1.0, (k, r)


def test_fixed_point_and_exact_widening():
    s = R.input_set("fixed_point", 4096)
    c = R.consts_from_state(_state32(3), B1, B2, 1e-15)
    out = R.adam_step32(s["p"], s["g"], s["m"], s["v"], c, copy_kind=1, copy=R.bf16_rne(s["p"]))
    z = (s["g"] == 0) & (s["m"] == 0) & (s["v"] == 0)
    assert z.sum() > 1000 and (~z).sum() > 1000
    for k in ("p", "m", "v"):
        R.assert_bits_equal(out[k][z], s[k][z], k)
    assert not out["g"].any()
    # -0.0 gradients: onto m = v = +0 the entry stays where it is, bit for bit
    s = R.input_set("neg_zero", 4096)
    out = R.adam_step32(s["p"], s["g"], s["m"], s["v"], c)
    z = np.signbit(s["g"]) & (s["g"] == 0) & (s["m"] == 0) & (s["v"] == 0)
    assert z.sum() > 100
    for k in ("p", "m", "v"):
        R.assert_bits_equal(out[k][z], s[k][z], k)
    # an f16 gradient buffer is widened exactly: same result as the float32 array holding the same values
    g16 = (R.input_set("typical", 4096)["g"] * f32(2.0**-6)).astype(np.float16)
    s = R.input_set("typical", 4096)
    a = R.adam_step32(s["p"], g16, s["m"], s["v"], c)
    b = R.adam_step32(s["p"], g16.astype(f64).astype(f32), s["m"], s["v"], c)
    for k in ("p", "m", "v"):
        R.assert_bits_equal(a[k], b[k], k)
    assert a["g"].dtype == np.float16 and not a["g"].any()


def test_skipped_step_touches_nothing_but_the_gradient():
    s = R.input_set("typical", 4096)
    c = R.consts_from_state(_state32(3), B1, B2, 1e-15)
    stale = (R.bf16_rne(s["p"]) ^ 0x0101).astype(np.uint16)
    out = R.adam_step32(s["p"], s["g"], s["m"], s["v"], c, skip=True, copy=stale, copy_kind=1)
    for k in ("p", "m", "v"):
        R.assert_bits_equal(out[k], s[k], k)
    R.assert_bits_equal(out["copy"], stale, "copy")
    assert not out["g"].any()


# ------------------------------------------------------------------------------------------------ the scalar state machine
SCHEDULE = dict(lr0=1e-2, eta_min=1e-2 / 30, t_max=8, beta1=B1, beta2=B2, growth=2.0, backoff=0.5, growth_interval=3)
INF_STEPS = (4, 5, 11)
# after step k: (iter, opt_step, growth tracker, skip, skipped_total, loss scale); written by hand from the contract
EXPECTED = [
    (1, 1, 1, 0, 0, 1024.0),
    (2, 2, 2, 0, 0, 1024.0),
    (3, 3, 0, 0, 0, 2048.0),       # third clean step: the scale grows, the tracker starts over
    (4, 4, 1, 0, 0, 2048.0),
    (5, 4, 0, 1, 1, 1024.0),       # inf: skipped, backoff, tracker reset, opt_step stays
    (6, 4, 0, 1, 2, 512.0),        # inf again
    (7, 5, 1, 0, 2, 512.0),
    (8, 6, 2, 0, 2, 512.0),
    (9, 7, 0, 0, 2, 1024.0),       # growth
    (10, 8, 1, 0, 2, 1024.0),
    (11, 9, 2, 0, 2, 1024.0),
    (12, 9, 0, 1, 3, 512.0),       # inf on the step that would have grown the scale
    (13, 10, 1, 0, 3, 512.0),
    (14, 11, 2, 0, 3, 512.0),
]
INV_SCALE = [1 / 1024, 1 / 1024, 1 / 1024, 1 / 2048, 1 / 2048, 1 / 1024, 1 / 512, 1 / 512, 1 / 512, 1 / 1024, 1 / 1024, 1 / 1024,
             1 / 512, 1 / 512]                                               # the scale each step STARTED with


def _run_schedule(alter=None, steps=14, inf_steps=INF_STEPS, init_scale=1024.0, **over):
    kw = dict(SCHEDULE, **over)
    sf, si = [0.0] * 8, [0] * 8
    sf[R.SF_SCALE] = init_scale
    out = []
    for k in range(steps):
        si[R.SI_FOUND] = int(k in inf_steps)
        sf, si = R.prologue64(sf, si, alter=alter, **kw)
        out.append((list(sf), list(si)))
    return out


def test_prologue64_reproduces_the_hand_written_table():
    lr0, eta = R.hyper(SCHEDULE["lr0"]), R.hyper(SCHEDULE["eta_min"])
    b1, b2 = R.hyper(B1), R.hyper(B2)
    for k, (sf, si) in enumerate(_run_schedule()):
        assert (si[0], si[1], si[2], si[4], si[5], sf[R.SF_SCALE]) == EXPECTED[k], k
        assert si[R.SI_FOUND] == 0 and sf[R.SF_INV] == INV_SCALE[k], k
        want = eta + (lr0 - eta) * (1 + math.cos(math.pi * min(k, 8) / 8)) / 2
        assert sf[R.SF_LR] == want, k
        if k >= 8:
            assert sf[R.SF_LR] == eta, k                                    # exactly eta_min from t_max on
        t = EXPECTED[k][1]
        assert sf[R.SF_BC1] == 1 - b1 ** t and sf[R.SF_BC2S] == math.sqrt(1 - b2 ** t), k
    assert _run_schedule()[0][0][R.SF_LR] == lr0


def test_amp_prologue64():
    sf, si = [0.0] * 8, [0] * 8
    sf[R.SF_SCALE], si[R.SI_ITER], si[R.SI_GROWTH] = 77.0, 5, 2
    sf, si = R.amp_prologue64(sf, si, 4096.0, 0.0, 3e-3, B1, B2)
    assert (si[R.SI_OPT], si[R.SI_SKIP], si[R.SI_SKIPPED]) == (1, 0, 0) and sf[R.SF_INV] == 1 / 4096 and sf[R.SF_LR] == R.hyper(3e-3)
    sf, si = R.amp_prologue64(sf, si, 8192.0, 1.0, 2e-3, B1, B2)
    assert (si[R.SI_OPT], si[R.SI_SKIP], si[R.SI_SKIPPED]) == (1, 1, 1) and sf[R.SF_INV] == 1 / 8192
    assert sf[R.SF_BC1] == 1 - R.hyper(B1) and sf[R.SF_LR] == R.hyper(2e-3)
    sf, si = R.amp_prologue64(sf, si, None, None, 2e-3, B1, B2)            # no scaler: scale 1, never skip
    assert (si[R.SI_OPT], si[R.SI_SKIP], si[R.SI_SKIPPED]) == (2, 0, 1) and sf[R.SF_INV] == 1.0
    assert sf[R.SF_BC2S] == math.sqrt(1 - R.hyper(B2) ** 2)
    assert (sf[R.SF_SCALE], si[R.SI_ITER], si[R.SI_GROWTH]) == (77.0, 5, 2)    # not this form's business


def test_scalar_bounds_admit_a_float32_evaluation_and_bc_relative_error_is_what_the_docstring_says():
    """numpy's float32 pow / cos / sqrt stand in for the device's: within the bounds at every step of the schedule; and
    1 - beta2^t formed in float32 is off by ~1e-5 relatively at t = 1 although every operation is good to an ulp."""
    one, b1, b2 = f32(1), f32(B1), f32(B2)
    worst = 0.0
    for t in range(1, 60):
        bc1, y = one - np.power(b1, f32(t)), one - np.power(b2, f32(t))
        assert abs(float(bc1) - (1 - R.hyper(B1) ** t)) <= R.bc_abs_bound()
        assert abs(float(y) - (1 - R.hyper(B2) ** t)) <= R.bc_abs_bound()
        assert abs(float(np.sqrt(y)) - math.sqrt(1 - R.hyper(B2) ** t)) <= R.bc2_sqrt_abs_bound(B2, t)
        worst = max(worst, abs(float(y) - (1 - R.hyper(B2) ** t)) / (1 - R.hyper(B2) ** t))
    assert 1e-6 < worst < R.bc_abs_bound() / 1e-3 * 1.01
    lr0, eta, T = f32(1e-2), f32(1e-2 / 30), 24
    for k in range(40):
        c = np.cos(f32(np.pi) * f32(min(k, T)) / f32(T))
        lr = eta + (lr0 - eta) * f32(0.5) * (one + c)
        assert lr.dtype == f32
        assert abs(float(lr) - R.cosine_lr64(1e-2, 1e-2 / 30, T, k)) <= R.lr_abs_bound(1e-2, 1e-2 / 30, T, k), k


# ------------------------------------------------------------------------------------------------ every defect is caught
def _scalar_defect_caught(alter, **kw):
    clean, bad = _run_schedule(**kw), _run_schedule(alter=alter, **kw)
    for k, ((sf, si), (bsf, bsi)) in enumerate(zip(clean, bad)):
        got_sf = np.array(bsf, f32)                                         # what a kernel with the defect would leave
        e = R.scalar_bounds(sf, si, SCHEDULE["lr0"], SCHEDULE["eta_min"], SCHEDULE["t_max"], B2, k)
        R.assert_scalar_state(np.array(sf, f32), si, sf, si, *e, what="clean step %d" % k)       # the clean form passes
        try:
            R.assert_scalar_state(got_sf, bsi, sf, si, *e, what="step %d" % k)
        except AssertionError as err:
            return k, str(err)
    return None, None


@pytest.mark.parametrize("alter,first,word", [("lr_at_iter_plus_1", 0, "lr"), ("growth_not_reset_on_skip", 4, "state_i"),
                                              ("opt_step_on_skip", 4, "state_i"), ("inv_scale_after_growth", 2, "inv_scale")])
def test_scalar_defects_fail_the_state_assertion(alter, first, word):
    k, msg = _scalar_defect_caught(alter)
    assert k == first and word in msg, (k, msg)


def test_amp_opt_step_on_skip_is_caught():
    sf, si = R.amp_prologue64([0.0] * 8, [0] * 8, 512.0, 1.0, 1e-3, B1, B2)
    bsf, bsi = R.amp_prologue64([0.0] * 8, [0] * 8, 512.0, 1.0, 1e-3, B1, B2, alter="opt_step_on_skip")
    with pytest.raises(AssertionError, match="state_i"):
        R.assert_scalar_state(np.array(bsf, f32), bsi, sf, si, 0.0, R.bc_abs_bound(), R.bc2_sqrt_abs_bound(B2, 1))


def _adam_defect(alter, name, eps, t=3, skip=False, copy_kind=0, stale=False):
    s = R.input_set(name, 4096)
    c = R.consts_from_state(_state32(t), B1, B2, eps)
    copy = R.round16(s["p"], copy_kind) if copy_kind else None
    if stale:
        copy = (copy ^ 0x0101).astype(np.uint16)
    want = R.adam_step32(s["p"], s["g"], s["m"], s["v"], c, skip=skip, copy=copy, copy_kind=copy_kind)
    got = R.adam_step32(s["p"], s["g"], s["m"], s["v"], c, skip=skip, copy=copy, copy_kind=copy_kind, alter=alter)
    return s, c, want, got


@pytest.mark.parametrize("alter,name,eps", [("bc2_for_bc2_sqrt", "typical", 1e-15), ("bc2_for_bc2_sqrt", "first_step", 1e-15),
                                            ("eps_before_divide", "tiny_v", 1e-8), ("eps_before_divide", "typical", 1e-8)])
def test_update_defects_fail_both_adam_assertions(alter, name, eps):
    s, c, want, got = _adam_defect(alter, name, eps)
    R.assert_step_exact(want, want)
    R.assert_step_within(want, s, c)
    with pytest.raises(AssertionError, match="p'"):
        R.assert_step_exact(got, want)
    with pytest.raises(AssertionError, match="p'"):
        R.assert_step_within(got, s, c)


def test_eps_before_the_divide_is_invisible_at_1e_15():
    """(sqrt(v) + 1e-15) / bc2_sqrt and sqrt(v) / bc2_sqrt + 1e-15 are the same float32 on ordinary moments: the reference's
    eps = 1e-15 cannot tell the two orders apart, which is why the kernels are also run with eps = 1e-8."""
    s, c, want, got = _adam_defect("eps_before_divide", "typical", 1e-15)
    R.assert_step_exact(got, want)


@pytest.mark.parametrize("alter,name,kw,word", [
    ("bf16_truncated", "bf16_ties", dict(copy_kind=1), "storage copy"),
    ("bf16_truncated", "typical", dict(copy_kind=1), "storage copy"),
    ("grad_not_cleared", "typical", dict(), "gradient not cleared"),
    ("grad_not_cleared", "typical", dict(skip=True), "gradient not cleared"),
    ("copy_on_skip", "typical", dict(skip=True, copy_kind=1, stale=True), "storage copy"),
    ("copy_on_skip", "f16_edges", dict(skip=True, copy_kind=2, stale=True), "storage copy")])
def test_outcome_defects_fail_the_exact_assertion(alter, name, kw, word):
    s, c, want, got = _adam_defect(alter, name, 1e-15, **kw)
    R.assert_step_exact(want, want)
    with pytest.raises(AssertionError, match=word):
        R.assert_step_exact(got, want)


def test_every_alter_is_exercised():
    import inspect
    import sys
    src = inspect.getsource(sys.modules[__name__])
    for a in R.ALTERS:
        assert src.count('"%s"' % a) >= 1, a


# ------------------------------------------------------------------------------------------------ 16-bit roundings
def _all_interesting_f32():
    rng = np.random.default_rng(5)
    rnd = rng.integers(0, 2**32, 200000, dtype=np.uint64).astype(np.uint32)
    edges = np.array(R.BF16_EDGE_BITS, np.uint32)
    fe = np.array(R.F16_EDGE_VALUES, f32).view(np.uint32)
    near = (fe[:, None].astype(np.int64) + np.arange(-3, 4)[None, :]).ravel().astype(np.uint32)
    special = np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffc12345, 1, 0x007fffff], np.uint32)
    b = np.concatenate([rnd, edges, edges | 0x80000000, near, near | 0x80000000, special])
    return b.view(f32)


def test_f16_rne_against_numpy_and_by_hand():
    x = _all_interesting_f32()
    got = R.f16_rne(x)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    nan = np.isnan(x)
    assert R.is_nan16(got[nan], 2).all() and not R.is_nan16(got[~nan], 2).any()
    assert np.array_equal(got[~nan], want[~nan])
    hand = {65504.0: 0x7bff, 65519.0: 0x7bff, 65520.0: 0x7c00, 65536.0: 0x7c00, -65520.0: 0xfc00, 2.0**-14: 0x0400, 2.0**-24: 0x0001,
            2.0**-25: 0x0000, 3 * 2.0**-25: 0x0002, 2.0**-25 * (1 + 2.0**-20): 0x0001, 1 + 2.0**-11: 0x3c00, 1 + 3 * 2.0**-11: 0x3c02,
            2.0**-14 * (1 - 2.0**-11): 0x0400, -0.0: 0x8000, float("inf"): 0x7c00}
    for v, bits in hand.items():
        assert int(R.f16_rne(np.array([v], f32))[0]) == bits, (v, hex(bits))


def test_bf16_rne_against_a_float64_statement_and_by_hand():
    x = _all_interesting_f32()
    got = R.bf16_rne(x)
    nan = np.isnan(x)
    assert R.is_nan16(got[nan], 1).all() and not R.is_nan16(got[~nan], 1).any()
    # nearest bf16 neighbour, ties to the even one, stated on values: the two candidates are trunc and trunc + 1 (in bits)
    xf = x[~nan]
    lo = (xf.view(np.uint32) & 0xffff0000)
    hi = (lo.astype(np.uint64) + 0x10000).astype(np.uint32)                 # next bf16 away from zero (may be inf)
    with np.errstate(all="ignore"):
        lo_v, hi_v = lo.view(f32).astype(f64), hi.view(f32).astype(f64)
        hi_v = np.where(np.isinf(hi_v) & np.isfinite(xf), np.sign(hi_v) * 2.0**128, hi_v)      # the overflow threshold, as IEEE rounds
        d_lo, d_hi = np.abs(xf.astype(f64) - lo_v), np.abs(hi_v - xf.astype(f64))
    pick_hi = (d_hi < d_lo) | ((d_hi == d_lo) & ((lo >> 16) & 1 == 1))
    pick_hi &= np.isfinite(xf)
    want = np.where(pick_hi, hi >> 16, lo >> 16).astype(np.uint16)
    assert np.array_equal(got[~nan], want)
    hand = {0x3f808000: 0x3f80, 0x3f818000: 0x3f82, 0x3f807fff: 0x3f80, 0x3f808001: 0x3f81, 0x7f7f8000: 0x7f80, 0x7f7f7fff: 0x7f7f,
            0x80000000: 0x8000, 0x00008000: 0x0000, 0x00018000: 0x0002, 0xff800000: 0xff80}
    for b, bits in hand.items():
        assert int(R.bf16_rne(np.array([b], np.uint32).view(f32))[0]) == bits, (hex(b), hex(bits))
    assert int(R.bf16_trunc(np.array([0x3f818000], np.uint32).view(f32))[0]) == 0x3f81


# ------------------------------------------------------------------------------------------------ MSE and the slab sum
@pytest.mark.parametrize("bg", [0.0, 1.0])
@pytest.mark.parametrize("scale", [1.0, 2.0**15])
def test_mse32_within_derived_bounds_of_mse64(bg, scale):
    rng = np.random.default_rng(11)
    n = 1025
    rgb, op, tg = rng.uniform(0, 1, (n, 3)).astype(f32), rng.uniform(0, 1, n).astype(f32), rng.uniform(0, 1, (n, 3)).astype(f32)
    tg[:64] = (rgb[:64].astype(f64) + (bg * (1 - op[:64].astype(f64)))[:, None] + 1e-7).astype(f32)      # cancels to ~1e-7
    loss, sq, g_rgb, g_op = R.mse64(rgb, op, tg, bg, n, scale)
    se32, g32, go32 = R.mse32(rgb, op, tg, bg, n, scale)
    b = np.abs(bg * (1 - op.astype(f64)))[:, None]
    diff = rgb.astype(f64) + bg * (1 - op.astype(f64))[:, None] - tg
    e = R.U * (2 * b + np.abs(diff + tg) + np.abs(diff)) * R.SLACK         # the forming error of one difference (docstring)
    k = 2.0 / (3.0 * n) * scale
    Bg = k * e + 3 * R.U * np.abs(g_rgb) * R.SLACK                          # k: the divide, the scale (exact); the product
    assert (np.abs(g32 - g_rgb) <= Bg).all()
    assert (np.abs(go32 - g_op) <= bg * Bg.sum(axis=1) + 6 * R.U * bg * np.abs(g_rgb).sum(axis=1) * R.SLACK).all()
    Bs = (e * (2 * np.abs(diff) + e)).sum(axis=1) + 4 * R.U * sq * R.SLACK
    assert (np.abs(se32 - sq) <= Bs).all()
    # the float64 sum of the float32 terms is well inside the loss bound, and the bound is a small fraction of the loss
    assert abs(float(se32.astype(f64).sum()) / (3 * n) - loss) <= R.mse_loss_bound(rgb, op, tg, bg, n) <= 1e-3 * loss
    if bg == 0.0:
        assert not g_op.any() and not go32.any()


def test_dw_reduce64():
    rng = np.random.default_rng(3)
    parts = rng.standard_normal((5, R.NW)).astype(f32)
    parts[3:] = 1e30                                                         # beyond n_parts
    s, a = R.dw_reduce64(parts, 3)
    assert np.array_equal(s, parts[0].astype(f64) + parts[1] + parts[2]) and np.array_equal(a, np.abs(parts[:3].astype(f64)).sum(0))
    assert (R.dw_bound(3, np.ones(R.NW), a) == 19 * R.U * (1 + a)).all()


# ------------------------------------------------------------------------------------------------ distance to torch's doubles
def test_distance_between_float32_hyperparameters_and_torch_doubles():
    """torch.optim.Adam(betas=(0.9, 0.999)) uses the Python doubles; the C ABI takes `float`.  The relative distance of the bias
    corrections is recorded in profiles/PARITY_NOTES.md and stays below the rtol (2e-5) of tests/test_gpu_apex_adam.py."""
    def rel(beta, t):
        a, b = 1 - beta ** t, 1 - R.hyper(beta) ** t
        return abs(a - b) / a
    assert rel(0.999, 1) == pytest.approx(1.29e-5, rel=0.01)
    assert rel(0.999, 1000) == pytest.approx(7.5e-6, rel=0.01)
    assert rel(0.999, 5000) == pytest.approx(4.4e-7, rel=0.02)
    assert rel(0.9, 1) == pytest.approx(2.4e-7, rel=0.02)
    for beta in (0.9, 0.999):
        for t in list(range(1, 200)) + [1000, 5000, 20000]:
            assert rel(beta, t) < 2e-5, (beta, t)
