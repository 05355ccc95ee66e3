"""The training step's epilogue on the GPU, held to tests/optim_reference.py: the scalar state machine of the four prologue forms
against prologue64 / amp_prologue64 after every step; every form of the Adam update bit for bit against the float32 restatement
driven by the device's own state, and within the derived bounds of the float64 contract driven by prologue64; the storage copies,
the gradient clearing and the skipped step; the inf / nan checks with their arrival counters; the two MSE kernels; the slab sum.
Every tolerance here is zero, a bound derived in optim_reference.py's docstring, or the measured powf / cosf allowance recorded in
profiles/PARITY_NOTES.md.  The kernels are called through the C ABI."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import torch

import optim_reference as R

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64
B1, B2 = 0.9, 0.999
SCHED = dict(lr0=1e-2, eta_min=1e-2 / 30, t_max=24, beta1=B1, beta2=B2, growth=2.0, backoff=0.5, growth_interval=5)
# clean steps 0-3, inf on step 4 (the step that would have grown the scale), growth on 9, two infs in a row, growth on 18, 23, 28
INF_STEPS = (4, 12, 13, 30)
BIG_N = 4 * (4096 * 256 + 3)            # just past the 4096-block grid cap of the 256-thread sweeps: the grid-stride loop's second trip
SIZES = (4, 1020, 1024, 1028, 4 * 256 * 17, BIG_N)


@pytest.fixture(scope="module")
def E(hip_lib):
    from ngp_hip import lib as L
    from ngp_hip import ops
    return SimpleNamespace(lib=hip_lib, check=L.check, ptr=ops._ptr, stream=ops._stream, ops=ops)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a.copy()).cuda()


def host(t, dtype=None):
    a = t.detach().cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def new_state(scale=R.SCALE):
    sf, si = np.zeros(8, f32), np.zeros(8, np.int32)
    sf[R.SF_SCALE] = scale
    return dev(sf), dev(si)


def prologue_args(kw):
    return (kw["lr0"], kw["eta_min"], kw["t_max"], kw["beta1"], kw["beta2"], kw["growth"], kw["backoff"], kw["growth_interval"])


def run_prologue(E, sf, si, kw=SCHED):
    E.check(E.lib.ngp_train_prologue(E.ptr(sf), E.ptr(si), *prologue_args(kw), E.stream()), "ngp_train_prologue")


def rel_consts(sf64, e):
    e_lr, e_bc1, e_bc2s = e
    return e_lr / sf64[R.SF_LR] + e_bc1 / sf64[R.SF_BC1] + e_bc2s / sf64[R.SF_BC2S]


# ------------------------------------------------------------------------------------------------ the scalar state machine
@pytest.mark.parametrize("form", ["prologue", "prologue_reduce"])
def test_prologue_trajectory(E, form):
    sf, si = new_state()
    sf64, si64 = [float(x) for x in host(sf)], [int(x) for x in host(si)]
    rng = np.random.default_rng(1)
    part = rng.standard_normal(R.NW).astype(f32)
    dW0 = rng.standard_normal(R.NW).astype(f32)
    parts, dW = dev(np.concatenate([part, np.full(R.NW, np.nan, f32)])), dev(dW0)
    worst = dict(lr=0.0, bc1=0.0, bc2_sqrt=0.0)
    for k in range(40):
        if k in INF_STEPS:
            si[R.SI_FOUND] = 1
            si64[R.SI_FOUND] = 1
        if form == "prologue":
            run_prologue(E, sf, si)
        else:
            dW.copy_(torch.from_numpy(dW0))
            E.check(E.lib.ngp_train_prologue_reduce(E.ptr(sf), E.ptr(si), *prologue_args(SCHED), E.ptr(parts), 1, E.ptr(dW), E.stream()),
                    "ngp_train_prologue_reduce")
        sf64, si64 = R.prologue64(sf64, si64, **SCHED)
        e = R.scalar_bounds(sf64, si64, SCHED["lr0"], SCHED["eta_min"], SCHED["t_max"], B2, k)
        got_sf, got_si = host(sf), host(si)
        R.assert_scalar_state(got_sf, got_si, sf64, si64, *e, what="%s step %d" % (form, k))
        for name, idx, b in (("lr", R.SF_LR, e[0]), ("bc1", R.SF_BC1, e[1]), ("bc2_sqrt", R.SF_BC2S, e[2])):
            if b > 0:
                worst[name] = max(worst[name], abs(float(got_sf[idx]) - sf64[idx]) / b)
        if form == "prologue_reduce":
            s, a = R.dw_reduce64(host(parts), 1)
            assert (np.abs(host(dW).astype(f64) - (dW0.astype(f64) + s)) <= R.dw_bound(1, dW0, a)).all(), k
    print("%s: worst error / bound %s" % (form, worst))
    # four backoffs (4, 12, 13, 30) and five growths (9, 18, 23, 28, 35)
    assert si64[R.SI_SKIPPED] == 4 and si64[R.SI_OPT] == 36 and sf64[R.SF_SCALE] == R.SCALE * 2.0**-4 * 2.0**5


@pytest.mark.parametrize("form", ["amp", "amp_null", "amp_check", "amp_check_null_scale"])
def test_amp_prologue_trajectory(E, form):
    """The scaler's tensors (or NULLs) come from outside: the scale and the flag follow the same schedule GradScaler would keep,
    lr is the host scheduler's value.  The fused form finds the inf in the gradients itself."""
    sf, si = new_state(77.0)                                                # the loss scale slot is not this form's business
    si[R.SI_ITER], si[R.SI_GROWTH] = 5, 2
    sf64, si64 = [float(x) for x in host(sf)], [int(x) for x in host(si)]
    gs64, gi64 = [0.0] * 8, [0] * 8                                         # the scaler: prologue64 run beside it
    gs64[R.SF_SCALE] = 2.0**12
    grads = [dev(np.linspace(-1, 1, n).astype(f32)) for n in (4096, 16, 1028)]
    G = (ctypes.c_void_p * 3)(*[g.data_ptr() for g in grads])
    N = (ctypes.c_longlong * 3)(*[g.numel() for g in grads])
    pair, done = dev(np.zeros(2, f32)), torch.zeros(17 * 32, dtype=torch.int32, device="cuda")
    scale_t, found_t = dev(np.zeros(1, f32)), dev(np.zeros(1, f32))
    for k in range(40):
        inf = k in INF_STEPS
        scale = gs64[R.SF_SCALE]
        lr = R.cosine_lr64(SCHED["lr0"], SCHED["eta_min"], SCHED["t_max"], k)
        scale_t.fill_(scale)
        use_scale = form in ("amp", "amp_check")
        if form == "amp":
            found_t.fill_(1.0 if inf else 0.0)
            E.check(E.lib.ngp_adam_amp_prologue(E.ptr(sf), E.ptr(si), E.ptr(scale_t), E.ptr(found_t), lr, B1, B2, E.stream()), form)
        elif form == "amp_null":
            inf = False
            E.check(E.lib.ngp_adam_amp_prologue(E.ptr(sf), E.ptr(si), E.ptr(None), E.ptr(None), lr, B1, B2, E.stream()), form)
        else:
            found, nxt = pair[k % 2:k % 2 + 1], pair[1 - k % 2:2 - k % 2]
            assert float(found) == 0.0                                      # cleared by the previous launch (or never set)
            if inf:
                grads[k % 3][(7 * k) % grads[k % 3].numel()] = float("inf")
            E.check(E.lib.ngp_adam_amp_check_prologue(3, G, N, E.ptr(found), E.ptr(nxt), E.ptr(done), E.ptr(sf), E.ptr(si),
                                                      E.ptr(scale_t if use_scale else None), lr, B1, B2, E.stream()), form)
            if inf:
                grads[k % 3][(7 * k) % grads[k % 3].numel()] = 0.5
            assert float(found) == (1.0 if inf else 0.0) and float(nxt) == 0.0 and not done.any()
        sf64, si64 = R.amp_prologue64(sf64, si64, scale if use_scale else None, 1.0 if inf else (None if form == "amp_null" else 0.0),
                                      lr, B1, B2)
        e = R.scalar_bounds(sf64, si64, None, None, None, B2, k)
        R.assert_scalar_state(host(sf), host(si), sf64, si64, *e, what="%s step %d" % (form, k))
        gi64[R.SI_FOUND] = int(inf)
        gs64, gi64 = R.prologue64(gs64, gi64, **SCHED)
    assert si64[R.SI_OPT] == (40 if form == "amp_null" else 36) and si64[R.SI_ITER] == 5 and sf64[R.SF_SCALE] == 77.0


# ------------------------------------------------------------------------------------------------ Adam, bit for bit
@functools.lru_cache(maxsize=None)
def device_state(t, skip=False):
    """(device sf, si, their host copies, prologue64's state beside them, rel_consts) after t clean steps (and one skipped)."""
    from ngp_hip import lib as L
    from ngp_hip import ops
    E_ = SimpleNamespace(lib=L.load(), check=L.check, ptr=ops._ptr, stream=ops._stream)
    kw = dict(SCHED, growth_interval=2000)
    sf, si = new_state()
    sf64, si64 = [float(x) for x in host(sf)], [int(x) for x in host(si)]
    for k in range(t + int(skip)):
        if k == t:
            si[R.SI_FOUND] = 1
            si64[R.SI_FOUND] = 1
        run_prologue(E_, sf, si, kw)
        sf64, si64 = R.prologue64(sf64, si64, **kw)
    e = R.scalar_bounds(sf64, si64, kw["lr0"], kw["eta_min"], kw["t_max"], B2, t + int(skip) - 1)
    R.assert_scalar_state(host(sf), host(si), sf64, si64, *e, what="state t=%d" % t)
    assert int(host(si)[R.SI_SKIP]) == int(skip) and float(host(sf)[R.SF_INV]) == 1.0 / R.SCALE
    return SimpleNamespace(sf=sf, si=si, sf_h=host(sf).copy(), sf64=sf64, rel=rel_consts(sf64, e), skip=skip)


@functools.lru_cache(maxsize=None)
def cached_set(name, n):
    return R.input_set(name, n)


def launch_adam(E, form, st, s, eps, copy_kind=0, grad16=False, stale=False, pairs=0):
    """Run one Adam form on input set s under device state st; returns (got, before): got = dict(p, m, v, g, copy, wpack)."""
    n = s["p"].size
    g_in = s["g"].astype(f16) if grad16 else s["g"]
    before = dict(p=s["p"], g=g_in, m=s["m"], v=s["v"])
    p, m, v = dev(s["p"]), dev(s["m"]), dev(s["v"])
    g = dev(g_in.view(np.int16)) if grad16 else dev(g_in)
    copy0 = copy_t = wpack = None
    if copy_kind:
        copy0 = R.round16(s["p"], copy_kind)
        if stale:
            copy0 = (copy0 ^ 0x0101).astype(np.uint16)
        copy_t = dev(copy0)
    common = (E.ptr(st.sf), E.ptr(st.si), B1, B2, eps)
    if form == "step":
        rc = E.lib.ngp_adam_step(E.ptr(p), E.ptr(g), E.ptr(m), E.ptr(v), n, *common, E.stream())
    elif form == "step_bf16":
        rc = E.lib.ngp_adam_step_bf16(E.ptr(p), E.ptr(g), E.ptr(m), E.ptr(v), n, *common, E.ptr(copy_t), E.stream())
    elif form == "all_ex":                                                  # the table range only (mlp == NULL)
        rc = E.lib.ngp_adam_all_ex(E.ptr(p), E.ptr(g), int(grad16), E.ptr(m), E.ptr(v), n, E.ptr(copy_t), copy_kind, E.ptr(None),
                                   E.ptr(None), E.ptr(None), E.ptr(None), *common, pairs, E.ptr(None), E.stream())
    elif form == "mlp_pack":
        assert n == R.NW
        wpack = torch.zeros(E.lib.ngp_mlp_wpack_halfs(), dtype=torch.float16, device="cuda")
        rc = E.lib.ngp_adam_mlp_pack(E.ptr(p), E.ptr(g), E.ptr(m), E.ptr(v), *common, pairs, E.ptr(wpack), E.stream())
    else:
        raise ValueError(form)
    E.check(rc, form)
    torch.cuda.synchronize()
    got = dict(p=host(p), m=host(m), v=host(v), g=host(g, f16) if grad16 else host(g),
               copy=host(copy_t, np.uint16) if copy_kind else None, wpack=wpack, p_dev=p)
    return got, before, copy0


def check_adam(E, got, before, copy0, st, eps, copy_kind, what, exact=True, floor=0.0):
    c_dev = R.consts_from_state(st.sf_h, B1, B2, eps)
    want = R.adam_step32(before["p"], before["g"], before["m"], before["v"], c_dev, skip=st.skip, copy=copy0, copy_kind=copy_kind)
    same = True
    if exact:
        R.assert_step_exact(got, want, what)
    else:
        same = all(np.array_equal(R.bits(got[k]), R.bits(want[k])) for k in ("p", "m", "v"))
        assert not np.asarray(got["g"]).astype(f32).any(), what
        if copy_kind:
            R.assert_bits_equal(got["copy"], R.round16(got["p"], copy_kind), what + " storage copy")
    if not st.skip:
        b64 = dict(before, g=np.asarray(before["g"]).astype(f32))
        R.assert_step_within(got, b64, c_dev, what + " (device state)", floor=floor)
        # ... and independently of the device's own scalars: an error shared by the prologue and the update shows here
        R.assert_step_within(got, b64, R.consts_from_state(st.sf64, B1, B2, eps), what + " (prologue64)", rel_consts=st.rel, floor=floor)
    return same


def pack_of(E, w_dev, pairs):
    if pairs == 0:
        return E.ops.mlp_pack([torch.from_numpy(w).cuda() for w in R.mlp_from_flat(host(w_dev))])
    W = [torch.from_numpy(w.copy()).cuda() for w in R.mlp_from_flat(host(w_dev))]
    out = torch.zeros(E.lib.ngp_mlp_wpack_halfs(), dtype=torch.float16, device="cuda")
    E.check(E.lib.ngp_mlp_pack(*[E.ptr(w) for w in W], pairs, E.ptr(out), E.stream()), "ngp_mlp_pack")
    return out


SET_EPS = [(name, eps) for name in R.EXACT_SETS for eps in cached_set(name, 8)["eps"]]
F16_GRAD_SETS = tuple(s for s in R.EXACT_SETS if s != "huge")               # |g| of `huge` is beyond f16: not an input of that form
ALL_EX = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]                   # (grad_is_f16, copy_kind); the trainer uses (0,0) (0,1) (1,2)


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("form,copy_kind", [("step", 0), ("step_bf16", 1), ("mlp_pack", 0)])
def test_adam_forms_bit_exact_on_every_set(E, form, copy_kind, t):
    st = device_state(t)
    for name, eps in SET_EPS:
        s = cached_set(name, R.NW if form == "mlp_pack" else 4096)
        pairs = t % 2
        got, before, copy0 = launch_adam(E, form, st, s, eps, copy_kind=copy_kind, pairs=pairs)
        check_adam(E, got, before, copy0, st, eps, copy_kind, "%s %s eps=%g t=%d" % (form, name, eps, t))
        if form == "mlp_pack":
            assert torch.equal(got["wpack"].view(torch.int16), pack_of(E, got["p_dev"], pairs).view(torch.int16)) and got["wpack"].any()


@pytest.mark.parametrize("grad16,copy_kind", ALL_EX)
def test_adam_all_ex_bit_exact_on_every_set(E, grad16, copy_kind):
    st = device_state(3)
    for name, eps in SET_EPS:
        if grad16 and name not in F16_GRAD_SETS:
            continue
        s = cached_set(name, 4096)
        got, before, copy0 = launch_adam(E, "all_ex", st, s, eps, copy_kind=copy_kind, grad16=bool(grad16))
        check_adam(E, got, before, copy0, st, eps, copy_kind, "all_ex f16=%d copy=%d %s eps=%g" % (grad16, copy_kind, name, eps))


@pytest.mark.parametrize("grad16,copy_kind", [(0, 1), (1, 2)])
def test_adam_all_ex_with_the_mlp_block(E, grad16, copy_kind):
    """Table range and MLP block in one launch: both bit-exact, wpack the repack of the updated weights."""
    for st in (device_state(3), device_state(3, skip=True)):
        s, w = cached_set("typical", 4 * 256 * 17), cached_set("cancel", R.NW)
        g_in = s["g"].astype(f16) if grad16 else s["g"]
        p, m, v, g = dev(s["p"]), dev(s["m"]), dev(s["v"]), dev(g_in.view(np.int16) if grad16 else g_in)
        copy0 = (R.round16(s["p"], copy_kind) ^ (0x0101 if st.skip else 0)).astype(np.uint16)
        copy_t = dev(copy0)
        wp, wg, wm, wv = dev(w["p"]), dev(w["g"]), dev(w["m"]), dev(w["v"])
        wpack = torch.zeros(E.lib.ngp_mlp_wpack_halfs(), dtype=torch.float16, device="cuda")
        E.check(E.lib.ngp_adam_all_ex(E.ptr(p), E.ptr(g), grad16, E.ptr(m), E.ptr(v), s["p"].size, E.ptr(copy_t), copy_kind, E.ptr(wp),
                                      E.ptr(wg), E.ptr(wm), E.ptr(wv), E.ptr(st.sf), E.ptr(st.si), B1, B2, 1e-15, 1, E.ptr(wpack),
                                      E.stream()), "ngp_adam_all_ex")
        got = dict(p=host(p), m=host(m), v=host(v), g=host(g, f16) if grad16 else host(g), copy=host(copy_t, np.uint16))
        check_adam(E, got, dict(p=s["p"], g=g_in, m=s["m"], v=s["v"]), copy0, st, 1e-15, copy_kind, "all_ex table skip=%d" % st.skip)
        got_w = dict(p=host(wp), m=host(wm), v=host(wv), g=host(wg), copy=None)
        check_adam(E, got_w, dict(p=w["p"], g=w["g"], m=w["m"], v=w["v"]), None, st, 1e-15, 0, "all_ex mlp skip=%d" % st.skip)
        assert torch.equal(wpack.view(torch.int16), pack_of(E, wp, 1).view(torch.int16)) and wpack.any()


@pytest.mark.parametrize("order", ["largest_last", "largest_first"])
def test_adam_multi_bit_exact(E, order):
    lengths = [4, 1028, R.NW, 4 * 256 * 3 + 4, 70000]
    if order == "largest_first":
        lengths = lengths[::-1]
    names = ["fixed_point", "cancel", "typical", "neg_zero", "first_step"]
    for st in (device_state(3), device_state(3, skip=True)):
        for eps in (1e-15, 1e-8):
            sets = [cached_set(nm, n) for nm, n in zip(names, lengths)]
            T = {k: [dev(s[k]) for s in sets] for k in ("p", "g", "m", "v")}
            arr = {k: (ctypes.c_void_p * 5)(*[t.data_ptr() for t in T[k]]) for k in T}
            N = (ctypes.c_longlong * 5)(*lengths)
            E.check(E.lib.ngp_adam_multi(5, arr["p"], arr["g"], arr["m"], arr["v"], N, E.ptr(st.sf), E.ptr(st.si), B1, B2, eps, E.stream()),
                    "ngp_adam_multi")
            for i, s in enumerate(sets):
                got = dict(p=host(T["p"][i]), m=host(T["m"][i]), v=host(T["v"][i]), g=host(T["g"][i]), copy=None)
                check_adam(E, got, s, None, st, eps, 0, "multi %s tensor %d (%s) eps=%g skip=%d" % (order, i, names[i], eps, st.skip))
    N[2] = 13
    assert E.lib.ngp_adam_multi(5, arr["p"], arr["g"], arr["m"], arr["v"], N, E.ptr(st.sf), E.ptr(st.si), B1, B2, eps, E.stream()) == -1


@pytest.mark.parametrize("form,copy_kind,grad16", [("step", 0, 0), ("step_bf16", 1, 0), ("all_ex", 1, 0), ("all_ex", 2, 1), ("mlp_pack", 0, 0)])
def test_skipped_step_leaves_everything_but_the_gradient(E, form, copy_kind, grad16):
    """The storage copy holds something that is NOT the rounding of p, so a rewrite from stale registers shows."""
    st = device_state(3, skip=True)
    for name in ("typical", "f16_edges", "neg_zero"):
        s = cached_set(name, R.NW if form == "mlp_pack" else 4096)
        got, before, copy0 = launch_adam(E, form, st, s, 1e-15, copy_kind=copy_kind, grad16=bool(grad16), stale=True)
        check_adam(E, got, before, copy0, st, 1e-15, copy_kind, "skipped %s %s" % (form, name))
        for k in ("p", "m", "v"):
            R.assert_bits_equal(got[k], s[k], "skipped %s %s %s" % (form, name, k))
        if copy_kind:
            R.assert_bits_equal(got["copy"], copy0, "skipped %s %s copy" % (form, name))
        if form == "mlp_pack":
            assert torch.equal(got["wpack"].view(torch.int16), pack_of(E, got["p_dev"], 0).view(torch.int16))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form,copy_kind,grad16", [("step", 0, 0), ("step_bf16", 1, 0), ("all_ex", 2, 1)])
def test_adam_sizes(E, form, copy_kind, grad16, n):
    st = device_state(3)
    s = cached_set("typical", n)
    got, before, copy0 = launch_adam(E, form, st, s, 1e-15, copy_kind=copy_kind, grad16=bool(grad16))
    c_dev = R.consts_from_state(st.sf_h, B1, B2, 1e-15)
    want = R.adam_step32(before["p"], before["g"], before["m"], before["v"], c_dev, copy=copy0, copy_kind=copy_kind)
    R.assert_step_exact(got, want, "%s n=%d" % (form, n))


def test_adam_rejects_lengths_that_are_no_multiple_of_four(E):
    st = device_state(3)
    t = [torch.zeros(16, device="cuda") for _ in range(4)]
    c16 = torch.zeros(16, dtype=torch.int16, device="cuda")
    a = [E.ptr(x) for x in t]
    tail = (E.ptr(st.sf), E.ptr(st.si), B1, B2, 1e-15)
    for n in (1, 6, 13):
        assert E.lib.ngp_adam_step(*a, n, *tail, E.stream()) == -1
        assert E.lib.ngp_adam_step_bf16(*a, n, *tail, E.ptr(c16), E.stream()) == -1
        assert E.lib.ngp_adam_all_ex(a[0], a[1], 0, a[2], a[3], n, E.ptr(None), 0, E.ptr(None), E.ptr(None), E.ptr(None), E.ptr(None),
                                     *tail, 0, E.ptr(None), E.stream()) == -1
    torch.cuda.synchronize()
    assert not any(x.any() for x in t)


def test_denormal_set_within_the_floored_bounds(E):
    """Intermediates below 2^-126: held to adam64 with the absolute floor; whether the device also matched adam32 bit for bit is
    printed (recorded in profiles/PARITY_NOTES.md), not required."""
    st = device_state(3)
    for form, copy_kind in (("step", 0), ("step_bf16", 1), ("mlp_pack", 0)):
        s = cached_set("denormal", R.NW if form == "mlp_pack" else 4096)
        got, before, copy0 = launch_adam(E, form, st, s, 1e-15, copy_kind=copy_kind)
        same = check_adam(E, got, before, copy0, st, 1e-15, copy_kind, "denormal " + form, exact=False, floor=R.DENORMAL_FLOOR)
        print("denormal set, %s: bit-identical to adam32: %s" % (form, same))


# ------------------------------------------------------------------------------------------------ a short coupled run
def test_coupled_run_bit_exact_per_step_and_within_the_accumulated_bound(E):
    """48 steps on 4096 parameters with g = 2 (p - target_k) * scale formed on the host from the device's parameters: one inf step,
    two growths, the schedule past t_max.  Every step bit for bit against adam32; the end against the float64 trajectory."""
    n, steps, inf_step = 4096, 48, 20
    kw = dict(SCHED, t_max=40, growth_interval=16)
    rng = np.random.default_rng(7)
    p0 = rng.uniform(-1, 1, n).astype(f32)
    base, phase = np.where(np.arange(n) % 2 == 0, 3.0, -3.0), rng.uniform(0, 6.28, n)
    sf, si = new_state(2.0**10)
    sf64, si64 = [float(x) for x in host(sf)], [int(x) for x in host(si)]
    p, m, v = dev(p0), dev(np.zeros(n, f32)), dev(np.zeros(n, f32))
    copy_t = dev(R.bf16_rne(p0))
    s32 = dict(p=p0, m=np.zeros(n, f32), v=np.zeros(n, f32), copy=R.bf16_rne(p0))
    s64 = dict(p=p0.astype(f64), m=np.zeros(n), v=np.zeros(n))
    err = dict(p=np.zeros(n), m=np.zeros(n), v=np.zeros(n))
    for k in range(steps):
        target = (base + 0.25 * np.sin(0.7 * k + phase)).astype(f32)
        scale = float(host(sf)[R.SF_SCALE])
        assert scale == sf64[R.SF_SCALE]
        g32 = (f32(2.0) * (s32["p"] - target)) * f32(scale)
        g64 = 2.0 * (s64["p"] - target.astype(f64)) * scale
        e_g = 2.0 * scale * (err["p"] + R.U * np.abs(s32["p"].astype(f64) - target) * R.SLACK)
        if k == inf_step:
            g32[5] = np.inf
            si[R.SI_FOUND] = 1
            si64[R.SI_FOUND] = 1
        g = dev(g32)
        run_prologue(E, sf, si, kw)
        E.check(E.lib.ngp_adam_step_bf16(E.ptr(p), E.ptr(g), E.ptr(m), E.ptr(v), n, E.ptr(sf), E.ptr(si), B1, B2, 1e-15, E.ptr(copy_t),
                                         E.stream()), "ngp_adam_step_bf16")
        sf64, si64 = R.prologue64(sf64, si64, **kw)
        e = R.scalar_bounds(sf64, si64, kw["lr0"], kw["eta_min"], kw["t_max"], B2, k)
        sf_h, si_h = host(sf), host(si)
        R.assert_scalar_state(sf_h, si_h, sf64, si64, *e, what="coupled step %d" % k)
        skip = k == inf_step
        assert int(si_h[R.SI_SKIP]) == int(skip)
        c_dev, c64 = R.consts_from_state(sf_h, B1, B2, 1e-15), R.consts_from_state(sf64, B1, B2, 1e-15)
        want = R.adam_step32(s32["p"], g32, s32["m"], s32["v"], c_dev, skip=skip, copy=s32["copy"], copy_kind=1)
        got = dict(p=host(p), m=host(m), v=host(v), g=host(g), copy=host(copy_t, np.uint16))
        R.assert_step_exact(got, want, "coupled step %d" % k)
        if not skip:
            err = R.trajectory_error_step(dict(s32, g=g32), dict(s64, g=g64), c_dev, c64, err, e_g, rel_consts(sf64, e))
            p1, m1, v1, _ = R.adam64(s64["p"], g64, s64["m"], s64["v"], c64)
            s64 = dict(p=p1, m=m1, v=v1)
        s32 = dict(p=want["p"], m=want["m"], v=want["v"], copy=want["copy"])
    assert si64[R.SI_SKIPPED] == 1 and sf64[R.SF_SCALE] == 2.0**10 * 2 * 0.5 * 2 and sf64[R.SF_LR] == R.hyper(kw["eta_min"])
    worst = {}
    for name in ("p", "m", "v"):
        d = np.abs(got[name].astype(f64) - s64[name])
        assert (d <= err[name]).all(), (name, float(np.max(d / err[name])))
        worst[name] = float(np.max(d / err[name]))
    moved = float(np.abs(got["p"] - p0).mean())
    print("coupled run: worst error / accumulated bound %s; mean |p - p0| = %.3g, mean bound on p %.3g" % (worst, moved, err["p"].mean()))
    assert moved > 0.1 and err["p"].max() < 1e-3 * moved                    # the parameters travelled, the bound stayed far below that


# ------------------------------------------------------------------------------------------------ the inf / nan checks
BAD = (float("inf"), float("-inf"), float("nan"))
FINITE_EDGES = np.array([3.4028234663852886e38, -3.4028234663852886e38, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -5e-40], f32)


@pytest.mark.parametrize("blocks", [1, 15, 16, 17, 31, 33, 4096])
def test_finite_checks(E, blocks):
    """ngp_check_finite_multi and the fused check + prologue: one bad value at each lane of the first / last float4 of the first
    (largest), a middle and the last (smallest) tensor; grid sizes around the two-level arrival counter's group size."""
    rng = np.random.default_rng(blocks)
    sizes = [blocks * 256 * 4, 512, 8]
    ts = [dev(rng.standard_normal(n).astype(f32)) for n in sizes]
    for t in ts[:2]:                                                        # finite extremes beside the places a bad value will go
        t[4:4 + FINITE_EDGES.size].copy_(torch.from_numpy(FINITE_EDGES))
    ts[2][:4].copy_(torch.from_numpy(FINITE_EDGES[:4]))
    G = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])
    N = (ctypes.c_longlong * 3)(*sizes)
    found = torch.zeros(1, device="cuda")
    pair = torch.zeros(2, device="cuda")
    done = torch.zeros(17 * 32, dtype=torch.int32, device="cuda")
    sf, si = new_state()
    calls = [0]

    def both(expect, what):
        found.zero_()
        E.check(E.lib.ngp_check_finite_multi(3, G, N, E.ptr(found), E.stream()), "ngp_check_finite_multi")
        assert float(found) == expect, what
        k = calls[0] % 2
        calls[0] += 1
        flag, nxt = pair[k:k + 1], pair[1 - k:2 - k]
        nxt.fill_(1.0)                                                      # the flag of the step before, as GradScaler.update() left it
        before = host(si).copy()
        E.check(E.lib.ngp_adam_amp_check_prologue(3, G, N, E.ptr(flag), E.ptr(nxt), E.ptr(done), E.ptr(sf), E.ptr(si), E.ptr(None), 1e-3,
                                                  B1, B2, E.stream()), "ngp_adam_amp_check_prologue")
        after = host(si)
        assert float(flag) == expect and float(nxt) == 0.0 and not done.any(), what
        assert int(after[R.SI_SKIP]) == int(expect) and int(after[R.SI_SKIPPED]) == int(before[R.SI_SKIPPED]) + int(expect), what
        assert int(after[R.SI_OPT]) == int(before[R.SI_OPT]) + 1 - int(expect), what

    both(0.0, "all finite: +-FLT_MAX, -0.0, denormals")
    for ti, t in enumerate(ts):
        for base in (0, t.numel() - 4):
            for lane in range(4):
                bad = BAD[(ti + base + lane) % 3] if blocks != 16 else None
                for b in ((bad,) if bad is not None else BAD):              # every value at every place for one grid size
                    keep = float(t[base + lane])
                    t[base + lane] = b
                    both(1.0, (ti, base, lane, b))
                    t[base + lane] = keep
                    both(0.0, "restored")                                   # opposite verdicts in consecutive calls, flags alternating
    keep = ts[1][8:12].clone()
    ts[1][8:12] = torch.tensor([float("inf"), float("-inf"), 1.0, 2.0], device="cuda")      # inf - inf in one float4
    both(1.0, "+inf and -inf in one float4")
    ts[1][8:12] = keep
    both(0.0, "restored")


# ------------------------------------------------------------------------------------------------ MSE loss and gradient
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_mse_kernels(E, n):
    rng = np.random.default_rng(n)
    rgb, op, tg0 = rng.uniform(0, 1, (n, 3)).astype(f32), rng.uniform(0, 1, n).astype(f32), rng.uniform(0, 1, (n, 3)).astype(f32)
    for bg in (0.0, 1.0):
        tg = tg0.copy()
        c = min(n, 64)                                                      # rgb + b - target cancels to ~1e-7 on these rays
        tg[:c] = (rgb[:c].astype(f64) + (bg * (1 - op[:c].astype(f64)))[:, None] + 1e-7 * rng.choice([-1, 1], (c, 3))).astype(f32)
        d_rgb, d_op, d_tg = dev(rgb), dev(op), dev(tg)
        for scale in (1.0, 2.0**15):
            sf, _ = new_state(scale)
            loss64 = R.mse64(rgb, op, tg, bg, n, scale)[0]
            se32, g32, go32 = R.mse32(rgb, op, tg, bg, n, scale)
            what = "n=%d bg=%g scale=%g" % (n, bg, scale)
            g_rgb, g_op = torch.full((n, 3), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
            E.check(E.lib.ngp_mse_loss_grad(E.ptr(d_rgb), E.ptr(d_op), E.ptr(d_tg), bg, n, E.ptr(sf), E.ptr(g_rgb), E.ptr(g_op), E.stream()),
                    "ngp_mse_loss_grad")
            R.assert_bits_equal(host(g_rgb), g32, what + " g_rgb")
            R.assert_bits_equal(host(g_op), go32, what + " g_opacity")
            got = host(sf)
            bound = R.mse_loss_bound(rgb, op, tg, bg, n)
            assert abs(float(got[R.SF_LOSS]) - loss64) <= bound, (what, float(got[R.SF_LOSS]), loss64, bound)
            assert bound <= 2e-3 * loss64 or n <= 64, (what, bound, loss64)     # (n <= 64: every ray is a cancelling one)
            assert float(got[R.SF_SCALE]) == scale and not got[1:5].any()
            g_rgb.fill_(7.0); g_op.fill_(7.0)
            sq = torch.full((n,), 7.0, device="cuda")
            E.check(E.lib.ngp_mse_loss_grad_rays(E.ptr(d_rgb), E.ptr(d_op), E.ptr(d_tg), bg, n, E.ptr(sf), E.ptr(g_rgb), E.ptr(g_op),
                                                 E.ptr(sq), E.stream()), "ngp_mse_loss_grad_rays")
            R.assert_bits_equal(host(g_rgb), g32, what + " rays g_rgb")
            R.assert_bits_equal(host(g_op), go32, what + " rays g_opacity")
            R.assert_bits_equal(host(sq), se32, what + " rays sq_err")
            E.check(E.lib.ngp_mse_loss_grad_rays(E.ptr(d_rgb), E.ptr(d_op), E.ptr(d_tg), bg, n, E.ptr(sf), E.ptr(g_rgb), E.ptr(g_op),
                                                 E.ptr(None), E.stream()), "ngp_mse_loss_grad_rays (no sq_err)")
            R.assert_bits_equal(host(g_rgb), g32, what + " rays g_rgb, sq_err NULL")


# ------------------------------------------------------------------------------------------------ the slab sum
@pytest.mark.parametrize("n_parts", [1, 15, 16, 17, 255, 256, 257, 300])
def test_mlp_dw_reduce(E, n_parts):
    rng = np.random.default_rng(n_parts)
    extra = 3                                                               # slabs beyond n_parts hold a sentinel that must not leak
    mixed = (rng.standard_normal((n_parts + extra, R.NW)) * 10.0 ** rng.uniform(-6, 3, (n_parts + extra, R.NW))).astype(f32)
    dyadic = (rng.integers(-64, 65, (n_parts + extra, R.NW)) * 2.0**-6).astype(f32)
    for name, parts, dW0 in (("mixed", mixed, (rng.standard_normal(R.NW) * 100).astype(f32)),
                             ("dyadic", dyadic, rng.integers(-1000, 1000, R.NW).astype(f32))):
        parts[n_parts:] = np.nan
        d_parts, dW = dev(parts), dev(dW0)
        E.check(E.lib.ngp_mlp_dw_reduce(E.ptr(d_parts), n_parts, E.ptr(dW), E.stream()), "ngp_mlp_dw_reduce")
        s, a = R.dw_reduce64(parts, n_parts)
        want, got = dW0.astype(f64) + s, host(dW).astype(f64)
        assert np.isfinite(got).all(), name
        if name == "dyadic":
            assert np.array_equal(got, want), (n_parts, float(np.abs(got - want).max()))     # exact in any order
        else:
            B = R.dw_bound(n_parts, dW0, a)
            assert (np.abs(got - want) <= B).all(), (n_parts, float(np.max(np.abs(got - want) / B)))
            assert float(np.median(B / np.maximum(np.abs(want), 1e-30))) < 1e-3
        assert np.array_equal(host(d_parts)[:n_parts], parts[:n_parts])
