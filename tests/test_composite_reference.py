"""The float64 compositing model (tests/composite_reference.py) earns its place on the CPU before the kernels are judged against it:
against the reference project's executed outputs and its autodiff tape (the two fixtures under tests/golden/), against central finite
differences, against the oracle's closed form; then the yardstick itself -- the emulation of composite.hip's order (wave32) stays within
K * E32 on every case of the table, E32 is non-zero for every quantity, five deliberate defects are each caught on a named ray, and at
most 2 % of a set's rays are undecided."""
import os

import numpy as np
import pytest

import composite_reference as cr
from conftest import GOLDEN

F = np.float32
BGS = (None, 0.5, 1.0)
BWD_VARIANTS = [(gws, gop, bg) for gws in (False, True) for gop in (False, True) for bg in (0.0, 0.5)]
FUSED_VARIANTS = [(bg, ls) for bg in (0.0, 0.5, 1.0) for ls in (1.0, 2.0**14)]
SETS = ("lengths", "placed", "a_one", "hovering", "counts")


def _fixture_rays(g):
    ra = g["rays_a"]
    order = np.argsort(ra[:, 0])
    lst = [("ray%d" % r, g["sigmas"][s:s + c], g["deltas"][s:s + c], g["ts"][s:s + c], g["rgbs"][s:s + c]) for r, s, c in ra[order]]
    return cr.make_rays(lst), ra[order]


def _pad(rays, ra, flat):
    out = np.zeros((rays.n, rays.L) + flat.shape[1:], flat.dtype)
    for i, (_, s, c) in enumerate(ra):
        out[i, :c] = flat[s:s + c]
    return out


def test_forward_against_the_reference_projects_outputs():
    g = np.load(os.path.join(GOLDEN, "ref_composite_train.npz"))
    rays, ra = _fixture_rays(g)
    assert not cr.undecided(rays).any()
    e32, ref = cr.forward_e32(rays)
    assert np.array_equal(ref["M"], g["total_samples"][ra[:, 0]]) and ref["M"].max() < rays.N.max()     # early termination happened
    ws = np.nan_to_num(_pad(rays, ra, g["ws"]))             # (the reference leaves ws behind the termination unwritten)
    got = dict(M=ref["M"], w=ws, R=g["rgb"][ra[:, 0]], D=g["depth"][ra[:, 0]], O=g["opacity"][ra[:, 0]])
    v, _ = cr.judge_forward(rays, got, e32)                 # the reference's run is a float32 evaluation like any other
    print("reference project's forward / E32:", v)
    assert v.ok(), v.failures


def test_reverse_sweep_against_the_autodiff_fixture():
    g = np.load(os.path.join(GOLDEN, "ref_composite_train_grad.npz"))
    rays, ra = _fixture_rays(g)
    assert not cr.undecided(rays).any()
    idx = ra[:, 0]
    ref = cr.forward64(rays)
    ds, dc, S = cr.backward64(rays, ref, g["g_rgb"][idx], g["g_depth"][idx], g["g_opacity"][idx], _pad(rays, ra, g["g_ws"]))
    want_ds, want_dc = _pad(rays, ra, g["d_sigmas"]).astype(np.float64), _pad(rays, ra, g["d_rgbs"]).astype(np.float64)
    # the fixture is a float32 reverse tape over <= 120 samples: about three roundings of 2^-24 per step, each relative to the
    # magnitude of what it rounds -> 120 * 3 * 2^-24 = 2.1e-5 of the magnitude sum S at the very most
    assert rays.N.max() <= 120
    worst = np.max(np.abs(ds - want_ds)[S > 0] / S[S > 0])
    print("autodiff tape vs reverse sweep: max |d_sigma difference| / S = %.3g" % worst)
    assert np.all(np.abs(ds - want_ds) <= 120 * 3 * 2.0**-24 * S + cr.TINY)
    assert np.all(np.abs(dc - want_dc) <= 120 * 2.0**-24 * np.abs(g["g_rgb"][idx]).astype(np.float64)[:, None, :] * ref["T"][:, :, None] + cr.TINY)
    assert np.all(want_ds[np.arange(rays.L)[None, :] >= ref["M"][:, None]] == 0)


def _fd_rays():
    rng = np.random.default_rng(7)
    lst = []
    for n in (1, 5, 70, 70):
        dl = 0.02 + 0.06 * rng.random(n)
        sd = 0.005 + 0.025 * rng.random(n)                  # total optical depth <= 2.1: T >= 0.12, three decades above thr
        lst.append(("fd_N%d" % n, (sd / dl).astype(F), dl.astype(F), (0.3 + np.cumsum(dl)).astype(F), rng.random((n, 3)).astype(F)))
    return cr.make_rays(lst), np.array([1, 5, 70, 35])      # the last ray is truncated mid-way: M held fixed


def test_reverse_sweep_against_finite_differences():
    rays, M = _fd_rays()
    assert not cr.undecided(rays).any()
    g_rgb, g_dep, g_op, g_ws = (x.astype(np.float64) for x in cr.gradients(rays, 11))

    def loss(r):
        f = cr.forward64(r, force_M=M)
        return np.sum(g_rgb * f["R"], 1) + g_dep * f["D"] + g_op * f["O"] + np.sum(g_ws * f["w"], 1)
    ref = cr.forward64(rays, force_M=M)
    assert np.array_equal(cr.forward64(rays)["M"][:3], M[:3])
    ds, dc, S = cr.backward64(rays, ref, g_rgb, g_dep, g_op, g_ws)
    h = 1e-6
    worst = 0.0
    for j in range(70):
        for what in ("sigma", "rgb0"):
            lo, hi = _perturbed(rays, what, j, -h), _perturbed(rays, what, j, +h)
            fd = (loss(hi) - loss(lo)) / (2 * h)
            live = j < M
            if what == "sigma":
                err, scale = np.abs(fd - ds[:, j]), S[:, j]
            else:
                err, scale = np.abs(fd - dc[:, j, 0]), np.abs(g_rgb[:, 0]) * ref["T"][:, j]
            assert np.all(err[~live] == 0) and np.all(err[live] <= 1e-6 * scale[live]), (what, j, err, scale)
            worst = max(worst, float(np.max(err[live] / scale[live], initial=0.0)))
    print("finite differences vs reverse sweep: worst relative to S = %.3g" % worst)


class _Rays64(cr.Rays):
    """The same batch with float64 storage, so that a 1e-6 step is not lost to float32 rounding."""

    def __init__(self, src, sigma, rgb):
        self.sigma, self.delta, self.t, self.rgb = sigma, src.delta, src.t, rgb
        self.N, self.names, self.n, self.L, self.valid = src.N, src.names, src.n, src.L, src.valid


def _perturbed(rays, what, j, h):
    sigma, rgb = rays.sigma.astype(np.float64), rays.rgb.astype(np.float64)
    if what == "sigma":
        sigma[:, j] += h
    else:
        rgb[:, j, 0] += h
    return _Rays64(rays, sigma, rgb)


def test_reverse_sweep_against_the_oracle(oracle):
    """Ties SURVEY A.5's closed form (the oracle evaluates it in double on float32 forward values) to the adjoint form once."""
    rays = cr.case_table()["hovering"].take(np.arange(40))
    lay = cr.Layout(rays, 5)
    rays_a = lay.rays_a.copy()
    rays_a[:, 0] = np.arange(rays.n)                        # (the oracle sizes its per-ray outputs by the row count)
    g_rgb, g_dep, g_op, g_ws = cr.gradients(rays, 12)
    ds, dc = oracle.composite_train_bwd(g_op, g_dep, g_rgb, lay.flat(g_ws), lay.sigmas, lay.rgbs, lay.deltas, lay.ts, rays_a, cr.THR)
    tot = oracle.composite_train_fwd(lay.sigmas, lay.rgbs, lay.deltas, lay.ts, rays_a, cr.THR)[0]
    e32 = cr.backward_e32(rays, g_rgb, g_dep, g_op, g_ws)
    v = cr.Verdict()
    cr.judge_counts(v, rays, tot)
    cr.judge_backward(rays, lay.padded(ds), lay.padded(dc), tot, e32, g_rgb, g_dep, g_op, g_ws, v=v)
    print("oracle closed form / E32:", v)
    assert v.ok(), v.failures


def _sets(half):
    t = cr.case_table()
    return {k: (r.with_rgb(r.rgb.astype(np.float16).astype(F)) if half else r) for k, r in t.items()}


def _wave32_verdicts(name, rays, alter=""):
    """Every judged quantity of every variant for one set, by the emulation of the kernels' order: [(what, Verdict, e32)]."""
    out = []
    for bg in BGS:
        e32, _ = cr.forward_e32(rays, bg)
        got = cr.wave32_forward(rays, alter=alter)
        if bg is not None:
            got["rgb_out"] = got["R"] + (F(bg) * (F(1) - got["O"]))[:, None]
        out.append(("forward bg=%s" % bg, cr.judge_forward(rays, got, e32, bg=bg)[0], e32))
    fwd = cr.wave32_forward(rays, alter=alter)
    g_rgb, g_dep, g_op, g_ws = cr.gradients(rays, 21)
    for gws, gop, bg in BWD_VARIANTS:
        a = (g_rgb, g_dep if gop else None, g_op if gop else None, g_ws if gws else None)
        e32 = cr.backward_e32(rays, *a, bg=bg)
        ds, dc = cr.wave32_backward(rays, fwd, *a, bg=bg, alter=alter)
        out.append(("backward g_ws=%d g_op/g_depth=%d bg=%g" % (gws, gop, bg), cr.judge_backward(rays, ds, dc, fwd["M"], e32, *a, bg=bg), e32))
    for bg, ls in FUSED_VARIANTS:
        tgt = cr.targets(rays, bg, 31)
        e32 = cr.fused_e32(rays, tgt, bg, ls, rays.n)
        got = cr.wave32_fused(rays, tgt, bg, ls, rays.n, alter=alter)
        out.append(("fused bg=%g loss_scale=%g" % (bg, ls), cr.judge_fused(rays, got, tgt, bg, ls, rays.n, e32), e32))
    return out


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", SETS)
def test_bound_is_meetable_and_not_vacuous(name, half):
    rays = _sets(half)[name]
    worst = {}
    for what, v, e32 in _wave32_verdicts(name, rays):
        assert all(e > 0 for e in e32.values()), (what, e32)
        assert v.ok(), (what, v.failures)
        for q, r in v.ratios.items():
            worst[q] = max(worst.get(q, 0.0), r)
    print("wave32 / E32 on %s (%s): %s" % (name, "f16" if half else "f32", ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= cr.K


@pytest.mark.parametrize("alter", sorted(cr.ALTERATIONS))
def test_bound_has_teeth(alter):
    """Each deliberate defect of the emulated kernel breaks the bound, the exact count or the exact-zero condition on a named ray."""
    caught = []
    for name in SETS:
        for what, v, _ in _wave32_verdicts(name, _sets(False)[name], alter=alter):
            caught += ["%s / %s / %s" % (name, what, f) for f in v.failures[:1]]
        if caught:
            break
    print("alteration (%s) %s: caught %d times, first: %s" % (alter, cr.ALTERATIONS[alter], len(caught), caught[:1]))
    assert caught, "alteration (%s) passes every case: the table is too weak" % alter


def test_decidability_share():
    for name, rays in cr.case_table().items():
        und = cr.undecided(rays)
        print("%s: %d of %d rays undecided: %s" % (name, und.sum(), rays.n, [rays.names[i] for i in np.flatnonzero(und)]))
        assert und.mean() <= 0.02, name
        if name in ("placed", "a_one"):
            assert not und.any()                            # decided by construction
        lo, hi = cr.count_bounds(rays)
        M = cr.forward64(rays)["M"]
        assert np.all((lo == M) & (hi == M) | und) and np.all((lo <= M) & (M <= hi))
        wide = (hi - lo > 2) | (M - lo > 1) | (hi - M > 1)
        assert all(rays.names[i].startswith("plateau") for i in np.flatnonzero(wide))
    assert cr.undecided(cr.case_table()["hovering"]).sum() >= 2   # the undecided class is present
