"""The numpy reference of the sphere-tracing contract (tests/sdf_trace_reference.py) against answers known by hand, against itself
(serial float32 vs float64 on decided rays) and against the cap on undecided rays -- no GPU."""
import numpy as np
import pytest

import sdf_trace_reference as R


@pytest.fixture(scope="module")
def small_levels(hip_lib):
    from ngp_hip import ops
    lv = ops.make_levels(2**12, 4, 8, 64, 2)
    return ops.levels_to_numpy(lv), lv.begin_fast_hash_level, lv.total_entries


@pytest.fixture(scope="module")
def cases(small_levels):
    from ngp_hip import ops
    levels, bfhl, entries = small_levels
    small = R.make_model(levels, bfhl, entries, 16, 1, 0.5, seed=3)
    wide = R.make_model(levels, bfhl, entries, 16, 1, 1.0, seed=3)
    lv = ops.make_levels(2**19, 16, 16, 2048, 2)
    default = R.default_arch_case(ops.levels_to_numpy(lv), lv.begin_fast_hash_level, lv.total_entries)
    return R.case_table(small) + [c for c in R.case_table(wide) if c.name in ("threshold_shell_n65", "crossing_refine8")] + [default]


def plane_model(levels, bfhl, entries):
    """Zero table, depth 1, every hidden pre-activation >= 0.5 on the box (Softplus is the identity there: 100 h > 20): neuron 0 is
    1 + z, the others are the constant 1 with output weight 0; b_out = -1.25.  f(x) = z - 0.25, exactly, in float32 as in float64."""
    W0 = np.zeros((16, 3 + 2 * len(levels[0])), np.float32)
    W0[0, 2] = 1.0
    w_out = np.zeros((1, 16), np.float32)
    w_out[0, 0] = 1.0
    layers = [(W0, np.ones(16, np.float32)), (w_out, np.full(1, -1.25, np.float32))]
    return R.Model(levels, bfhl, np.zeros((entries, 2), np.float32), layers, 0.5)


# the ray o = (0, 0, 1), d = (0, 1/8, -1/2) enters the box at t = 1 (z = 0.5) and leaves it at t = 3; along it f = 0.75 - t / 2.
PLANE_O, PLANE_D = np.array([[0.0, 0.0, 1.0]], np.float32), np.array([[0.0, 0.125, -0.5]], np.float32)


@pytest.mark.parametrize("T", [np.float64, np.float32])
def test_plane_threshold_path_is_the_geometric_recurrence(small_levels, T):
    """step_scale = 1, min_step = 0: f_k = 2^-(k+2), t_k = 1 + (1 - 2^-k) / 2, every value a short binary fraction: exact in float32.
    The first f_k <= eps = 1e-3 is f_8 = 2^-10: HIT at t_8 after 9 evaluations."""
    m = plane_model(*small_levels)
    grid = R.Grid(np.full(32**3 // 8, 255, np.uint8), 0.5, 32)
    r = R.trace(m, grid, PLANE_O, PLANE_D, T, eps=1e-3, step_scale=1.0, min_step=0.0, n_refine=8, max_evals=256)
    assert r["status"][0] == R.HIT and r["n_eval"][0] == 9
    assert r["t"][0] == 1.0 + 0.5 * (1.0 - 2.0**-8) and r["f_last"][0] == 2.0**-10
    assert np.array_equal(r["xyz"][0], [0.0, 0.125 * r["t"][0], 1.0 - 0.5 * r["t"][0]])
    r = R.trace(m, grid, PLANE_O, PLANE_D, T, eps=1e-3, step_scale=1.0, min_step=0.0, n_refine=8, max_evals=5)
    assert r["status"][0] == R.ABANDONED and r["n_eval"][0] == 5 and r["t"][0] == 1.0 + 0.5 * (1.0 - 2.0**-5)


@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("n_refine", [0, 1, 8])
def test_plane_crossing_path_returns_the_root(small_levels, T, n_refine):
    """eps = 0, min_step = dt_min: eight geometric steps (f_0..f_7 > dt_min), then steps of dt_min: f_8 = 2^-10 and f_9 = f_8 - dt_min / 2
    are positive, f_10 is negative: 11 evaluations, the crossing is bracketed, n_refine bisections follow, and the interpolation of a
    linear f returns its root t = 1.5 whatever the bracket."""
    m = plane_model(*small_levels)
    grid = R.Grid(np.full(32**3 // 8, 255, np.uint8), 0.5, 32)
    r = R.trace(m, grid, PLANE_O, PLANE_D, T, eps=0.0, step_scale=1.0, min_step=float(R.DT_MIN), n_refine=n_refine, max_evals=256)
    assert r["status"][0] == R.HIT and r["n_eval"][0] == 11 + n_refine
    assert abs(float(r["t"][0]) - 1.5) <= (4 * 2.0**-24 * 1.5 if T == np.float32 else 1e-15)


def test_fma_is_one_rounding():
    """against exact rational arithmetic, on products that a double-rounded a * b + c gets wrong"""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.uniform(-1e-6, 1e-6, 4000))).astype(np.float32)      # heavy cancellation
    c[::2] = rng.standard_normal(2000).astype(np.float32)
    got = R.fma(a, b, c, np.float32)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                                  # float(Fraction) rounds once to 53 bits; compare by distance
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))
        assert abs(Fraction(float(got[i])) - exact) == abs(Fraction(float(best)) - exact)


def test_field_float32_tracks_float64(small_levels):
    """the serial float32 field stays within a few float32 roundings of the float64 one, inside the box, on faces and outside"""
    levels, bfhl, entries = small_levels
    m = R.make_model(levels, bfhl, entries, 16, 1, 0.5, seed=3)
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-0.5, 0.5, (300, 3)), rng.choice([-0.5, 0.5, 0.0], (50, 3)), rng.uniform(-2, 2, (50, 3))]).astype(np.float32)
    f64, f32 = R.field(m, x, np.float64), R.field(m, x, np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - f64).max() < 64 * 2.0**-24 * max(1.0, np.abs(f64).max())


def test_serial_float32_agrees_on_decided_rays(cases):
    for c in cases:
        r64, r32, dec = c.ref()
        assert np.array_equal(r64["status"][dec], r32["status"][dec]) and np.array_equal(r64["n_eval"][dec], r32["n_eval"][dec]), c.name
        R.invariants(c, {k: r32[k] for k in ("status", "t", "xyz", "n_eval", "f_last")})
        if not c.only_invariants:
            R.judge(c, {k: r32[k] for k in ("status", "t", "xyz", "n_eval", "f_last")})


def test_undecided_caps(cases):
    for c in cases:
        if not c.only_invariants:
            assert c.undecided_fraction() <= R.MAX_UNDECIDED, "%s: %.4f of the rays undecided" % (c.name, c.undecided_fraction())


def test_named_sets_reach_every_branch(cases):
    by = {c.name: c.ref()[0] for c in cases if c.model.scale == 0.5}
    st = lambda name: np.bincount(by[name]["status"], minlength=4)
    assert st("threshold_shell_n1153")[R.HIT] > 100 and st("crossing_refine8")[R.HIT] > 50
    assert (by["crossing_refine8"]["n_eval"] >= 8 + 2)[by["crossing_refine8"]["status"] == R.HIT].any()
    assert st("inside_ones")[R.INSIDE] == 130 and st("abandoned_max3")[R.ABANDONED] > 20
    assert (by["all_zeros"]["status"] == R.MISS).all() and (by["all_zeros"]["n_eval"] == 0).all()
    assert ((by["miss_slab"]["status"] == R.MISS) & (by["miss_slab"]["n_eval"] == 0)).sum() > 50          # behind the box, or beside it
    past = by["miss_past_surface"]
    assert ((past["status"] == R.MISS) & (past["n_eval"] > 0)).sum() > 20
