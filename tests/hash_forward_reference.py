"""Serial numpy restatement of the hash-grid encoder's FORWARD gather -- the CPU reference of tests/test_hash_forward_reference.py and
tests/test_gpu_hash_forward_exact.py.  numpy only: the corner rule (entries, weights, saturation) is the one
tests/hash_input_grad_reference.py already restates; what is added here is the blend, as the kernels are meant to evaluate it:

    enc[l, f] = (((0 + w_0 T_0) + w_1 T_1) + ... + w_7 T_7)        corners 0 .. 7 in order, every product and every sum rounded

`forward32` does that in the arithmetic of each table kind; `forward64` (hash_input_grad_reference) sums the same float32 weights in
float64, and `forward_bound` is the distance the two may have.  The GPU kernels are held to `forward32` bit for bit.

Edge rules this restatement fixes (csrc/hash_common.h: cell_frac, level_index; ngp_device.h: f2u_sat):
  * the cell is floor(x * scale + 0.5) converted to uint32 with saturation: NaN and negatives give 0, 2^32 and above give 0xffffffff,
    and the far corner of cell 0xffffffff wraps to grid point 0;
  * the fraction is pos - float(cell), so a NaN coordinate has cell 0 and a NaN fraction, hence NaN weights on all eight corners;
  * every corner entry is the raw 32-bit index modulo the level's size, for any input;
  * the half form rounds float(cell) through float16 before the subtract (cells above 2048 lose bits, cells above 65504 become inf)."""
import numpy as np

from hash_input_grad_reference import cell_frac, corners, forward64, level_table  # noqa: F401  (re-exported for the tests)

f16, f32, f64 = np.float16, np.float32, np.float64
KINDS = ("f32", "bf16", "f16")
FILL = f32(-7.0)            # what the GPU tests pre-fill every output buffer with
_CHUNK = 32768              # rows per corners() call: bounds the [rows, L, 8] temporaries


def bf16_bits(a):
    """float32 -> bf16 bit patterns (uint16), round to nearest even.  Finite inputs only."""
    u = np.ascontiguousarray(a, dtype=f32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def widen(table, kind):
    """The table as float32 values, exactly: f32 as is, bf16 from its uint16 bit patterns, f16 from float16."""
    if kind == "bf16":
        t = np.ascontiguousarray(table)
        assert t.dtype == np.uint16
        return (t.astype(np.uint32) << np.uint32(16)).view(f32)
    if kind == "f16":
        assert np.asarray(table).dtype == f16
        return np.asarray(table).astype(f32)
    assert kind == "f32" and np.asarray(table).dtype == f32
    return np.asarray(table)


def blend(idx, w, T, kind, order=range(8), single_rounding=False):
    """One chunk: idx, w [m, L, 8] from corners(), T [entries, F] float32 -> [m, L * F].  `order` and `single_rounding` exist for the
    altered restatements of the CPU tests only."""
    m, L, _ = idx.shape
    F = T.shape[1]
    out = np.empty((m, L * F), dtype=f16 if kind == "f16" else f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for l in range(L):
            acc = np.zeros((m, F), dtype=out.dtype)                     # +0
            for c in order:
                if single_rounding:                                      # the exact product rounded once (what v_fma_mixlo_f16 gives)
                    term = (w[:, l, c, None].astype(f64) * T[idx[:, l, c]].astype(f64)).astype(f16)
                else:
                    term = w[:, l, c, None] * T[idx[:, l, c]]            # one float32 product
                    assert term.dtype == f32
                    if kind == "f16":
                        term = term.astype(f16)                          # ... then the cast: the second rounding
                acc = acc + term                                         # one rounded sum in the accumulator's type
                assert acc.dtype == out.dtype
            out[:, l * F:(l + 1) * F] = acc
    return out


def forward32(x, table, lv, kind="f32"):
    """enc [n, L * F]: float32 for the f32 and bf16 kinds, float16 for f16 (the `_ex` form widens it exactly to float32).

    f32   acc = acc + w * T, both float32 operations, acc starting from +0.
    bf16  the same on the bf16 table widened exactly to float32.
    f16   term = f16(f32(w * f32(T))); acc = f16(acc + term) from +0.  numpy evaluates a float16 sum in float32 and rounds it to
          float16; float32 carries 24 >= 2 * 11 + 2 bits, so that double rounding equals the single correctly rounded float16 sum."""
    assert kind in KINDS
    t = level_table(lv)
    x = np.asarray(x, dtype=f32).reshape(-1, 3)
    T = widen(table, kind).reshape(-1, t["F"])
    out = np.empty((x.shape[0], t["L"] * t["F"]), dtype=f16 if kind == "f16" else f32)
    for a in range(0, x.shape[0], _CHUNK):
        idx, w = corners(x[a:a + _CHUNK], lv, half=(kind == "f16"))
        out[a:a + _CHUNK] = blend(idx, w, T, kind)
    return out


def forward_bound(mag, kind):
    """Largest |forward32 - forward64| an element may have; `mag` is forward64's sum_c |w_c T_c| of that element.

    Write u for the unit roundoff of the accumulator (2^-24 in float32, 2^-11 in float16).  Each of the 8 products is rounded:
    |term_c - w_c T_c| <= u |w_c T_c|, together u * mag.  The first sum 0 + term_0 is exact; each of the other 7 rounds a partial sum
    whose magnitude is at most the sum of the |term_c|, itself at most mag (1 + u): 7 u mag (1 + u)^7.  First order: (1 + 7) u mag;
    the factor (1 + 2^-10) [f32] or (1 + 2^-8) [f16] is the slack for the second-order terms, and in float16 for the float32 rounding
    of the product before its cast (2^-24 relative, far inside 8 * 2^-11 * 2^-8).
    In float16 a product may round into the denormal range, where the error is absolute: at most half the denormal spacing 2^-24 per
    operation, 8 * 2^-25 in all (float16 sums of float16 values are exact there).  The float32 kinds need no such floor at these
    magnitudes: a product below 2^-126 does not occur with normal tables and weights above 2^-100.
    The bf16 kind is the f32 arithmetic on the widened table, so it has the f32 bound against forward64 on that widened table."""
    mag = np.asarray(mag, dtype=f64)
    if kind == "f16":
        return 8 * 2.0**-11 * mag * (1 + 2.0**-8) + 8 * 2.0**-25
    return 8 * 2.0**-24 * mag * (1 + 2.0**-10)


def normalise(x, lo, hi):
    """(x - lo) / (hi - lo): the two float32 operations of the fused position normalisation.  No clipping."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        return (np.asarray(x, dtype=f32) - f32(lo)) / (f32(hi) - f32(lo))


def denormalise(x, lo, hi):
    """Some float32 positions whose `normalise` lands near x: the inputs of the normalisation cases (exactness is not needed: the
    reference of such a case is forward32(normalise(raw)))."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.asarray(x, dtype=f32) * (f32(hi) - f32(lo)) + f32(lo)


def to_pair_major(enc, n_max, fill=FILL):
    """Natural rows [n, 32] -> the pair-major planes [8][n_max][4]: plane p holds level p in floats 0-1 and level 15 - p in floats
    2-3.  Rows [n, n_max) of every plane hold `fill`."""
    enc = np.asarray(enc)
    n = enc.shape[0]
    assert enc.shape[1] == 32 and n <= n_max
    out = np.full((8, n_max, 4), fill, dtype=enc.dtype)
    for p in range(8):
        out[p, :n, 0:2] = enc[:, 2 * p:2 * p + 2]
        out[p, :n, 2:4] = enc[:, 2 * (15 - p):2 * (15 - p) + 2]
    return out


def from_pair_major(planes, n):
    """The first n rows of pair-major planes [8][n_max][4] as natural rows [n, 32]."""
    planes = np.asarray(planes)
    assert planes.shape[0] == 8 and planes.shape[2] == 4 and n <= planes.shape[1]
    out = np.empty((n, 32), dtype=planes.dtype)
    for p in range(8):
        out[:, 2 * p:2 * p + 2] = planes[p, :n, 0:2]
        out[:, 2 * (15 - p):2 * (15 - p) + 2] = planes[p, :n, 2:4]
    return out


def same_bits(got, want):
    """Bit equality where `want` is not NaN, NaN where it is (a NaN's sign and payload are not part of the contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    bits = np.uint16 if got.dtype == f16 else np.uint32
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(bits)[~nan], want.view(bits)[~nan]))


# ---------------------------------------------------------------------------------------------------------------- the named inputs
SHAPES = {
    "c2": (2**19, 16, 16, 1024, 2),
    "c3": (2**19, 16, 16, 4096, 2),
    "mod": (3 * 2**17, 16, 16, 1024, 2),        # hashed levels of 393 216 entries: the real modulo
    "g5f1": (2**14, 5, 8, 300, 1), "g5f2": (2**14, 5, 8, 300, 2), "g5f4": (2**14, 5, 8, 300, 4), "g5f8": (2**14, 5, 8, 300, 8),
}
N_TRIPS2, N_TRIPS3 = 768 * 128 + 129, 2 * 768 * 128 + 129      # two and three trips of the persistent grid of 768 tiles
N_LIST = 200000
NORMS = ((-0.5, 0.5), (-8.0, 8.0), (-0.3, 0.3), (-1.7, 2.9), (0.0, 2.0**-63), (0.0, 2.0**64))
# name: (level table, table kind, rows, normalisation of the positions or None)
CASES = {
    "c2_f32": ("c2", "f32", N_TRIPS3, None), "c3_f32": ("c3", "f32", N_TRIPS3, None), "mod_f32": ("mod", "f32", N_TRIPS2, None),
    "c2_bf16": ("c2", "bf16", N_TRIPS2, None), "g5_bf16": ("g5f2", "bf16", 4097, None),
    "c2_f16": ("c2", "f16", N_TRIPS3, None), "g5_f16": ("g5f2", "f16", 65553, None),
    "c3_f16": ("c3", "f16", N_TRIPS2, None),      # cells up to 4096: above 2048 the half form's float16 cell loses bits inside the box
    "list_f32": ("c3", "f32", N_LIST, (-1.7, 2.9)), "list_bf16": ("c3", "bf16", N_LIST, (-8.0, 8.0)),
    "g5f1_f32": ("g5f1", "f32", 209800, None), "g5f2_f32": ("g5f2", "f32", 4097, None), "g5f4_f32": ("g5f4", "f32", 4097, None),
    "g5f8_f32": ("g5f8", "f32", 4097, None),
}
for _k, _lohi in enumerate(NORMS):
    CASES["norm%d_f32" % _k] = ("c2", "f32", 4097, _lohi)
    CASES["norm%d_f16" % _k] = ("c2", "f16", 4097, _lohi)
N_EDGE = 17
_cache = {}


def positions(n, top_scale, seed=11):
    """[n, 3] float32, uniform in the unit cube; the first N_EDGE rows are the fixed edges: the box corners, a face, a point next to
    the upper and lower faces, one less than an ulp inside a cell face of the finest level, four points outside the box (two of
    them far enough to saturate the cell), one NaN and one +inf coordinate."""
    x = np.random.default_rng(seed).random((max(n, N_EDGE), 3), dtype=f32)
    top = f32(top_scale)
    face = np.nextafter(f32((np.floor(top / f32(2)) - f32(0.5)) / top), f32(0))      # x * top + 0.5 just below a grid point
    x[:N_EDGE] = [[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [0.5, 0.25, 1.0],
                  [0.999999, 1e-7, 0.5], [face, 0.3, face], [-0.25, 1.5, 0.5], [1.25, -0.25, 3.0], [1e30, 0.5, 0.5],
                  [-1e30, 0.2, 3.0], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5]]
    return x[:n]


def make_table(n_values, kind, seed):
    """Signed normal values in the table's storage type: float32, bf16 bit patterns (uint16) or float16 (scaled by 0.5: nothing
    overflows float16 in an 8-term sum of weights that add up to 1)."""
    t = np.random.default_rng(seed).standard_normal(n_values).astype(f32)
    if kind == "bf16":
        return bf16_bits(t)
    if kind == "f16":
        return (t * f32(0.5)).astype(f16)
    return t


def case(name, make_levels):
    """The named case: dict(lv, kind, x [the kernel's input], xn [the normalised positions the reference encodes], norm, table, and
    lazily `ref` = forward32 over all rows, through `reference`).  `make_levels(max_params, levels, base_res, max_res, features)`
    builds the level struct (the project's or the oracle's: the CPU tests hold them equal).  Generated once, cached, never modified."""
    if name in _cache:
        return _cache[name]
    shape, kind, n, norm = CASES[name]
    lv = make_levels(*SHAPES[shape])
    xn = positions(n, lv.scale[lv.n_levels - 1])
    x = xn
    if norm is not None:
        x = denormalise(xn, *norm)
        xn = normalise(x, *norm)
    table = make_table(int(lv.total_entries) * int(lv.n_features), kind, seed=sum(map(ord, shape + kind)))
    for a in (x, xn, table):
        a.setflags(write=False)
    _cache[name] = dict(name=name, lv=lv, kind=kind, x=x, xn=xn, norm=norm, table=table, n=n)
    return _cache[name]


def reference(c):
    """forward32 over all rows of a case, computed once."""
    if "ref" not in c:
        c["ref"] = forward32(c["xn"], c["table"], c["lv"], c["kind"])
        c["ref"].setflags(write=False)
    return c["ref"]
