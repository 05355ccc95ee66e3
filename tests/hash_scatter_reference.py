"""Float64 reference of the hash encoder's scatter-add (the backward with respect to the table), term by term -- the CPU side of
tests/test_hash_scatter_reference.py and tests/test_gpu_hash_scatter_sliced_exact.py, which hold the LDS-sliced kernels of
csrc/hash_bwd_lds.hip to it.  Built on hash_input_grad_reference.py (level_table, cell_frac, corners): corner entries and forward
weights are the forward's bit for bit.

Terms.  Sample i with a gradient row that is not exactly zero adds, to element (entry of corner c, feature f) of level l,

    p = fl32(w_c * g_f)                      f32 form: w_c the forward's float32 weight ((1 * wx) * wy) * wz, g_f the float32 gradient
    p = fl16(fl32(w_c * fl16(g_f)))          half2 form: the cell goes through f16 before the subtract (corners(half=True))

which is the product accumulate<KIND> forms (the library is built with -ffp-contract=off).  Per element that receives a nonzero
term this module gives  sum = the float64 sum of its terms,  S = sum |p|,  k = the number of nonzero terms,  k_sub = the number of
terms with 0 < |p| < 2^-14 (f16 subnormals; meaningful for the half2 form).  Elements without a nonzero term are not listed: the
kernels must leave them alone, bit for bit.

`sum` is accumulated serially in float64 (np.bincount / np.cumsum), so |sum - exact| <= (k - 1) 2^-53 S; the bound below carries
k 2^-52 S for the float64 accumulation of both sides together.  test_hash_scatter_reference.py compares it with math.fsum.

Bound.  The kernel sums the products in float64 in LDS and rounds once when it flushes.  With u = 2^-24 (f32 form) or 2^-11 (half2),
nrep[l] and the merge bit of level l from ngp_hash_bwd_sliced_plan, delta = 1 on merge levels (a row pre-sum is at most 15 float32
adds of products whose magnitudes sum to at most S), for one element onto a table filled with `fill`:

    |got - fill - sum| <= u |sum| (1 + 2^-10)                       one rounding at the flush (half2: f64 -> f32 -> f16)
                        + k 2^-52 S                                 the f64 accumulation, either side
                        + delta 15 2^-24 S                          f32 run pre-sums
                        + [nrep > 1] (nrep + 1) u (|fill| + S)      replicas meeting in float / packed-f16 atomics
                        + [fill != 0] u (|fill| + |sum|)            the add onto the table
                        + k_sub 2^-24 + tiny                        half2 only; tiny = 2^-149 (f32 form), 2^-25 (half2)

Nothing in it is measured.  The oracle (oracle/ngp_oracle.c: ora_hash_bwd_f32 / _f16) accumulates the same products in float64 in
sample order and rounds once to float32 -- it is NOT a serial float32 sum --, so its own distance from `sum` is bounded by the
first two lines with u = 2^-24 (oracle_bound); a serial float32 sum would be allowed k 2^-24 S, which is far wider.

Inputs.  The builders below make the smallest inputs that reach the owner loop's (bwd_task) rarely run parts: piece compaction
with more than 64 non-empty 8-sample pieces per super-chunk, a hit queue that fills by 64 per round and drains at exactly 128, the
ring's wrap-around, run pre-sums over whole rows and across row / batch / super-chunk boundaries, replicas with an empty sample
range.  Each builder asserts the structure it promises from THIS module's cells, never from a kernel."""
import ctypes

import numpy as np

import hash_input_grad_reference as ref

f16, f32, f64 = np.float16, np.float32, np.float64

TABLES = {"C2": (2**19, 16, 16, 1024, 2), "C3": (2**19, 16, 16, 4096, 2), "real_modulo": (3 * 2**17, 16, 16, 1024, 2),
          "fine": (2**19, 16, 16, 16384, 2)}
SLICE_LOG2 = 13                                    # BW_SLICE_LOG2: a slice is 8192 entries
BOX = 2.0**-16                                     # side of the box the samples of one cell are drawn in
MARGIN = 0.05                                      # ... and their least distance from every cell face, in cells
N_ONE_CELL, N_PIECES = 9000, 4200
PREFIXES = (1, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 9000)
ONE_CELL_ZERO_ROWS = (5, 100)                      # inside the run: exactly zero gradient rows
SUBNORMAL_F16 = 2.0**-14


class Scatter:
    """entries: sorted flat element indices (entry * F + feature) with at least one nonzero term; sum, S, k, k_sub per element."""

    def __init__(self, entries, total, S, k, k_sub):
        self.entries, self.sum, self.S, self.k, self.k_sub = entries, total, S, k, k_sub


# ------------------------------------------------------------------------------------------------ terms and their sums
def terms(x, g, lv, half=False, live_idx=None, count=None):
    """flat [n, L, 8, F] int64 element indices and p [n, L, 8, F] float32 terms (zero where the sample's row of that level is zero).
    live_idx / count: row j of g belongs to position x[live_idx[j]], and only the first `count` rows exist."""
    t = ref.level_table(lv)
    L, F = t["L"], t["F"]
    g = np.asarray(g, dtype=f32)
    n = g.shape[0] if count is None else min(g.shape[0], int(count))
    x = np.asarray(x, dtype=f32)
    xs = x[:n] if live_idx is None else x[np.asarray(live_idx, dtype=np.int64)[:n]]
    gs = g[:n].reshape(n, L, 1, F)
    if half:
        gs = gs.astype(f16).astype(f32)
    idx, w = ref.corners(xs, lv, half)
    p = w[..., None] * gs
    assert p.dtype == f32
    if half:
        p = p.astype(f16).astype(f32)
    p = np.where(np.any(gs != 0, axis=3, keepdims=True), p, f32(0))
    flat = idx.astype(np.int64)[..., None] * F + np.arange(F, dtype=np.int64)
    return flat, p


def scatter(x, g, lv, half=False, live_idx=None, count=None):
    """The Scatter of an input."""
    flat, p = terms(x, g, lv, half, live_idx, count)
    flat, p = flat.reshape(-1), p.reshape(-1)
    on = p != 0
    flat, p = flat[on], p[on].astype(f64)
    entries, inv = np.unique(flat, return_inverse=True)
    m = entries.size
    return Scatter(entries, np.bincount(inv, weights=p, minlength=m), np.bincount(inv, weights=np.abs(p), minlength=m),
                   np.bincount(inv, minlength=m).astype(np.int64),
                   np.bincount(inv, weights=(np.abs(p) < SUBNORMAL_F16).astype(f64), minlength=m).astype(np.int64))


def prefix_scatters(x, g, lv, prefixes, half=False):
    """{n: Scatter of the first n samples} for an input whose samples all share their entries (asserted): cumulative sums."""
    flat, p = terms(x, g, lv, half)
    n = flat.shape[0]
    assert np.all(flat == flat[0]), "the samples do not share their entries"
    cols = flat[0].reshape(-1)
    P = p.reshape(n, -1).astype(f64)
    entries, inv = np.unique(cols, return_inverse=True)
    T, A = np.zeros((n, entries.size)), np.zeros((n, entries.size))
    K, KS = np.zeros((n, entries.size), dtype=np.int64), np.zeros((n, entries.size), dtype=np.int64)
    for j in range(cols.size):                     # (two corners of a hashed level may name one entry)
        T[:, inv[j]] += P[:, j]
        A[:, inv[j]] += np.abs(P[:, j])
        K[:, inv[j]] += P[:, j] != 0
        KS[:, inv[j]] += (P[:, j] != 0) & (np.abs(P[:, j]) < SUBNORMAL_F16)
    T, A, K, KS = np.cumsum(T, axis=0), np.cumsum(A, axis=0), np.cumsum(K, axis=0), np.cumsum(KS, axis=0)
    out = {}
    for m in prefixes:
        on = K[m - 1] > 0
        out[m] = Scatter(entries[on], T[m - 1][on], A[m - 1][on], K[m - 1][on], KS[m - 1][on])
    return out


def level_of(entries, lv):
    """Level of each flat element index."""
    t = ref.level_table(lv)
    ends = np.array([t["offset"][l] + t["size"][l] for l in range(t["L"])], dtype=np.int64)
    return np.searchsorted(ends, np.asarray(entries, dtype=np.int64) // t["F"], side="right")


def sliced_plan(lv):
    """(task count, nrep[16], merge mask) of ngp_hash_bwd_sliced_plan (host logic, no GPU); task count -2: the table is refused."""
    from ngp_hip import lib
    nrep = np.zeros(16, dtype=np.uint8)
    mm = ctypes.c_uint32(0)
    n = lib.load().ngp_hash_bwd_sliced_plan(ctypes.byref(lv), None, 0, None, None, nrep.ctypes.data_as(ctypes.c_void_p), ctypes.byref(mm),
                                            None)
    return int(n), nrep.astype(np.int64), int(mm.value)


SINGLE, MERGE, REPLICATED = 0, 1, 2
CLASS_NAMES = ("single-owner non-merge", "merge", "replicated")


def level_class(level, nrep, merge_mask):
    """Per element: MERGE on run pre-summing levels, else REPLICATED where the slice has several owners, else SINGLE."""
    merge = ((merge_mask >> level) & 1).astype(bool)
    return np.where(merge, MERGE, np.where(nrep[level] > 1, REPLICATED, SINGLE))


def bound(sc, lv, nrep, merge_mask, fill=0.0, half=False):
    """The module docstring's bound, per element of sc."""
    u, tiny = (2.0**-11, 2.0**-25) if half else (2.0**-24, 2.0**-149)
    level = level_of(sc.entries, lv)
    rep = nrep[level].astype(f64)
    delta = ((merge_mask >> level) & 1).astype(f64)
    a = np.abs(sc.sum)
    b = u * a * (1.0 + 2.0**-10) + sc.k * 2.0**-52 * sc.S + delta * 15.0 * 2.0**-24 * sc.S
    b += np.where(rep > 1, (rep + 1.0) * u * (abs(fill) + sc.S), 0.0)
    if fill != 0.0:
        b += u * (abs(fill) + a)
    if half:
        b += sc.k_sub * 2.0**-24
    return b + tiny


def oracle_bound(sc):
    """|oracle - sum|: the oracle sums the same products in float64 in sample order and rounds once to float32."""
    return 2.0**-24 * np.abs(sc.sum) * (1.0 + 2.0**-10) + sc.k * 2.0**-52 * sc.S + 2.0**-149


def rounded(sc, half=False):
    """fl32(sum), or fl16(fl32(sum)) as float32: what a single owner's flush onto zeros stores."""
    r = sc.sum.astype(f32)
    return r.astype(f16).astype(f32) if half else r


def near_tie(sc, half=False):
    """Elements whose sum lies within k 2^-52 S of a rounding boundary of the flush: there a float64 accumulation in another order may
    round the other way.  The half2 form has none: its terms are f16 numbers, integer multiples of 2^-24, and S < 2^28 (asserted), so
    every partial sum in any order is an integer multiple of 2^-24 below 2^52 of them -- float64 adds them exactly, both sides hold
    the same exact sum and round it the same way, ties included."""
    if half:
        assert float(sc.S.max()) < 2.0**28 and np.all(sc.sum * 2.0**24 == np.rint(sc.sum * 2.0**24))
        return np.zeros(sc.sum.shape, dtype=bool)
    slack = sc.k * 2.0**-52 * sc.S
    r = sc.sum.astype(f32)
    lo, hi = np.nextafter(r, f32(-np.inf)).astype(f64), np.nextafter(r, f32(np.inf)).astype(f64)
    return (np.abs(sc.sum - 0.5 * (r.astype(f64) + lo)) <= slack) | (np.abs(sc.sum - 0.5 * (r.astype(f64) + hi)) <= slack)


# ------------------------------------------------------------------------------------------------ input builders
def gradients(rng, n, width, lo_exp=-20.0, hi_exp=2.0):
    """[n, width] float32 with random signs and magnitudes 2^U(lo_exp, hi_exp), clipped into [2^lo_exp, 2^hi_exp]: with the f32
    defaults no product with a weight above 2^-100 is an f32 subnormal."""
    mag = np.exp2(rng.uniform(lo_exp, hi_exp, size=(n, width))).astype(f32)
    mag = np.clip(mag, f32(2.0**lo_exp), f32(2.0**hi_exp))
    g = (mag * np.where(rng.random((n, width)) < 0.5, f32(-1), f32(1))).astype(f32)
    assert g.dtype == f32 and np.all(np.abs(g) >= f32(2.0**lo_exp)) and np.all(np.abs(g) <= f32(2.0**hi_exp))
    return g


def half_gradients(rng, n, width):
    """|g| in [1, 2) with random signs: with weights of at least MARGIN^3 no half2 term is an f16 subnormal."""
    g = ((f32(1) + rng.random((n, width), dtype=f32)) * np.where(rng.random((n, width)) < 0.5, f32(-1), f32(1))).astype(f32)
    g = np.minimum(np.abs(g), np.nextafter(f32(2), f32(0))) * np.sign(g)
    assert np.all(np.abs(g) >= 1) and np.all(np.abs(g) < 2)
    return g.astype(f32)


def find_centres(lv, count, seed):
    """The first `count` centres of a seeded search around which a box of side BOX stays MARGIN of a cell away from every face on
    every level (float64 estimate with a little room; the builders assert the real thing from the float32 cells)."""
    t = ref.level_table(lv)
    rng = np.random.default_rng(seed)
    found = []
    for _ in range(64):
        c = (rng.random((4096, 3)) * 0.8 + 0.1).astype(f32)
        ok = np.ones(4096, dtype=bool)
        for l in range(t["L"]):
            sc = f64(t["scale"][l])
            pos = c.astype(f64) * sc + 0.5
            fr = pos - np.floor(pos)
            room = MARGIN + 0.51 * BOX * sc + 0.01
            ok &= np.all((fr >= room) & (fr <= 1.0 - room), axis=1)
        found.extend(c[ok])
        if len(found) >= count:
            return np.array(found[:count], dtype=f32)
    raise AssertionError("no centre found")


def _box(rng, centre, n):
    return (np.asarray(centre, dtype=f32) + (rng.random((n, 3), dtype=f32) - f32(0.5)) * f32(BOX)).astype(f32)


def assert_one_cell(x, lv):
    """Every sample of x lies in one cell on every level, at least MARGIN of a cell from every face.  Returns the cells [L, 3]."""
    t = ref.level_table(lv)
    cells = []
    for l in range(t["L"]):
        cell, fr = ref.cell_frac(x, t["scale"][l])
        assert np.all(cell == cell[0]), "level %d: the samples do not share a cell" % l
        assert np.all(fr >= MARGIN) and np.all(fr <= 1.0 - MARGIN), "level %d: a sample is within %g of a cell face" % (l, MARGIN)
        cells.append(cell[0])
    return np.array(cells)


def one_cell(lv, seed=1, half=False):
    """N_ONE_CELL samples in one cell on every level (every sample a hit of the same slices, every bitmap word full, every 16-lane
    row one run), gradient rows ONE_CELL_ZERO_ROWS exactly zero: (x, g)."""
    rng = np.random.default_rng(seed)
    x = _box(rng, find_centres(lv, 1, seed)[0], N_ONE_CELL)
    assert_one_cell(x, lv)
    assert len(np.unique(x, axis=0)) >= N_ONE_CELL - 3
    width = int(lv.n_levels) * int(lv.n_features)
    g = half_gradients(rng, N_ONE_CELL, width) if half else gradients(rng, N_ONE_CELL, width)
    g[list(ONE_CELL_ZERO_ROWS)] = 0.0
    assert np.all(np.any(g[[0, 1, 62, 63, 64]] != 0, axis=1))
    return x, g


def _hit_slices(x1, lv, l):
    """Slices (contiguous 8192-entry ranges) of a hashed level l that the corners of position x1 fall into."""
    t = ref.level_table(lv)
    idx, _ = ref.corners(x1[None, :], lv)
    return set(int(v) for v in (idx[0, l].astype(np.int64) - t["offset"][l]) >> SLICE_LOG2)


def pieces(lv, by, seed=2):
    """N_PIECES samples alternating between two one-cell boxes A and B, by sample parity (by = 1) or by 8-sample piece (by = 8).  A
    and B lie in different cells on every level (so on the run pre-summing levels a run ends at every lane / every eighth lane), and
    on every many-slice hashed level some slice is hit by A alone: its owner's bitmap has every 8-sample piece (by = 8: every other
    piece) non-empty with gaps -- 512 (256) non-empty pieces per 4096-sample super-chunk, several trips of the compaction.  (x, g)."""
    assert by in (1, 8)
    rng = np.random.default_rng(seed)
    ca, cb = find_centres(lv, 2, seed)
    sel = (np.arange(N_PIECES) // by) % 2
    x = np.where(sel[:, None] == 0, _box(rng, ca, N_PIECES), _box(rng, cb, N_PIECES)).astype(f32)
    cells_a, cells_b = assert_one_cell(x[sel == 0], lv), assert_one_cell(x[sel == 1], lv)
    assert np.all(np.any(cells_a != cells_b, axis=1)), "A and B share a cell on some level"
    t = ref.level_table(lv)
    many = [l for l in range(t["bfhl"], t["L"]) if t["size"][l] > (8 << SLICE_LOG2)]
    assert many and all(_hit_slices(x[sel == 0][0], lv, l) - _hit_slices(x[sel == 1][0], lv, l) for l in many), "no slice is hit by A alone"
    g = gradients(rng, N_PIECES, t["L"] * t["F"])
    return x, g


def mixed(seed=3):
    """About 6000 samples: ray-like runs (consecutive samples share coarse cells), uniform points, the box's corners; every seventh
    gradient row zero.  (x, g, perm, m): perm a permutation to launch through as the live list, m < n the device count to use."""
    rng = np.random.default_rng(seed)
    n_rays, per_ray = 60, 50
    o = rng.random((n_rays, 1, 3), dtype=f32) * f32(0.8) + f32(0.1)
    d = rng.standard_normal((n_rays, 1, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    tt = (np.arange(per_ray, dtype=f32) * f32(0.0017))[None, :, None]
    x = np.clip(o + d * tt, 0.0, 1.0).reshape(-1, 3).astype(f32)
    x = np.concatenate([x, rng.random((3003, 3), dtype=f32),
                        np.array([[0, 0, 0], [1, 1, 1], [1, 0, 1], [0.999999, 1e-7, 0.5]], dtype=f32)]).astype(f32)
    n = x.shape[0]
    g = gradients(rng, n, 32)
    g[::7] = 0.0
    perm = rng.permutation(n).astype(np.int32)
    m = n - 1234
    assert n > 4096 and n % 64 != 0 and m % 64 != 0 and m > 4096
    return x, g, perm, m


def normalised(x01, lo, hi):
    """(x, x01'): positions x in [lo, hi] whose fused normalisation (x - lo) / (hi - lo), two float32 operations, is x01'."""
    x = (np.asarray(x01, dtype=f32) * (f32(hi) - f32(lo)) + f32(lo)).astype(f32)
    back = ((x - f32(lo)) / (f32(hi) - f32(lo))).astype(f32)
    assert back.dtype == f32 and np.all(back >= 0) and np.all(back <= 1)
    return x, back
