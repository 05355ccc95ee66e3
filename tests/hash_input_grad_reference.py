"""Closed-form numpy restatement of the hash-grid encoder's corner rule (csrc/hash_common.h: cell_frac, corner_weight, level_index) and
of the gradient of the encoding with respect to the sample position -- the CPU reference of tests/test_hash_input_grad.py and
tests/test_gpu_hash_input_grad.py.

Cells and fractions are separate float32 operations in the order cell_frac writes them (the half2 encoder's cell goes through
np.float16), so corner entries and forward weights are the forward's bit for bit.  Everything after that is float64 (`grad64`), or a
serial float32 evaluation of the same formula written out on its own (`grad32`), whose distance from `grad64` is the yardstick the
GPU tests hold the kernel to.

    enc[l,f] = sum_c w_c(fr) * T[off_l + idx_c, f]
    dx_k     = sum_l scale_l * sum_f denc[l,f] * sum_c s_k(c) * prod_{j != k} w_j(c) * T[off_l + idx_c, f]

s_k(c) = +1 where corner c (bit d set: the far side along axis d) lies on the far side along k, -1 otherwise; w_j(c) = fr_j on the far
side, 1 - fr_j otherwise."""
import numpy as np

f32, f64 = np.float32, np.float64
PRIME_Y, PRIME_Z = 2654435761, 805459861
M32 = 0xffffffff


def level_table(lv):
    """The fields of an ngp_hash_levels struct as plain numpy / Python values."""
    L = int(lv.n_levels)
    return {"L": L, "F": int(lv.n_features), "bfhl": int(lv.begin_fast_hash_level),
            "scale": np.array([lv.scale[i] for i in range(L)], dtype=f32),
            "res": [int(lv.resolution[i]) for i in range(L)], "size": [int(lv.map_size[i]) for i in range(L)],
            "offset": [int(lv.offset[i]) for i in range(L)]}


def _f2u_sat(v):
    """f32 -> u32, truncating and saturating: NaN and negatives give 0, values of 2^32 and more give 0xffffffff."""
    v = np.asarray(v, dtype=f64)
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(v) | (v < 0), 0.0, np.minimum(v, float(M32)))
    return v.astype(np.uint64)


def cell_frac(x, scale, half=False, exact=False):
    """cell [n,3] uint64 (< 2^32) and fraction [n,3] of positions x on a level.  float32 in cell_frac's order; `half` rounds the cell
    through float16 before the subtract; `exact` does it all in float64 instead (the finite-difference test only)."""
    with np.errstate(invalid="ignore", over="ignore"):
        if exact:
            pos = np.asarray(x, dtype=f64) * f64(scale) + f64(0.5)
            cell = _f2u_sat(np.floor(pos))
            return cell, pos - cell.astype(f64)
        pos = np.asarray(x, dtype=f32) * f32(scale) + f32(0.5)
        cell = _f2u_sat(np.floor(pos))
        cf = cell.astype(f32)
        if half:
            cf = cf.astype(np.float16).astype(f32)
        return cell, pos - cf


def level_index(dense, size, res, gx, gy, gz):
    """Entry of grid point (gx, gy, gz) relative to the level's first: the raw 32-bit index modulo the level's size."""
    if dense:
        h = (gx + gy * np.uint64(res) + gz * np.uint64((res * res) & M32)) & np.uint64(M32)
    else:
        h = gx ^ ((gy * np.uint64(PRIME_Y)) & np.uint64(M32)) ^ ((gz * np.uint64(PRIME_Z)) & np.uint64(M32))
    return (h % np.uint64(size)).astype(np.int64)


def _level(x, t, l, half, exact):
    """Level l: entries [n,8] int64 (from the table's start) and the per-axis weights side[k][bit] [n] (near, far)."""
    cell, fr = cell_frac(x, t["scale"][l], half, exact)
    one = fr.dtype.type(1.0)
    side = [(one - fr[:, k], fr[:, k]) for k in range(3)]
    idx = np.empty((x.shape[0], 8), dtype=np.int64)
    for c in range(8):
        g = [(cell[:, d] + np.uint64((c >> d) & 1)) & np.uint64(M32) for d in range(3)]
        idx[:, c] = t["offset"][l] + level_index(l < t["bfhl"], t["size"][l], t["res"][l], *g)
    return idx, side


def corners(x, lv, half=False):
    """idx [n,L,8] uint32 (entries from the table's start) and the forward's trilinear weights w [n,L,8] float32, in the forward's
    product order ((1 * wx) * wy) * wz."""
    t = level_table(lv)
    x = np.asarray(x, dtype=f32)
    idx = np.empty((x.shape[0], t["L"], 8), dtype=np.uint32)
    w = np.empty((x.shape[0], t["L"], 8), dtype=f32)
    for l in range(t["L"]):
        li, side = _level(x, t, l, half, False)
        idx[:, l] = li
        with np.errstate(invalid="ignore"):
            for c in range(8):
                w[:, l, c] = ((f32(1.0) * side[0][c & 1]) * side[1][(c >> 1) & 1]) * side[2][(c >> 2) & 1]
    return idx, w


def forward64(x, table, lv, half=False, exact=False):
    """enc [n, L*F] float64 and the magnitude sum sum_c |w_c * T| per element, from the forward's weights widened to float64
    (`exact`: weights formed in float64 from float64 cells)."""
    t = level_table(lv)
    L, F = t["L"], t["F"]
    x = np.asarray(x, dtype=f64 if exact else f32)
    T = np.asarray(table).astype(f64).reshape(-1, F)
    enc = np.zeros((x.shape[0], L * F), dtype=f64)
    mag = np.zeros_like(enc)
    with np.errstate(invalid="ignore"):
        for l in range(L):
            idx, side = _level(x, t, l, half, exact)
            for c in range(8):
                w = (side[0][c & 1] * side[1][(c >> 1) & 1]) * side[2][(c >> 2) & 1]      # 1 * wx is exact
                term = w.astype(f64)[:, None] * T[idx[:, c]]
                enc[:, l * F:(l + 1) * F] += term
                mag[:, l * F:(l + 1) * F] += np.abs(term)
    return enc, mag


def grad64(x, table, denc, lv, half=False, exact=False):
    """dx64 [n,3] float64 and S [n,3] = sum_l scale_l sum_f |denc| sum_c prod_{j != k} |w_j| * |T|, the magnitude every bound on dx
    is relative to.  The per-axis weights are the forward's float32 values (fr and 1 - fr); everything after is float64."""
    t = level_table(lv)
    L, F = t["L"], t["F"]
    x = np.asarray(x, dtype=f64 if exact else f32)
    T = np.asarray(table).astype(f64).reshape(-1, F)
    g = np.asarray(denc).astype(f64).reshape(x.shape[0], L, F)
    dx = np.zeros((x.shape[0], 3), dtype=f64)
    S = np.zeros_like(dx)
    with np.errstate(invalid="ignore"):
        for l in range(L):
            idx, side = _level(x, t, l, half, exact)
            side = [(a.astype(f64), b.astype(f64)) for a, b in side]
            sc = f64(t["scale"][l])
            for c in range(8):
                tc = (g[:, l] * T[idx[:, c]]).sum(1)
                ta = (np.abs(g[:, l]) * np.abs(T[idx[:, c]])).sum(1)
                for k in range(3):
                    j, m = (k + 1) % 3, (k + 2) % 3
                    w = side[j][(c >> j) & 1] * side[m][(c >> m) & 1]
                    sgn = 1.0 if (c >> k) & 1 else -1.0
                    dx[:, k] += sc * sgn * w * tc
                    S[:, k] += sc * np.abs(w) * ta
    return dx, S


def grad32(x, table, denc, lv, half=False):
    """The same formula evaluated serially in float32, every product and sum a float32 operation in the order the formula is
    written: levels outermost, then features, then corners.  Returns dx32 [n,3] float32."""
    t = level_table(lv)
    L, F = t["L"], t["F"]
    x = np.asarray(x, dtype=f32)
    T = np.asarray(table).astype(f32).reshape(-1, F)            # bf16 / f16 tables widen exactly
    g = np.asarray(denc).astype(f32).reshape(x.shape[0], L, F)
    n = x.shape[0]
    dx = np.zeros((n, 3), dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            scale = f32(t["scale"][l])
            cell, fr = cell_frac(x, scale, half, False)
            near = f32(1.0) - fr
            dense = l < t["bfhl"]
            entries = []
            for c in range(8):
                gx = (cell[:, 0] + np.uint64(c & 1)) & np.uint64(M32)
                gy = (cell[:, 1] + np.uint64((c >> 1) & 1)) & np.uint64(M32)
                gz = (cell[:, 2] + np.uint64((c >> 2) & 1)) & np.uint64(M32)
                entries.append(t["offset"][l] + level_index(dense, t["size"][l], t["res"][l], gx, gy, gz))
            for k in range(3):
                j, m = (k + 1) % 3, (k + 2) % 3
                level_sum = np.zeros(n, dtype=f32)
                for f in range(F):
                    corner_sum = np.zeros(n, dtype=f32)
                    for c in range(8):
                        wj = fr[:, j] if (c >> j) & 1 else near[:, j]
                        wm = fr[:, m] if (c >> m) & 1 else near[:, m]
                        term = (wj * wm) * T[entries[c], f]
                        corner_sum = corner_sum + term if (c >> k) & 1 else corner_sum - term
                    level_sum = level_sum + g[:, l, f] * corner_sum
                dx[:, k] = dx[:, k] + scale * level_sum
    assert dx.dtype == f32
    return dx
