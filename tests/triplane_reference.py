"""Closed-form numpy restatement of the reference's tri-plane encoder (modules/triplane.py:35-98) and of its gradient -- the CPU
oracle of tests/test_triplane.py and tests/test_gpu_triplane.py.

Every step is a separate float32 operation, in the order the reference writes it, so the forward is bit-exact to a build with
-ffp-contract=off.  The gradient is summed in float64 and returned sparsely (max_res 4096 has 201 M entries)."""
import numpy as np

F = 4
f32 = np.float32


def resolutions(base_res, max_res, levels):
    """utils.py:31-39 (f64 log_b) then grid_scale / grid_resolution of triplane.py:27-33 in f32."""
    log_b = np.log(float(max_res) / float(base_res)) / float(levels - 1)
    res = []
    for l in range(levels):
        sc = f32(base_res) * np.exp(f32(l) * f32(log_b)) - f32(1.0)
        res.append(int(np.uint32(np.ceil(sc))) + 1)
    return res


def _corners(x, r, max_res):
    """Per axis: grid point g, the two weights (1 - frac, frac) and the two full-resolution coordinates."""
    x = np.clip(np.asarray(x, dtype=f32), f32(0), f32(1))
    pos = x * f32(r - 1) + f32(0.5)
    g = np.floor(pos).astype(np.uint32)
    fr = pos - g.astype(f32)
    w = (f32(1.0) - fr, fr)
    ori = tuple((((g + np.uint32(k)).astype(f32) / f32(r)) * f32(max_res - 1)).astype(np.uint32) for k in (0, 1))
    return g, w, ori


def _lookups(x, r, max_res):
    """For plane p, corner c: (entry index [n] int64 of feature 0, weight [n] f32)."""
    _, w, ori = _corners(x, r, max_res)
    M = np.int64(max_res)
    out = []
    for p in range(3):
        a, b = p, (p + 1) % 3
        row = []
        for c in range(4):
            idx = ori[c & 1][:, a].astype(np.int64) + ori[c >> 1][:, b].astype(np.int64) * M
            wt = w[c & 1][:, a] * w[c >> 1][:, b]
            row.append(((np.int64(p) * M * M + idx) * F, wt))
        out.append(row)
    return out


def _plane_sums(table, look):
    lf = []
    for p in range(3):
        s = np.zeros((look[p][0][1].shape[0], F), dtype=f32)
        for base, wt in look[p]:
            t = table[base[:, None] + np.arange(F)]
            s = s + wt[:, None] * t
        lf.append(s)
    return lf


def forward(x, table, max_res, res):
    """x [n,3] f32 -> [n, L*F] f32, column j*L + level."""
    x = np.asarray(x, dtype=f32)
    L = len(res)
    out = np.empty((x.shape[0], L * F), dtype=f32)
    for l, r in enumerate(res):
        lf = _plane_sums(table, _lookups(x, r, max_res))
        o = ((f32(1.0) * lf[0]) * lf[1]) * lf[2]
        for j in range(F):
            out[:, j * L + l] = o[:, j]
    return out


def backward(x, dout, table, max_res, res):
    """True d(sum(out * dout)) / d(table), sparse: (entry indices int64 ascending, values f64, sum of |terms| per entry f64)."""
    x = np.asarray(x, dtype=f32)
    L = len(res)
    idx_all, val_all = [], []
    for l, r in enumerate(res):
        look = _lookups(x, r, max_res)
        lf = [v.astype(np.float64) for v in _plane_sums(table, look)]
        d = np.stack([dout[:, j * L + l] for j in range(F)], 1).astype(np.float64)
        others = (lf[1] * lf[2], lf[0] * lf[2], lf[0] * lf[1])
        for p in range(3):
            for base, wt in look[p]:
                idx_all.append(base[:, None] + np.arange(F))
                val_all.append(d * others[p] * wt.astype(np.float64)[:, None])
    idx = np.concatenate([i.reshape(-1) for i in idx_all])
    val = np.concatenate([v.reshape(-1) for v in val_all])
    uniq, inv = np.unique(idx, return_inverse=True)
    return uniq, np.bincount(inv, weights=val, minlength=len(uniq)), np.bincount(inv, weights=np.abs(val), minlength=len(uniq))
