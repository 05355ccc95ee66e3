"""CPU reference of the hash encoder's DOUBLE backward (csrc/hash_grad_input2.hip) -- the yardstick of tests/test_hash_input_grad2.py and
tests/test_gpu_hash_input_grad2.py.  Cells, corner entries and level tables come from hash_input_grad_reference.

With the first backward dx_k = sum_l scale_l sum_c s_k(c) prod_{j != k} w_j(c_j) t_c (t_c = g . T_c, g = denc[i,l,:]), v = ddx[i,:] the
gradient of a loss with respect to dx and A_c = sum_k v_k s_k(c) prod_{j != k} w_j(c_j):

    d_denc[i,l,f]           = scale_l sum_c A_c T_c,f
    d_x[i,m]                = sum_l scale_l^2 sum_{k != m} v_k M_km,     M_km = sum_c s_k(c) s_m(c) w_j(c_j) t_c   (j the third axis)
    d_table[off_l+idx_c,f] += scale_l A_c g_f

`bwd2_64` evaluates them in float64 from the forward's float32 weights (fr and 1 - fr, widened) together with, per element, the sum S
of the magnitudes of all its terms; `bwd2_32` evaluates the same formulas serially in float32, written out on their own;
`TorchEncoder` is the encoder in plain torch, which torch's own autograd differentiates twice."""
import numpy as np
import torch

import hash_input_grad_reference as ref

f32, f64 = np.float32, np.float64


def bwd2_64(x, table, denc, ddx, lv, exact=False):
    """d_denc64 [n, L*F], S_denc, d_x64 [n,3], S_x, d_table64 [entries*F], S_table.  `exact`: float64 positions, cells and weights (the
    finite-difference test only)."""
    t = ref.level_table(lv)
    L, F = t["L"], t["F"]
    x = np.asarray(x, dtype=f64 if exact else f32)
    n = x.shape[0]
    T = np.asarray(table).astype(f64).reshape(-1, F)
    g = np.asarray(denc).astype(f64).reshape(n, L, F)
    v = np.asarray(ddx).astype(f64).reshape(n, 3)
    d_denc, S_denc = np.zeros((n, L, F)), np.zeros((n, L, F))
    d_x, S_x = np.zeros((n, 3)), np.zeros((n, 3))
    d_table, S_table = np.zeros_like(T), np.zeros_like(T)
    with np.errstate(invalid="ignore"):
        for l in range(L):
            idx, side = ref._level(x, t, l, False, exact)
            side = [(a.astype(f64), b.astype(f64)) for a, b in side]
            sc = f64(t["scale"][l])
            # d_denc in the difference form of the kernels (far minus near corner along k, weighted by the two other axes): the same
            # terms as sum_c A_c T_c, and exactly 0 for a table that is constant over the cell
            for k in range(3):
                j, m = (k + 1) % 3, (k + 2) % 3
                for a in range(2):
                    for b in range(2):
                        near = (a << j) | (b << m)
                        w = side[j][a] * side[m][b]
                        d_denc[:, l] += sc * (v[:, k] * w)[:, None] * (T[idx[:, near | (1 << k)]] - T[idx[:, near]])
            for c in range(8):
                bit = [(c >> d) & 1 for d in range(3)]
                sgn = [1.0 if b else -1.0 for b in bit]
                Tc = T[idx[:, c]]
                A, Aabs = np.zeros(n), np.zeros(n)
                for k in range(3):
                    j, m = (k + 1) % 3, (k + 2) % 3
                    w = side[j][bit[j]] * side[m][bit[m]]
                    A += v[:, k] * sgn[k] * w
                    Aabs += np.abs(v[:, k]) * np.abs(w)
                S_denc[:, l] += sc * Aabs[:, None] * np.abs(Tc)
                np.add.at(d_table, idx[:, c], sc * A[:, None] * g[:, l])
                np.add.at(S_table, idx[:, c], sc * Aabs[:, None] * np.abs(g[:, l]))
                tc = (g[:, l] * Tc).sum(1)
                ta = (np.abs(g[:, l]) * np.abs(Tc)).sum(1)
                for m in range(3):
                    for k in range(3):
                        if k == m:
                            continue
                        j = 3 - k - m
                        d_x[:, m] += sc * sc * v[:, k] * sgn[k] * sgn[m] * side[j][bit[j]] * tc
                        S_x[:, m] += sc * sc * np.abs(v[:, k]) * np.abs(side[j][bit[j]]) * ta
    return d_denc.reshape(n, L * F), S_denc.reshape(n, L * F), d_x, S_x, d_table.reshape(-1), S_table.reshape(-1)


def bwd2_32(x, table, denc, ddx, lv):
    """The same three formulas, every product and sum a float32 operation in the order the formula is written (levels outermost, then
    corners, then axes); the scatter accumulates in sample order.  Returns d_denc32 [n, L*F], d_x32 [n,3], d_table32 [entries*F]."""
    t = ref.level_table(lv)
    L, F = t["L"], t["F"]
    x = np.asarray(x, dtype=f32)
    n = x.shape[0]
    T = np.asarray(table).astype(f32).reshape(-1, F)
    g = np.asarray(denc).astype(f32).reshape(n, L, F)
    v = np.asarray(ddx).astype(f32).reshape(n, 3)
    d_denc = np.zeros((n, L, F), dtype=f32)
    d_x = np.zeros((n, 3), dtype=f32)
    contrib = np.zeros((n, L, 8, F), dtype=f32)
    entry = np.zeros((n, L, 8), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            scale = f32(t["scale"][l])
            cell, fr = ref.cell_frac(x, scale, False, False)
            w = (f32(1.0) - fr, fr)                              # w[bit][:, axis]
            dense = l < t["bfhl"]
            level_x = np.zeros((n, 3), dtype=f32)
            level_denc = np.zeros((n, F), dtype=f32)
            for c in range(8):
                bx, by, bz = c & 1, (c >> 1) & 1, (c >> 2) & 1
                e = t["offset"][l] + ref.level_index(dense, t["size"][l], t["res"][l], (cell[:, 0] + np.uint64(bx)) & np.uint64(ref.M32),
                                                     (cell[:, 1] + np.uint64(by)) & np.uint64(ref.M32),
                                                     (cell[:, 2] + np.uint64(bz)) & np.uint64(ref.M32))
                entry[:, l, c] = e
                wx, wy, wz = w[bx][:, 0], w[by][:, 1], w[bz][:, 2]
                A = np.zeros(n, dtype=f32)
                for vk, far, prod in ((v[:, 0], bx, wy * wz), (v[:, 1], by, wz * wx), (v[:, 2], bz, wx * wy)):
                    A = A + vk * prod if far else A - vk * prod
                tc = np.zeros(n, dtype=f32)
                for f in range(F):
                    level_denc[:, f] = level_denc[:, f] + A * T[e, f]
                    contrib[:, l, c, f] = (scale * A) * g[:, l, f]
                    tc = tc + g[:, l, f] * T[e, f]
                # mixed second derivatives: the sign of corner c in M_km is s_k(c) * s_m(c), its weight the third axis's
                sxy, syz, szx = (wz * tc, bx == by), (wx * tc, by == bz), (wy * tc, bz == bx)
                for m_axis, pairs in ((0, ((v[:, 1], sxy), (v[:, 2], szx))), (1, ((v[:, 0], sxy), (v[:, 2], syz))),
                                      (2, ((v[:, 0], szx), (v[:, 1], syz)))):
                    for vk, (term, plus) in pairs:
                        level_x[:, m_axis] = level_x[:, m_axis] + vk * term if plus else level_x[:, m_axis] - vk * term
            d_denc[:, l] = scale * level_denc
            d_x = d_x + (scale * scale) * level_x
        d_table = np.zeros(T.size, dtype=f32)
        flat = (entry[:, :, :, None] * F + np.arange(F)[None, None, None, :]).reshape(-1)
        np.add.at(d_table, flat, contrib.reshape(-1))            # unbuffered: one float32 add per contribution, in sample order
    assert d_denc.dtype == f32 and d_x.dtype == f32 and d_table.dtype == f32
    return d_denc.reshape(n, L * F), d_x, d_table


class TorchEncoder:
    """The hash encoding in plain torch on the CPU: enc = TorchEncoder(lv, dtype)(x, table) is differentiable any number of times by
    torch's autograd.  Corner entries come from `corners`; the fraction is the forward's float32 value (computed as cell_frac does)
    with d fr / d x = scale attached, and 1 - fr is the float32 difference; everything after runs in `dtype` (float64: the reference,
    float32: the yardstick)."""

    def __init__(self, lv, dtype):
        self.lv, self.t, self.dtype = lv, ref.level_table(lv), dtype

    def __call__(self, x, table):
        t, dt = self.t, self.dtype
        L, F = t["L"], t["F"]
        xn = x.detach().to(torch.float32).numpy()
        idx, _ = ref.corners(xn, self.lv)
        idx = torch.from_numpy(idx.astype(np.int64))
        n = idx.shape[0]
        # one gather for all levels and corners: its backward is ONE index_add into a table-sized buffer, not L * 8 of them
        Tc = table.to(dt).view(-1, F).index_select(0, idx.reshape(-1)).view(n, L, 8, F)
        xd = x.to(dt)
        outs = []
        for l in range(L):
            scale = f32(t["scale"][l])
            _, fr = ref.cell_frac(xn, scale, False, False)
            lin = (xd - xd.detach()) * float(scale)                        # exactly 0, derivative scale
            far = torch.from_numpy(fr).to(dt) + lin
            near = torch.from_numpy(f32(1.0) - fr).to(dt) - lin
            side = (near, far)
            acc = None
            for c in range(8):
                w = (side[c & 1][:, 0] * side[(c >> 1) & 1][:, 1]) * side[(c >> 2) & 1][:, 2]
                term = w[:, None] * Tc[:, l, c]
                acc = term if acc is None else acc + term
            outs.append(acc)
        return torch.cat(outs, 1)
