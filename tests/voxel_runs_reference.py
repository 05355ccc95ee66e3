"""Serial float32 restatement of the voxel-grid backward's run merge (ngp_voxel_bwd / ngp_voxel_trilinear_bwd; csrc/voxel_grid.hip),
and the inputs on which it is exact.

The kernels give one wave 64 consecutive samples, sum each run of equal row (nearest) or equal base cell (trilinear) in lane order,
`v = 0; for s in run: v += T[s][col]`, and issue one float atomic per run and address.  Float addition is commutative, so an address
that receives at most TWO adds holds the same bits in whatever order they arrive; `merge()` counts the adds per address and
`make_case()` builds inputs that stay within two.  Then the kernel can be held bit for bit to this file.  Every operation below is a
single float32 numpy operation in the kernel's order (the library is built with -ffp-contract=off)."""
import numpy as np

import voxel_reference as vr

G = 8
R = np.float32(0.0125)
WAVE = 64
F32 = np.float32
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)


def basis(deg, dirs):
    """[n, D] eval_sh basis of voxel_reference._basis_table in the dtype of `dirs` (unit directions), factors multiplied in order."""
    x, y, z = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    cols = []
    for const, factors in vr._basis_table(x, y, z)[:(deg + 1)**2]:
        t = np.full(x.shape, const, dtype=dirs.dtype)
        for f in factors:
            t = t * f
        cols.append(t)
    return np.stack(cols, 1)


def normalized_index(x):
    """(p - m) / r in f32, as vr.normalized_index."""
    return (x.astype(F32) - vr.grid_min(G, R)) / R


def tile_rows(deg, c):
    """(T [n, 3 D + 1] f32, contributes [n] bool): the row every lane writes, column ch * D + k = g[ch] * Y[k], column 3 D = gs."""
    D = (deg + 1)**2
    gs = np.where(c["sigmas"] > 0, c["dsigmas"], F32(0))
    g = c["drgbs"] * (c["rgbs"] * (F32(1) - c["rgbs"]))
    Y = basis(deg, c["dirs"] / np.sqrt((c["dirs"] * c["dirs"]).sum(1, dtype=F32))[:, None])
    T = np.concatenate([(g[:, :, None] * Y[:, None, :]).reshape(-1, 3 * D), gs[:, None]], 1)
    assert T.dtype == F32
    return T, ~((gs == 0) & (g == 0).all(1))


def runs(keys):
    """(start, end) of every run of equal key >= 0 inside a wave of 64 consecutive samples."""
    out = []
    for w0 in range(0, len(keys), WAVE):
        s = w0
        w1 = min(w0 + WAVE, len(keys))
        while s < w1:
            e = s + 1
            while e < w1 and keys[e] == keys[s]:
                e += 1
            if keys[s] >= 0:
                out.append((s, e))
            s = e
    return out


def merge(deg, c, trilinear):
    """(dsh [G^3, 3 D], ddensity [G^3], adds_sh, adds_density): the gradients as the kernel forms them, and how many atomic adds
    each address receives."""
    D = (deg + 1)**2
    T, contributes = tile_rows(deg, c)
    u = normalized_index(c["xyzs"])
    dsh, dden = np.zeros((G**3, 3 * D), F32), np.zeros(G**3, F32)
    n_sh, n_den = np.zeros((G**3, 3 * D), np.int64), np.zeros(G**3, np.int64)

    def add(row, v):
        """one atomic per nonzero value: columns [0, 3 D) into dsh[row], column 3 D into ddensity[row]"""
        nz = v != 0
        dsh[row][nz[:3 * D]] += v[:3 * D][nz[:3 * D]]
        n_sh[row] += nz[:3 * D]
        if nz[3 * D]:
            dden[row] += v[3 * D]
            n_den[row] += 1

    if not trilinear:
        a = np.rint(u)
        inside = ((a >= 0) & (a < G)).all(1)
        ai = np.where(inside[:, None], a, 0).astype(np.int64)
        keys = np.where(inside & contributes, (ai[:, 0] * G + ai[:, 1]) * G + ai[:, 2], -1)
        for s0, s1 in runs(keys):
            v = np.zeros(3 * D + 1, F32)
            for s in range(s0, s1):
                v = v + T[s]
            add(keys[s0], v)
        return dsh, dden, n_sh, n_den
    inside = ((u >= -1) & (u < G)).all(1)
    u = np.where(inside[:, None], u, F32(0))
    b = np.floor(u)
    f = u - b
    b = b.astype(np.int64)
    keys = np.where(inside & contributes, ((b[:, 0] + 1) * (G + 1) + b[:, 1] + 1) * (G + 1) + b[:, 2] + 1, -1)
    wts = np.stack([(f[:, 0] if k & 4 else F32(1) - f[:, 0]) * (f[:, 1] if k & 2 else F32(1) - f[:, 1])
                    * (f[:, 2] if k & 1 else F32(1) - f[:, 2]) for k in range(8)], 1)
    assert wts.dtype == F32
    for s0, s1 in runs(keys):
        for k in range(8):
            q = b[s0] + np.array([k >> 2, (k >> 1) & 1, k & 1])
            if ((q < 0) | (q >= G)).any():
                continue
            v = np.zeros(3 * D + 1, F32)
            for s in range(s0, s1):
                v = v + wts[s, k] * T[s]
            add((q[0] * G + q[1]) * G + q[2], v)
    return dsh, dden, n_sh, n_den


N_SAMPLES = (64, 256, 256 + 17, 3 * 256 + 17)              # one wave, one block, a ragged tail, several blocks


def make_case(n, trilinear, seed=0):
    """Inputs of one case: every voxel (base cell) is visited in ONE contiguous stretch of 1 to 90 samples that crosses at most one
    wave boundary, or is cut once by an inactive sample, never both: no address gets more than two adds.  Trilinear base cells come
    from {-1, 1, 3, 5, 7}^3: two of them differ by two on some axis, so they share no corner row, and -1 and G - 1 have corners
    outside the grid.  Inactive samples (out of the grid; all four gradients zero) sit between stretches and, once, inside some;
    some sigmas are <= 0; directions are the six axes at length 1 or 2; rgbs are arbitrary f32 in (0, 1)."""
    rng = np.random.default_rng([n, int(trilinear), seed])
    m = vr.grid_min(G, R)
    if trilinear:
        lattice = np.array([-1, 1, 3, 5, 7])
        cells = np.stack(np.meshgrid(lattice, lattice, lattice, indexing="ij"), -1).reshape(-1, 3)
    else:
        cells = np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), -1).reshape(-1, 3)
    cells = cells[rng.permutation(len(cells))]
    u = np.zeros((n, 3))
    dead = np.zeros(n, np.int64)                                           # 0: live, 1: out of the grid, 2: zero gradients
    s, visit, n_dead = 0, 0, 0
    while s < n:
        # an inactive sample between two stretches; the kinds alternate, and the first stretch has one of each around it
        if (n_dead < 2 and visit == n_dead) or rng.random() < 0.3:
            dead[s] = 1 + n_dead % 2
            n_dead += 1
            u[s] = cells[visit] + 0.5
            s += 1
            continue
        length = int(rng.integers(1, 7) if rng.random() < 0.5 else rng.integers(1, 91))
        length = min(length, n - s, 2 * WAVE - s % WAVE)                   # at most one wave boundary inside the stretch
        lo = (0.05, 0.95) if trilinear else (-0.4, 0.4)
        u[s:s + length] = cells[visit] + rng.uniform(*lo, (length, 3))
        crosses = (s % WAVE) + length > WAVE
        if not crosses and length >= 3 and rng.random() < 0.4:             # cut the stretch once
            dead[s + rng.integers(1, length - 1)] = 1 + n_dead % 2
            n_dead += 1
        s += length
        visit += 1
    assert visit <= len(cells)
    c = {"xyzs": (m + u.astype(F32) * R).astype(F32)}
    c["xyzs"][dead == 1] = F32(5.0)
    c["dirs"] = AXES[rng.integers(0, 6, n)] * rng.integers(1, 3, n)[:, None].astype(F32)
    c["sigmas"] = rng.uniform(0.1, 3.0, n).astype(F32)
    k = rng.random(n)
    c["sigmas"][k < 0.15] = 0                                               # d sigma / d density = 0 there: no density gradient
    c["sigmas"][k > 0.9] = -0.5
    c["rgbs"] = rng.uniform(0.02, 0.98, (n, 3)).astype(F32)
    c["dsigmas"] = rng.standard_normal(n).astype(F32)
    c["drgbs"] = rng.standard_normal((n, 3)).astype(F32)
    c["dsigmas"][dead == 2] = 0
    c["drgbs"][dead == 2] = 0
    c["drgbs"][rng.random(n) < 0.1, 1] = 0                                 # single zero channels: columns that sum to nothing
    return c
