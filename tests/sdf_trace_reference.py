"""numpy reference of the sphere-tracing contract (include/ngp_hip.h, "sphere tracing"; csrc/sdf_trace.hip): the field and the trace,
each evaluated in np.float64 and as a SERIAL float32 restatement (every rounding a separate binary32 operation, fmaf one rounding).

Both arithmetics run the same code: arrays of dtype T, numpy's float32 operations are IEEE binary32, and `fma` is exact-then-rounded
(float64 product, two-sum, round to odd, one rounding to float32).  The trace is vectorised over rays in the kernel's own round
structure and logs every decision it takes with the quantity decided on.

decide()      a ray is DECIDED when, along the float64 path, every decision holds with a margin of 4 x max(|q32 - q64| on that ray at
              that decision, one float32 ulp of the quantity -- for a value of f: of max(|f|, |b_out|), the size of the terms that
              cancel in it); the serial float32 path must have taken the same decisions in the same
              order.  Decisions: t < t2, the slab's exit > 0, the occupancy bit of the probed cell (the same bit at t +- margin),
              f > eps, f >= 0, every bisection sign.
judge()       on decided rays status and n_eval are exact and t, xyz, f_last lie within 4 x E32 of float64; E32 = the largest
              |serial32 - float64| of that quantity over the decided rays of the set, at least one float32 ulp of its scale.
invariants()  hold for ANY output, undecided rays included.
MAX_UNDECIDED is a condition on the sets, not a measurement: the CPU test asserts it for the float64 reference alone."""
import numpy as np

MAX_UNDECIDED = 0.02                       # as tests/resample_reference.py
MISS, HIT, INSIDE, ABANDONED = 0, 1, 2, 3
DT_MIN = np.float32(1.7320508075688772 / 1024)
DEFAULTS = dict(eps=1e-4, step_scale=1.0, min_step=float(DT_MIN), n_refine=8, max_evals=256)
K_T2, K_SLAB, K_OCC, K_EPS, K_ZERO, K_BISECT = range(6)
PRIME_Y, PRIME_Z = np.uint32(2654435761), np.uint32(805459861)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def fma(a, b, c, T):
    """a * b + c with ONE rounding in T."""
    if T == np.float64:
        return a * b + c
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    p = a * b                                           # exact: 24 + 24 bits
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                   # two-sum: p + c = s + e exactly
    fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.int64) & 1) == 0)
    up = (e > 0.0) == (s > 0.0)                         # the exact sum lies further from zero than s
    bits = s.view(np.int64) + np.where(fix, np.where(up, 1, -1), 0)
    return bits.view(np.float64).astype(np.float32)     # round to odd in 53 bits, then once to 24


class Model:
    """A field: level table columns (scale f32, res, size, offset as arrays, bfhl), table [entries, 2] f32, MLP layers as
    [(W [out, in], b [out]), ..] f32 (the last one: w_out [1, width], b_out [1]), the box scale."""

    def __init__(self, levels, bfhl, table, layers, scale):
        self.lv_scale, self.lv_res, self.lv_size, self.lv_offset = (np.asarray(a) for a in levels)
        self.bfhl, self.table, self.layers, self.scale = int(bfhl), np.asarray(table, np.float32).reshape(-1, 2), layers, float(scale)
        self.width, self.depth = layers[0][0].shape[0], len(layers) - 1

    def value(self, x, T):
        return field(self, x, T)

    def pack(self):
        parts = []
        for W, b in self.layers:
            parts += [W.reshape(-1), b.reshape(-1)]
        return np.concatenate(parts).astype(np.float32)


def geometric_layers(rng, n_in, width, depth, radius):
    dims = [n_in] + [width] * depth
    layers = [((rng.standard_normal((b, a)) * np.sqrt(2.0 / b)).astype(np.float32), np.zeros(b, np.float32)) for a, b in zip(dims[:-1], dims[1:])]
    w_out = (np.sqrt(np.pi / width) + 1e-4 * rng.standard_normal((1, width))).astype(np.float32)
    return layers + [(w_out, np.full(1, -radius, np.float32))]


def embed(m, x01, T):
    """[n, 2 L] in T: the corner rule of hash_common.h, acc = 0; acc += w_c * v_c (multiply, then add)."""
    n, L = x01.shape[0], len(m.lv_res)
    out = np.zeros((n, 2 * L), T)
    one = T(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            pos = x01 * T(m.lv_scale[l]) + T(0.5)
            cell_f = np.clip(np.nan_to_num(np.floor(pos), nan=0.0, posinf=4294967295.0, neginf=0.0), 0.0, 4294967295.0)   # v_cvt_u32_f32
            cell = cell_f.astype(np.uint64).astype(np.uint32)
            fr = pos - cell.astype(T)
            res, size = np.uint32(m.lv_res[l]), np.uint32(m.lv_size[l])
            a0, a1 = np.zeros(n, T), np.zeros(n, T)
            for ci in range(8):
                g = [cell[:, k] + np.uint32((ci >> k) & 1) for k in range(3)]
                if l < m.bfhl:
                    h = g[0] + g[1] * res + g[2] * (res * res)
                else:
                    h = g[0] ^ (g[1] * PRIME_Y) ^ (g[2] * PRIME_Z)
                w = one
                for k in range(3):
                    w = w * (fr[:, k] if (ci >> k) & 1 else one - fr[:, k])
                v = m.table[(h % size).astype(np.int64) + int(m.lv_offset[l])].astype(T)
                a0 = a0 + w * v[:, 0]
                a1 = a1 + w * v[:, 1]
            out[:, 2 * l], out[:, 2 * l + 1] = a0, a1
    return out


def softplus(h, T):
    with np.errstate(over="ignore", invalid="ignore"):
        z = T(100.0) * h
        return np.where(z > T(20.0), h, np.log1p(np.exp(np.minimum(z, T(30.0)))) / T(100.0)).astype(T)


def field(m, x, T, return_enc=False):
    """f(x) for world positions x [n, 3] in the arithmetic T; sums in input-index order, bias first, one fma each."""
    x = np.asarray(x).astype(T)
    lo, hi = T(np.float32(-m.scale)), T(np.float32(m.scale))
    with np.errstate(invalid="ignore"):
        x01 = (x - lo) / (hi - lo)
    enc = embed(m, x01, T)
    h = np.concatenate([x, enc], 1)
    for W, b in m.layers[:-1]:
        t = np.broadcast_to(b.astype(T), (x.shape[0], W.shape[0])).copy()
        for j in range(W.shape[1]):
            t = fma(h[:, j:j + 1], W[:, j].astype(T)[None, :], t, T)
        h = softplus(t, T)
    W, b = m.layers[-1]
    f = np.full(x.shape[0], b[0], T)
    for k in range(W.shape[1]):
        f = fma(h[:, k], T(W[0, k]), f, T)
    return (f, enc) if return_enc else f


# ---- occupancy grid -------------------------------------------------------------------------------------------------------------------
def _expand_bits(v):
    v = (v * np.uint32(0x00010001)) & np.uint32(0xFF0000FF)
    v = (v * np.uint32(0x00000101)) & np.uint32(0x0F00F00F)
    v = (v * np.uint32(0x00000011)) & np.uint32(0xC30C30C3)
    return (v * np.uint32(0x00000005)) & np.uint32(0x49249249)


def morton3d(x, y, z):
    return _expand_bits(x) | (_expand_bits(y) << np.uint32(1)) | (_expand_bits(z) << np.uint32(2))


def cascades_of(scale):
    return max(1 + int(np.ceil(np.log2(2 * scale))), 1)


def shell_bitfield(scale, G, r0, r1):
    """cascades * G^3 bits: the cells whose centre lies at a radius in [r0, r1]."""
    casc = cascades_of(scale)
    i = np.arange(G, dtype=np.uint32)
    X, Y, Z = np.meshgrid(i, i, i, indexing="ij")
    code = morton3d(X.ravel(), Y.ravel(), Z.ravel()).astype(np.int64)
    bits = np.zeros(casc * G**3, np.uint8)
    for mip in range(casc):
        mb = min(2.0**(mip - 1), scale)
        c = ((np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1) + 0.5) / G * 2 - 1) * mb
        r = np.linalg.norm(c, axis=1)
        bits[mip * G**3 + code] = (r >= r0) & (r <= r1)
    return np.packbits(bits, bitorder="little")


def _frexp_bit(x):
    """ceil(log2 x) with exact powers of two mapped to their exponent (ngp_device.h frexp_bit); 0 for x = 0."""
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mant, e = np.frexp(x)                     # x = mant 2^e, mant in [0.5, 1)
    return np.where(x == 0, 0, np.where(mant == 0.5, e - 1, e)).astype(np.int64)


class Grid:
    def __init__(self, bitfield, scale, G):
        self.bits, self.scale, self.G, self.casc = np.asarray(bitfield, np.uint8), float(scale), int(G), cascades_of(scale)
        assert self.bits.size == self.casc * self.G**3 // 8

    def probe(self, o, d, t, T):
        """-> (occupied, xyz, nxyz, mip_bound) of the cell of o + t d, in the arithmetic T (march_common.h probe_cell at dt_min)."""
        G = T(self.G)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            xyz = o + t[:, None] * d
            if self.casc == 1:
                mip = np.zeros(len(t), np.int64)
            else:
                mx = np.nan_to_num(np.abs(xyz).max(1), nan=0.0)
                mip_pos = np.clip(_frexp_bit(mx) + 1, 0, self.casc - 1)
                mip_dt = np.clip(_frexp_bit(T(DT_MIN) * G), 0, self.casc - 1)
                mip = np.maximum(mip_pos, mip_dt)
            pw = np.ldexp(1.0, mip - 1)
            mb = np.where(pw <= self.scale, pw, self.scale).astype(T)
            mb_inv = np.where(pw <= self.scale, np.ldexp(1.0, 1 - mip), T(1.0) / T(np.float32(self.scale))).astype(T)
            v = T(0.5) * (xyz * mb_inv[:, None] + T(1.0)) * G
            nxyz = np.fmin(G - T(1.0), np.fmax(T(0.0), v))
            nxyz = np.where(np.isnan(nxyz), T(0.0), nxyz)
            c = nxyz.astype(np.uint32)
            idx = mip * self.G**3 + morton3d(c[:, 0], c[:, 1], c[:, 2]).astype(np.int64)
        occ = (self.bits[idx >> 3] >> (idx & 7).astype(np.uint8)) & 1
        return occ.astype(bool), xyz, nxyz, mb

    def skip_target(self, d, d_inv, t, xyz, nxyz, mb, T):
        with np.errstate(invalid="ignore", over="ignore"):
            sg = np.sign(d).astype(T)
            v = (((nxyz + T(0.5) + T(0.5) * sg) * T(1.0 / self.G) * T(2.0) - T(1.0)) * mb[:, None] - xyz) * d_inv
            tmin = v[:, 0]
            for k in (1, 2):
                tmin = np.fmin(tmin, v[:, k])
            return t + np.fmax(T(0.0), tmin)


def slab(o, d_inv, scale, T):
    with np.errstate(invalid="ignore", over="ignore"):
        half = (T(np.float32(scale)) - (-T(np.float32(scale)))) / T(2.0)
        tmin, tmax = (T(0.0) - half - o) * d_inv, (T(0.0) + half - o) * d_inv
        lo, hi = np.fmin(tmin, tmax), np.fmax(tmin, tmax)
        a1, a2 = lo[:, 0], hi[:, 0]
        for k in (1, 2):
            a1, a2 = np.fmax(a1, lo[:, k]), np.fmin(a2, hi[:, k])
        hit = a2 > T(0.0)
    return np.where(hit, np.fmax(a1, T(np.float32(0.01))), T(-1.0)), np.where(hit, a2, T(-1.0)), a2


# ---- the trace -------------------------------------------------------------------------------------------------------------------------
def trace(m, grid, o, d, T, eps=1e-4, step_scale=1.0, min_step=float(DT_MIN), n_refine=8, max_evals=256):
    """-> dict status, t, xyz, n_eval, f_last (arrays over rays, t / xyz / f_last in T) and `log`: the decisions as columns
    (ray, kind, q, scale, aux) in the order each ray took them."""
    o, d = np.asarray(o, np.float32).astype(T), np.asarray(d, np.float32).astype(T)
    n = o.shape[0]
    eps, step_scale, min_step = (T(np.float32(v)) for v in (eps, step_scale, min_step))
    with np.errstate(divide="ignore"):
        d_inv = T(1.0) / d
    t1, t2, a2 = slab(o, d_inv, m.scale, T)
    log = []
    fs = max(abs(float(m.layers[-1][1][0])), float(eps))      # the scale of f: a sum that starts at b_out and cancels down to ~0 at the surface

    def record(rays, kind, q, scale, aux=None):
        if len(rays):
            log.append((rays.copy(), np.full(len(rays), kind), np.asarray(q, np.float64), np.asarray(scale, np.float64),
                        np.zeros(len(rays)) if aux is None else np.asarray(aux, np.float64)))

    every = np.arange(n)
    record(every, K_SLAB, np.nan_to_num(a2.astype(np.float64), nan=-1.0, posinf=1e30, neginf=-1e30), np.abs(np.nan_to_num(a2, nan=1.0, posinf=1.0, neginf=1.0)))
    status = np.full(n, -1, np.int64)
    t = t1.copy()
    t_fin = np.zeros(n, T)
    n_eval, f_last = np.zeros(n, np.int64), np.zeros(n, T)
    have_prev, refine = np.zeros(n, bool), np.zeros(n, bool)
    prev_t, prev_f, ta, fa, tb, fb = (np.zeros(n, T) for _ in range(6))
    k_ref = np.zeros(n, np.int64)

    def finish(rays, st, tf):
        status[rays], t_fin[rays] = st, tf

    bad = ~((t2 >= 0) & np.isfinite(t2))
    finish(every[bad], MISS, T(-1.0))
    with np.errstate(invalid="ignore", over="ignore"):
        while (status < 0).any():
            # every live ray walks to its next evaluation point
            te = t.copy()
            pending = (status < 0) & refine
            te[pending] = T(0.5) * (ta[pending] + tb[pending])
            walk = every[(status < 0) & ~refine]
            while len(walk):
                record(walk, K_T2, (t[walk] - t2[walk]), np.maximum(np.abs(t[walk]), np.abs(t2[walk])))
                out = ~(t[walk] < t2[walk])
                finish(walk[out], MISS, t2[walk[out]])
                walk = walk[~out]
                if not len(walk):
                    break
                occ, xyz, nxyz, mb = grid.probe(o[walk], d[walk], t[walk], T)
                record(walk, K_OCC, t[walk], np.abs(t[walk]), occ)
                full = occ & (n_eval[walk] >= max_evals)
                finish(walk[full], ABANDONED, t[walk[full]])
                go = occ & ~full
                pending[walk[go]] = True
                te[walk[go]] = t[walk[go]]
                e = ~occ
                w = walk[e]
                tn = grid.skip_target(d[w], d_inv[w], t[w], xyz[e], nxyz[e], mb[e], T) + T(DT_MIN)
                have_prev[w] = False
                stuck = ~(tn > t[w])
                finish(w[stuck], ABANDONED, t[w[stuck]])
                t[w[~stuck]] = tn[~stuck]
                walk = w[~stuck]
            p = every[pending]
            if not len(p):
                continue
            f = m.value(o[p] + te[p][:, None] * d[p], T)
            n_eval[p] += 1
            f_last[p] = f
            fin = np.isfinite(f)
            finish(p[~fin], ABANDONED, te[p[~fin]])
            p, f = p[fin], f[fin]
            rf = refine[p]
            # the march
            q, fq = p[~rf], f[~rf]
            record(q, K_EPS, fq - eps, np.maximum(np.abs(fq), fs))
            far = fq > eps
            a = q[far]
            prev_t[a], prev_f[a], have_prev[a] = t[a], fq[far], True
            t[a] = t[a] + np.fmax(fq[far] * step_scale, min_step)
            q, fq = q[~far], fq[~far]
            record(q, K_ZERO, fq, np.maximum(np.abs(fq), fs))
            pos = fq >= 0
            finish(q[pos], HIT, t[q[pos]])
            q, fq = q[~pos], fq[~pos]
            first = ~have_prev[q]
            finish(q[first], INSIDE, t[q[first]])
            q, fq = q[~first], fq[~first]
            ta[q], fa[q], tb[q], fb[q], k_ref[q], refine[q] = prev_t[q], prev_f[q], t[q], fq, 0, True
            # a bisection step
            b, fm = p[rf], f[rf]
            record(b, K_BISECT, fm, np.maximum(np.abs(fm), fs))
            up = fm >= 0
            ta[b[up]], fa[b[up]] = te[b[up]], fm[up]
            tb[b[~up]], fb[b[~up]] = te[b[~up]], fm[~up]
            k_ref[b] += 1
            z = every[(status < 0) & refine & (k_ref >= n_refine)]
            th = ta[z] + ((tb[z] - ta[z]) * fa[z]) / (fa[z] - fb[z])
            ok = np.isfinite(th)
            finish(z[ok], HIT, th[ok])
            finish(z[~ok], ABANDONED, tb[z[~ok]])
        xyz = o + t_fin[:, None] * d
    cols = [np.concatenate(c) for c in zip(*log)]
    order = np.argsort(cols[0], kind="stable")
    return {"status": status, "t": t_fin, "xyz": xyz, "n_eval": n_eval, "f_last": f_last, "t2": t2, "t1": t1,
            "log": tuple(c[order] for c in cols)}


def decide(m, grid, o, d, r64, r32, eps):
    """bool [n]: the rays whose every decision along the float64 path holds with the margin of the module docstring."""
    n = len(r64["status"])
    ray64, kind64, q64, sc64, aux64 = r64["log"]
    ray32, kind32, q32, _, aux32 = r32["log"]
    c64, c32 = np.bincount(ray64, minlength=n), np.bincount(ray32, minlength=n)
    decided = c64 == c32
    s64, s32 = np.concatenate([[0], np.cumsum(c64)]), np.concatenate([[0], np.cumsum(c32)])
    keep = decided[ray64]                                         # align the logs of the rays with equal decision counts
    pos = (np.arange(len(ray64)) - s64[ray64])[keep]
    i64 = np.flatnonzero(keep)
    i32 = s32[ray64[keep]] + pos
    same = (kind64[i64] == kind32[i32]) & ((kind64[i64] != K_OCC) | (aux64[i64] == aux32[i32]))
    margin = 4.0 * np.maximum(np.abs(q32[i32] - q64[i64]), ulp32(sc64[i64]))
    k, q = kind64[i64], q64[i64]
    held = same.copy()
    thr = np.isin(k, (K_T2, K_SLAB, K_EPS, K_ZERO, K_BISECT))     # all of these compare their quantity with 0 (eps is subtracted)
    held &= ~thr | (np.abs(q) > margin)
    oc = np.flatnonzero(k == K_OCC)
    if len(oc):
        rr = ray64[i64][oc]
        o64, d64 = np.asarray(o, np.float32).astype(np.float64)[rr], np.asarray(d, np.float32).astype(np.float64)[rr]
        for sgn in (-1.0, 1.0):
            occ = grid.probe(o64, d64, q[oc] + sgn * margin[oc], np.float64)[0]
            held[oc] &= occ == aux64[i64][oc].astype(bool)
    np.logical_and.at(decided, ray64[i64], held)
    return decided & (r64["status"] == r32["status"]) & (r64["n_eval"] == r32["n_eval"])


class Case:
    """A named set: a model, an occupancy grid, rays, trace parameters.  `only_invariants`: a grazing set."""

    def __init__(self, name, model, grid, o, d, only_invariants=False, **params):
        self.name, self.model, self.grid, self.only_invariants = name, model, grid, only_invariants
        self.o, self.d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        self.params = dict(DEFAULTS, **params)
        self._ref = None

    def ref(self):
        if self._ref is None:
            r64 = trace(self.model, self.grid, self.o, self.d, np.float64, **self.params)
            r32 = trace(self.model, self.grid, self.o, self.d, np.float32, **self.params)
            dec = decide(self.model, self.grid, self.o, self.d, r64, r32, self.params["eps"])
            self._ref = (r64, r32, dec)
        return self._ref

    def undecided_fraction(self):
        return 1.0 - float(self.ref()[2].mean())

    def e32(self):
        """per quantity: the largest |serial32 - float64| over the decided rays, at least one float32 ulp of the quantity's scale."""
        r64, r32, dec = self.ref()
        out = {}
        for k in ("t", "xyz", "f_last"):
            a, b = r64[k][dec].astype(np.float64), r32[k][dec].astype(np.float64)
            fin = np.isfinite(a) & np.isfinite(b)
            scale = np.abs(a[fin]).max() if fin.any() else 1.0
            out[k] = max(float(np.abs(a - b)[fin].max()) if fin.any() else 0.0, float(ulp32(scale)))
        return out


def judge(case, got):
    """got: dict of numpy arrays status, t, xyz, n_eval, f_last.  Asserts the contract on the decided rays; returns the figures."""
    r64, _, dec = case.ref()
    e32 = case.e32()
    assert np.array_equal(got["status"][dec], r64["status"][dec]), "%s: status differs on a decided ray" % case.name
    assert np.array_equal(got["n_eval"][dec], r64["n_eval"][dec]), "%s: n_eval differs on a decided ray" % case.name
    fig = {"undecided": 1.0 - float(dec.mean())}
    for k in ("t", "xyz", "f_last"):
        a, b = np.asarray(got[k], np.float64)[dec], r64[k][dec]
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin), "%s: %s finite where the reference is not, or the reverse" % (case.name, k)
        err = float(np.abs(a - b)[fin].max()) if fin.any() else 0.0
        fig[k] = err / e32[k]
        assert err <= 4.0 * e32[k], "%s: %s off by %.3g = %.2f x E32 (bound 4)" % (case.name, k, err, err / e32[k])
    return fig


def invariants(case, got):
    """What holds for ANY output of the kernel on this case, undecided rays included."""
    st, t, xyz, ne = got["status"], got["t"].astype(np.float32), got["xyz"].astype(np.float32), got["n_eval"]
    assert ((st >= 0) & (st <= 3)).all(), "%s: status outside 0..3" % case.name
    with np.errstate(invalid="ignore", over="ignore"):
        want = case.o + t[:, None] * case.d                       # float32: a multiply, then an add, as the kernel forms it
    assert np.array_equal(xyz, want, equal_nan=True), "%s: xyz is not o + t d" % case.name
    r64 = case.ref()[0]
    t1, t2 = r64["t1"].astype(np.float32), r64["t2"].astype(np.float32)
    slab_miss = (st == MISS) & (t == -1.0)
    tol = 4 * np.spacing(np.maximum(np.abs(t1), np.abs(t2)))      # t1, t2 here are float64 roundings of what the kernel computes
    inside = (t >= t1 - tol) & (t <= t2 + tol)
    no_interval = (st == MISS) & ~(t1 + tol < t2 - tol)            # the slab's entry lies behind its exit: a miss on the slab too
    assert (inside | slab_miss | no_interval).all(), "%s: t outside [t1, t2]" % case.name
    assert (ne >= 0).all() and (ne <= case.params["max_evals"] + case.params["n_refine"]).all(), "%s: n_eval beyond max_evals + n_refine" % case.name
    assert (ne[slab_miss] == 0).all()


# ---- the named sets --------------------------------------------------------------------------------------------------------------------
def make_model(levels, bfhl, n_entries, width, depth, scale, seed, amplitude=0.05, radius=0.25, decay=False):
    """geometric initialisation + a table of U(-amplitude, amplitude); decay: a level's amplitude falls with its resolution, as in a
    trained field (at a resolution of 2048 a constant amplitude is a slope of 100, and f amplifies every rounding of the position)."""
    rng = np.random.default_rng(seed)
    table = rng.uniform(-amplitude, amplitude, (n_entries, 2)).astype(np.float32)
    if decay:
        for l in range(len(levels[1])):
            a, b = int(levels[3][l]), int(levels[3][l]) + int(levels[2][l])
            table[a:b] *= np.float32(float(levels[1][0]) / float(levels[1][l]))
    return Model(levels, bfhl, table, geometric_layers(rng, 3 + 2 * len(levels[0]), width, depth, radius), scale)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def rays_at(rng, n, dist, r_aim_lo, r_aim_hi, lo=0.35, mixed=False):
    """n rays that pass a point at a distance in [r_aim_lo, r_aim_hi] from the centre, starting `dist` before it.  The direction
    components are drawn from [lo, 1] before normalisation and are all POSITIVE unless `mixed`: an empty-cell skip along a
    negative component is the march's (nxyz + 0) / G * 2 - 1) * mip_bound - xyz, zero in exact arithmetic and rounding noise over
    d_k in float32, so on such rays float32 and float64 drift apart by 1e-5 over a hundred skips and a fixed share of all
    occupancy transitions falls inside the margin.  With positive components every skip is a whole cell."""
    u = rng.uniform(lo, 1.0, (n, 3))
    if mixed:
        u = u * rng.choice([-1.0, 1.0], (n, 3))
    d = _unit(u)
    aim = _unit(rng.standard_normal((n, 3))) * rng.uniform(r_aim_lo, r_aim_hi, (n, 1))
    d32 = _unit(d.astype(np.float32).astype(np.float64)).astype(np.float32)
    return (aim - dist * d).astype(np.float32), d32


def case_table(model, G=32, seed=11):
    """The named sets on one model (box scale model.scale): every branch of the rule."""
    rng = np.random.default_rng(seed)
    s = model.scale
    shell = Grid(shell_bitfield(s, G, 0.10, 0.42), s, G)
    ones = Grid(np.full(cascades_of(s) * G**3 // 8, 255, np.uint8), s, G)
    zeros = Grid(np.zeros(cascades_of(s) * G**3 // 8, np.uint8), s, G)
    cases = []
    for n in (1, 63, 64, 65, 1153):
        o, d = rays_at(rng, n, 1.2 + s, 0.0, 0.2)
        cases.append(Case("threshold_shell_n%d" % n, model, shell, o, d, eps=1e-3, min_step=0.0))
    o, d = rays_at(rng, 257, 1.2 + s, 0.0, 0.2)
    cases.append(Case("threshold_ones", model, ones, o, d, eps=1e-3, min_step=0.0))
    # eight bisections bring |fm| down to the slope times 2^-8 of a step: the sign stays decided only while float32 and float64 agree
    # on t to a few ulp, which they do where no skip has drifted them apart -- that set runs on the full grid
    for nr in (0, 1, 8):
        cases.append(Case("crossing_refine%d" % nr, model, ones if nr == 8 else shell, o, d, eps=0.0, n_refine=nr))
    cases.append(Case("defaults_ones", model, ones, o, d))
    cases.append(Case("all_zeros", model, zeros, o, d))
    oi, di = rays_at(rng, 130, 0.0, 0.0, 0.08)
    cases.append(Case("inside_ones", model, ones, oi, di))
    cases.append(Case("inside_shell", model, shell, oi, di))
    cases.append(Case("abandoned_max3", model, ones, o, d, max_evals=3))
    om, dm = rays_at(rng, 130, 1.2 + s, 2.5 * s, 4.0 * s)
    cases.append(Case("miss_slab", model, ones, om, dm))
    op, dp = rays_at(rng, 130, 1.2 + s, 0.36, 0.40)
    cases.append(Case("miss_past_surface", model, ones, op, dp))
    oz = np.array([[0.03, -1.3, 0.02], [0.0, 0.05, -1.4], [-1.5, 0.0, 0.0], [0.04, -0.9, -1.2]], np.float32)
    dz = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.6, 0.8]], np.float32)
    cases.append(Case("zero_component", model, ones, oz, dz))
    og, dg = rays_at(rng, 257, 1.2 + s, 0.2, 0.3)
    cases.append(Case("grazing", model, shell, og, dg, only_invariants=True))
    ox, dx = rays_at(rng, 257, 1.2 + s, 0.0, 0.3, mixed=True)
    cases.append(Case("mixed_signs", model, shell, ox, dx, only_invariants=True))
    return cases


def default_arch_case(levels, bfhl, n_entries, G=32):
    """65 rays on the default architecture (16 levels, width 64, depth 2), the threshold path on the full grid."""
    model = make_model(levels, bfhl, n_entries, 64, 2, 0.5, seed=5, amplitude=0.1, decay=True)
    o, d = rays_at(np.random.default_rng(21), 65, 1.7, 0.0, 0.2)
    return Case("default_arch_threshold", model, Grid(np.full(G**3 // 8, 255, np.uint8), 0.5, G), o, d, eps=1e-3, min_step=0.0)


def eval_points(rng, n, scale):
    """n positions: the box's interior, its faces, cell corners of the coarse levels, and outside the box (in that order, cyclically)."""
    kinds = np.arange(n) % 4
    x = rng.uniform(-scale, scale, (n, 3))
    face = rng.integers(0, 3, n)
    x[kinds == 1, face[kinds == 1]] = rng.choice([-scale, scale], (kinds == 1).sum())
    x[kinds == 2] = (rng.integers(0, 9, ((kinds == 2).sum(), 3)) / 8.0 * 2 - 1) * scale
    x[kinds == 3] = rng.uniform(-4 * scale, 4 * scale, ((kinds == 3).sum(), 3))
    return x.astype(np.float32)
