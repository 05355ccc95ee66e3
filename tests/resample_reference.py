"""Float64 evaluation of the importance-resampling contract (include/ngp_hip.h, "importance resampling"), its serial float32
evaluation, and the yardstick the kernels of csrc/resample.hip are held to (tests/test_resample_reference.py on the CPU,
tests/test_gpu_resample.py on the GPU).  numpy only.

The contract, per ray: w_j = max(ws_j, 0) + floor; c = cumsum(w); draw k has target = (k + noise) / K * c_last, lands in the first
section j with c_j > target at t* = lo_j + (target - c_{j-1}) / w_j * delta_j, and is KEPT iff lo_j < t* < hi_j and t* differs from
the previous draw's; a section with m kept cuts becomes m + 1 children (edges lo, cuts.., hi; t = (a + b) / 2, delta = b - a), a section
without a cut is copied.  A ray with N = 0, a non-finite weight or c_last not > 0 is copied through.

  refine_ray(ray, K, floor, dt)   the contract for one ray in the number format dt: np.float64 (the model) or np.float32 (every rounding
                                  a separate float32 operation, the CDF summed serially left to right).  One function, two formats.
  decide(ray, K, floor)           which draws are DECIDED: in float64, target is further than 4 E32_cdf from both CDF edges of its section,
                                  and t* further than that margin, mapped to t, from lo, hi and the previous draw's cut in the section.
                                  E32_cdf is the error of the serial float32 evaluation against float64 on that ray: the largest
                                  |c32_j - c64_j| and |target32_k - target64_k|, with a floor of one float32 ulp of c_last (any float32
                                  CDF, whatever its summation order, is at least that far off).  Mapped to t the margin is
                                  4 (E32_cdf delta_j / w_j + ulp32(hi_j)): the second term is the rounding of lo, hi and t* themselves.
                                  A ray is decided when all its draws are.
  case_e32 / judge                the project's yardstick on decided rays: counts, parent and rays_a' exact, and
                                  |got - f64| <= 4 E32 scale for ts, deltas, xyzs, E32 = max |serial32 - f64| / scale over the named set
                                  with a floor of one ulp (2^-23).  Scales: an edge of a cut section j is uncertain by the CDF's error
                                  times delta_j / w_j, so ts and deltas of its children have the scale hi_j + delta_j c_last / w_j; the
                                  child of an uncut section is a copy (scale hi_j; it must in fact be exact); xyz_a has |o_a| + scale |d_a|.
  invariants                      what must hold for ANY evaluation's own output, undecided draws included: ts strictly increasing,
                                  deltas > 0, parent non-decreasing and naming every section, the children's deltas summing to the
                                  parent's within 4 ulps of hi per child (an edge is a float32 number of the size of t, so that is the
                                  ulp that counts, not delta's), copied rays bit-identical.
"""
import numpy as np

F = np.float32
K_YARD = 4
ULP = 2.0 ** -23
SENTINEL = -7.0e33
MAX_UNDECIDED = 0.02


def ulp32(x):
    return float(np.spacing(F(abs(float(x)))))


class Ray:
    """ws, deltas, ts [N] float32, o, d [3] float32, noise float32 in [0, 1), name."""

    def __init__(self, name, ws, deltas, ts, o, d, noise):
        self.name = name
        self.ws, self.deltas, self.ts = (np.ascontiguousarray(x, F) for x in (ws, deltas, ts))
        self.o, self.d, self.noise = np.asarray(o, F), np.asarray(d, F), F(noise)
        self.N = len(self.ws)
        assert len(self.deltas) == self.N == len(self.ts) and 0.0 <= float(self.noise) < 1.0


def refine_ray(ray, K, floor, dt):
    """-> dict: passthrough, c [N] (the CDF), w [N], target, tstar [K], sec [K] (N = dropped), kept [K] bool, and the children:
    ts, deltas [N'], parent [N'] (section index within the ray), lo, hi [N'] (their edges), xyzs [N', 3]."""
    N = ray.N
    x = ray.ws.astype(dt)
    half = dt(0.5)
    t_in, d_in = ray.ts.astype(dt), ray.deltas.astype(dt)
    lo_e, hi_e = t_in - half * d_in, t_in + half * d_in
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = np.where(x < 0, dt(0), x) + dt(F(floor))
        c = np.cumsum(w, dtype=dt)                            # sequential: c_j = c_{j-1} + w_j, one rounding each
        c_last = c[-1] if N else dt(0)
        through = N == 0 or not np.all(np.isfinite(x)) or not (c_last > 0) or not np.isfinite(c_last)
        target, tstar = np.full(K, np.nan, dt), np.full(K, np.nan, dt)
        sec, kept = np.full(K, N, np.int64), np.zeros(K, bool)
        if not through:
            for k in range(K):
                u = (dt(k) + dt(ray.noise)) / dt(K)
                target[k] = u * c_last
                j = int(np.searchsorted(c, target[k], side="right"))      # the first c_j > target
                sec[k] = j
                if j >= N:
                    continue
                c_prev = c[j - 1] if j > 0 else dt(0)
                tstar[k] = lo_e[j] + (target[k] - c_prev) / w[j] * d_in[j]
                kept[k] = lo_e[j] < tstar[k] < hi_e[j] and not (k > 0 and tstar[k] == tstar[k - 1])
    ts, dl, parent, los, his = [], [], [], [], []
    ks = np.flatnonzero(kept)
    for j in range(N):
        cuts = [tstar[k] for k in ks[sec[ks] == j]]
        if not cuts:
            ts.append(t_in[j]); dl.append(d_in[j]); parent.append(j); los.append(lo_e[j]); his.append(hi_e[j])
            continue
        edges = [lo_e[j]] + cuts + [hi_e[j]]
        for a, b in zip(edges[:-1], edges[1:]):
            ts.append(half * (a + b)); dl.append(b - a); parent.append(j); los.append(a); his.append(b)
    ts, dl, los, his = (np.asarray(v, dt).reshape(-1) for v in (ts, dl, los, his))
    xyzs = ray.o.astype(dt)[None, :] + ts[:, None] * ray.d.astype(dt)[None, :]
    return dict(passthrough=bool(through), c=c, w=w, c_last=c_last, target=target, tstar=tstar, sec=sec, kept=kept, ts=ts, deltas=dl,
                parent=np.asarray(parent, np.int64).reshape(-1), lo=los, hi=his, xyzs=xyzs, lo_e=lo_e, hi_e=hi_e)


def decide(ray, K, floor, r64=None, r32=None):
    """-> dict decided [K] bool, e32_cdf, ray_decided.  A copied-through ray has no draws to decide unless a float32 evaluation could
    disagree about copying it (c_last within the margin of 0): none of the named sets has such a ray."""
    r64 = refine_ray(ray, K, floor, np.float64) if r64 is None else r64
    r32 = refine_ray(ray, K, floor, F) if r32 is None else r32
    if r64["passthrough"]:
        return dict(decided=np.ones(K, bool), e32_cdf=0.0, ray_decided=bool(r32["passthrough"]))
    with np.errstate(invalid="ignore"):
        e = max(float(np.max(np.abs(r32["c"].astype(np.float64) - r64["c"]))),
                float(np.nanmax(np.abs(r32["target"].astype(np.float64) - r64["target"]))), ulp32(r64["c_last"]))
    m = K_YARD * e
    decided = np.zeros(K, bool)
    N = ray.N
    for k in range(K):
        j, tg = int(r64["sec"][k]), r64["target"][k]
        if j >= N:
            continue
        c_prev = r64["c"][j - 1] if j > 0 else 0.0
        if not (tg - c_prev > m and r64["c"][j] - tg > m):
            continue
        mt = K_YARD * (e * float(ray.deltas[j]) / r64["w"][j] + ulp32(r64["hi_e"][j]))
        ts_ = r64["tstar"][k]
        if not (ts_ - r64["lo_e"][j] > mt and r64["hi_e"][j] - ts_ > mt):
            continue
        if k > 0 and r64["sec"][k - 1] == j and not (ts_ - r64["tstar"][k - 1] > mt):
            continue
        decided[k] = True
    return dict(decided=decided, e32_cdf=e, ray_decided=bool(decided.all()))


# ------------------------------------------------------------------------------------------------------------------ named sets
class Case:
    def __init__(self, name, rays, K, floor=0.0, tie=False):
        self.name, self.rays, self.K, self.floor, self.tie = name, rays, int(K), float(floor), tie
        self._ref = None

    def ref(self):
        """(r64, r32, decision) per ray, computed once."""
        if self._ref is None:
            out = []
            for ray in self.rays:
                r64, r32 = refine_ray(ray, self.K, self.floor, np.float64), refine_ray(ray, self.K, self.floor, F)
                out.append((r64, r32, decide(ray, self.K, self.floor, r64, r32)))
            self._ref = out
        return self._ref

    def undecided_fraction(self):
        dec = [d["decided"] for r64, _, d in self.ref() if not r64["passthrough"]]
        return float(np.mean(~np.concatenate(dec))) if dec else 0.0


def _track(rng, N, gaps=False):
    pos = 0.05 + 0.45 * rng.random()
    t, dl = np.zeros(N), np.zeros(N)
    for j in range(N):
        dl[j] = 1.7e-3 * (1.0 + 0.3 * rng.random())
        t[j] = pos + 0.5 * dl[j]
        pos += dl[j]
        if gaps and rng.random() < 0.3:
            pos += 1e-2 * rng.random()
    return t.astype(F), dl.astype(F)


def _od(rng):
    d = rng.standard_normal(3)
    return (rng.random(3) - 0.5).astype(F), (d / np.linalg.norm(d)).astype(F)


def _bump(rng, N, width=None):
    """A NeuS-like weight: a shell a few sections wide somewhere along the ray, exact zeros elsewhere."""
    if N == 0:
        return np.zeros(0, F)
    j0 = rng.random() * N
    s = min(max(N / 8.0, 1.0), 6.0) if width is None else width
    w = np.exp(-0.5 * ((np.arange(N) - j0) / s) ** 2) * (0.2 + 0.8 * rng.random())
    w[w < 1e-2 * w.max()] = 0.0
    return w.astype(F)


def _ray(rng, name, N, ws=None, gaps=False, noise=None):
    t, dl = _track(rng, N, gaps)
    o, d = _od(rng)
    nz = F(0.05 + 0.9 * rng.random()) if noise is None else noise
    return Ray(name, _bump(rng, N) if ws is None else ws, dl, t, o, d, nz)


LENGTHS = (0, 1, 63, 64, 65, 129, 1024)
KS = (1, 7, 64, 65, 128)
RAY_COUNTS = (1, 4, 5, 37)


def case_table():
    """name -> Case; every ray is generated once from a fixed seed."""
    if _TABLE:
        return _TABLE
    T = _TABLE
    for K in KS:
        rng = np.random.default_rng(300 + K)
        T["lengths_K%d" % K] = Case("lengths_K%d" % K, [_ray(rng, "N%d" % N, N) for N in LENGTHS], K)
    for n in RAY_COUNTS:
        rng = np.random.default_rng(320 + n)
        T["rays%d" % n] = Case("rays%d" % n, [_ray(rng, "r%d_N" % i, int(rng.integers(1, 150))) for i in range(n)], 7)
    rng = np.random.default_rng(330)
    rays = []
    for N, j in ((1, 0), (64, 63), (65, 64), (130, 0), (130, 77)):
        ws = np.zeros(N, F); ws[j] = 0.7
        rays.append(_ray(rng, "one_N%d_j%d" % (N, j), N, ws))
    T["one_section"] = Case("one_section", rays, 64)
    rng = np.random.default_rng(331)
    rays = []
    for N in (5, 64, 129, 200):
        ws = (0.1 + rng.random(N)).astype(F); ws[rng.random(N) < 0.6] = 0.0; ws[N // 2] = 0.5
        rays.append(_ray(rng, "zeros_N%d" % N, N, ws))
    T["zeros_interleaved"] = Case("zeros_interleaved", rays, 65)
    rng = np.random.default_rng(332)
    rays = []
    for N in (3, 70, 129):
        ws = _bump(rng, N, 4.0); neg = ws == 0; ws[neg] = -(0.1 + rng.random(int(neg.sum()))).astype(F); ws[N // 2] = 0.3
        rays.append(_ray(rng, "neg_N%d" % N, N, ws))
    rays.append(_ray(rng, "allneg_N40", 40, -np.ones(40, F)))                    # every weight clamps to 0: copied through
    T["negative"] = Case("negative", rays, 7)
    rng = np.random.default_rng(333)
    T["floor"] = Case("floor", [_ray(rng, "zero_N37", 37, np.zeros(37, F)), _ray(rng, "zero_N64", 64, np.zeros(64, F)),
                                _ray(rng, "bump_N90", 90)], 7, floor=1e-5)
    rng = np.random.default_rng(334)
    T["zero_ray"] = Case("zero_ray", [_ray(rng, "bump_N50", 50), _ray(rng, "zero_N70", 70, np.zeros(70, F)), _ray(rng, "bump_N66", 66)], 7)
    rng = np.random.default_rng(335)
    T["gaps"] = Case("gaps", [_ray(rng, "gap_N%d" % N, N, gaps=True) for N in (2, 40, 64, 65, 200)], 64)
    rng = np.random.default_rng(336)
    rays = []
    for i in range(9):                                      # every other ray has weight everywhere: the CDF's carry crosses groups
        N = int(rng.integers(1, 300))
        rays.append(_ray(rng, "perm%d_N%d" % (i, N), N, (0.05 + rng.random(N)).astype(F) if i % 2 else None))
    T["permuted"] = Case("permuted", rays, 7)
    rng = np.random.default_rng(337)
    rays = [_ray(rng, "fin%d" % i, int(rng.integers(1, 150))) for i in range(6)]
    ws = _bump(rng, 100); ws[17] = np.nan
    rays.insert(2, _ray(rng, "nan_N100", 100, ws))
    ws = _bump(rng, 70); ws[69] = np.inf
    rays.insert(5, _ray(rng, "inf_N70", 70, ws))
    T["nan"] = Case("nan", rays, 7)
    rng = np.random.default_rng(339)
    T["K256"] = Case("K256", [_ray(rng, "k256_N%d" % N, N) for N in (3, 65, 300)], 256)
    rng = np.random.default_rng(340)
    # longer than the march's max_samples (1024): the count kernel keeps such a ray's CDF in global memory instead of LDS
    T["long"] = Case("long", [_ray(rng, "long_N1025", 1025), _ray(rng, "short_N30", 30),
                              _ray(rng, "long_N1500", 1500, (0.05 + rng.random(1500)).astype(F) * (rng.random(1500) < 0.1))], 65)
    rng = np.random.default_rng(338)
    # noise exactly 0: draw 0 has target 0 = the lower CDF edge of its section (t* = lo: not kept) -- a tie by construction, so this
    # set is asserted on its decided draws only
    T["noise0"] = Case("noise0", [_ray(rng, "nz0_N%d" % N, N, noise=F(0.0)) for N in (1, 64, 100)], 7, tie=True)
    return T


_TABLE = {}


# ------------------------------------------------------------------------------------------------------------------ buffer layout
class Layout:
    """The buffers the kernels see for a named set: row r of rays_a is ray r with the ray index ray_idx[r] (a sample of a permutation of
    range(n + 3): rays_o / rays_d / noise have rows no ray uses), the sample ranges allocated in yet another order with 0-5 unused
    samples between them and 16 spare ones at the end.  Unused entries hold finite junk."""

    def __init__(self, case, seed):
        rng = np.random.default_rng(seed)
        rays = case.rays
        n = len(rays)
        self.case, self.n, self.n_orig = case, n, n + 3
        self.ray_idx = rng.permutation(self.n_orig)[:n].astype(np.int32)
        self.N = np.array([r.N for r in rays], np.int32)
        self.start, pos = np.zeros(n, np.int32), 0
        for r in rng.permutation(n):
            pos += int(rng.integers(0, 6))
            self.start[r] = pos
            pos += rays[r].N
        self.S = pos + 16
        self.rays_a = np.stack([self.ray_idx, self.start, self.N], 1).astype(np.int32)
        self.ws, self.deltas, self.ts = np.full(self.S, 0.25, F), np.full(self.S, 0.01, F), np.full(self.S, 1.0, F)
        self.rays_o, self.rays_d, self.noise = np.full((self.n_orig, 3), 0.1, F), np.full((self.n_orig, 3), 0.5, F), np.full(self.n_orig, 0.5, F)
        for r, ray in enumerate(rays):
            s = slice(self.start[r], self.start[r] + ray.N)
            self.ws[s], self.deltas[s], self.ts[s] = ray.ws, ray.deltas, ray.ts
            self.rays_o[self.ray_idx[r]], self.rays_d[self.ray_idx[r]], self.noise[self.ray_idx[r]] = ray.o, ray.d, ray.noise

    def split(self, rays_a_out, ts, deltas, parent, xyzs, dirs=None):
        """Flat outputs -> one dict per row: ts, deltas, parent (section index within the ray), xyzs, dirs."""
        out = []
        for r in range(self.n):
            s = slice(int(rays_a_out[r, 1]), int(rays_a_out[r, 1]) + int(rays_a_out[r, 2]))
            out.append(dict(ts=ts[s], deltas=deltas[s], parent=parent[s].astype(np.int64) - int(self.start[r]), xyzs=xyzs[s],
                            dirs=None if dirs is None else dirs[s]))
        return out


def expected_rays_a(lay, counts):
    counts = np.asarray(counts, np.int64)
    return np.stack([lay.ray_idx.astype(np.int64), np.concatenate([[0], np.cumsum(counts)[:-1]]), counts], 1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def _scales(ray, r64):
    """Per child of the float64 evaluation: the scale of ts and deltas, and of xyzs [N', 3]."""
    j = r64["parent"]
    cut = np.bincount(j, minlength=ray.N)[j] > 1 if len(j) else np.zeros(0, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.where(cut, ray.deltas.astype(np.float64)[j] * r64["c_last"] / r64["w"][j], 0.0)
    st = np.abs(r64["hi_e"][j]) + amp
    sx = np.abs(ray.o.astype(np.float64))[None, :] + st[:, None] * np.abs(ray.d.astype(np.float64))[None, :]
    return st, sx


def case_e32(case):
    """E32 of ts, deltas, xyzs over the decided rays of the set (floor: one ulp).  The serial float32 evaluation must itself make the
    float64 decisions on a decided ray -- that is what decided means; asserted here."""
    e = dict(ts=ULP, deltas=ULP, xyzs=ULP)
    for ray, (r64, r32, d) in zip(case.rays, case.ref()):
        if not d["ray_decided"] or len(r64["ts"]) == 0:
            continue
        assert np.array_equal(r64["parent"], r32["parent"]), "serial float32 disagrees with float64 on the decided ray %s" % ray.name
        st, sx = _scales(ray, r64)
        e["ts"] = max(e["ts"], float(np.max(np.abs(r32["ts"] - r64["ts"]) / st)))
        e["deltas"] = max(e["deltas"], float(np.max(np.abs(r32["deltas"] - r64["deltas"]) / st)))
        e["xyzs"] = max(e["xyzs"], float(np.max(np.abs(r32["xyzs"] - r64["xyzs"]) / sx)))
    return e


def judge(case, got, e32):
    """got: one dict per ray (Layout.split).  -> (failures, worst ratio |got - f64| / (E32 scale) per quantity, decided rays judged)."""
    fails, worst, judged = [], dict(ts=0.0, deltas=0.0, xyzs=0.0), 0
    for ray, g, (r64, _, d) in zip(case.rays, got, case.ref()):
        if not d["ray_decided"]:
            continue
        judged += 1
        if len(g["ts"]) != len(r64["ts"]) or not np.array_equal(g["parent"], r64["parent"]):
            fails.append("%s: %d children, parents %s; float64 has %d" % (ray.name, len(g["ts"]), g["parent"][:8], len(r64["ts"])))
            continue
        if len(r64["ts"]) == 0:
            continue
        st, sx = _scales(ray, r64)
        for q, sc in (("ts", st), ("deltas", st), ("xyzs", sx)):
            ratio = float(np.max(np.abs(np.asarray(g[q], np.float64) - r64[q]) / (e32[q] * sc)))
            worst[q] = max(worst[q], ratio)
            if not ratio <= K_YARD:
                fails.append("%s: %s is %.3g E32 scale off the float64 model (allowed %d)" % (ray.name, q, ratio, K_YARD))
    return fails, worst, judged


def invariants(case, got):
    """Failures of the properties every evaluation's own output must have, undecided draws included."""
    fails = []
    for ray, g, (r64, _, _) in zip(case.rays, got, case.ref()):
        ts, dl, par = np.asarray(g["ts"]), np.asarray(g["deltas"]), np.asarray(g["parent"])
        if len(ts) < ray.N or len(ts) > ray.N + case.K:
            fails.append("%s: %d children of %d sections with K = %d" % (ray.name, len(ts), ray.N, case.K))
            continue
        if ray.N == 0:
            continue
        if not np.all(np.diff(ts) > 0):
            fails.append("%s: ts is not strictly increasing" % ray.name)
        if not np.all(dl > 0):
            fails.append("%s: a delta is not > 0" % ray.name)
        if not (np.all(np.diff(par) >= 0) and np.array_equal(np.unique(par), np.arange(ray.N))):
            fails.append("%s: parent is not non-decreasing over every section" % ray.name)
            continue
        m = np.bincount(par, minlength=ray.N)
        tot = np.bincount(par, weights=dl.astype(np.float64), minlength=ray.N)
        hi = ray.ts.astype(np.float64) + 0.5 * ray.deltas.astype(np.float64)
        tol = 4.0 * m * np.array([ulp32(h) for h in hi])
        if not np.all(np.abs(tot - ray.deltas.astype(np.float64)) <= tol):
            fails.append("%s: the children's deltas do not sum to the parent's within 4 ulps per child" % ray.name)
        single = m[par] == 1
        if not (np.array_equal(ts[single].astype(F).view(np.uint32), ray.ts[par[single]].view(np.uint32))
                and np.array_equal(dl[single].astype(F).view(np.uint32), ray.deltas[par[single]].view(np.uint32))):
            fails.append("%s: an uncut section is not a bit-identical copy" % ray.name)
        if r64["passthrough"] and len(ts) != ray.N:
            fails.append("%s: a ray that must be copied through was cut" % ray.name)
        if g.get("dirs") is not None and not np.array_equal(np.ascontiguousarray(g["dirs"], F).view(np.uint32),
                                                             np.tile(ray.d, (len(ts), 1)).view(np.uint32)):
            fails.append("%s: dirs is not the ray's direction" % ray.name)
    return fails
