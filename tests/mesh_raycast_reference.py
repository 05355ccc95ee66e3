"""numpy reference of the ray-casting contract (include/ngp_hip.h, "ray casting against a triangle mesh"; csrc/mesh_raycast.hip): a brute
force over ALL faces, no hierarchy, in two arithmetics that run the same code.  The meshes are those of tests/mesh_sdf_reference.py.

  np.float64   the truth
  np.float32   the kernel's ray / face formula restated operation for operation (numpy's float32 operations are IEEE binary32, one
               rounding each), including the float64 recomputation of the edge functions where one is exactly 0; it gives E32, the
               error a correct float32 evaluation has on a set

E32_t = max |t32 - t64| over the rays of the set on which both brute forces return the same face, at least one float32 ulp of the largest
float64 t of the set; E32_b the same for the barycentrics (float64 ON FLOAT32'S FACE), at least one ulp of 1.  Bounds: B = 4 x E32.

THE MARGIN.  The signs of U, V, W are exact for the 2-D corners the float32 formula computes (csrc/mesh_raycast.hip), so float32 tests
the origin of the sheared plane against a triangle whose corners are moved.  A sheared coordinate such as Bx = B[kx] - Sx B[kz] carries the
roundings of B = b - o, of Sx, of the product and of the difference: at most 4 x 2^-24 x R per coordinate, R = the largest |corner - o|
component of the face.  The margin is
    rho = MARGIN x 2^-24 x R,    MARGIN = 16        (4 sqrt(2) is the count above for the two coordinates of a corner; not tuned)
and, on the normalised edge functions e = (U, V, W) / det of float64 (the barycentrics: inside means all >= 0), m_i = rho |edge_i| / |det|:
e_i > m_i says the origin is farther than rho from the line of edge i.  A face is CLEARLY MISSED by a ray when float64 rejects it and the
origin is farther than rho from its outline (the three 2-D segments), CLEARLY HIT when every e_i > m_i, t64 lies in [t_min + B_t, t_max -
B_t] and the face is not culled.  A culled face is out of the question only where the three m_i sum to less than 1 (the corners cannot
move enough to turn the sign of det).

DECIDED.  A ray is decided when every face that could be its first hit is clearly hit or clearly missed.  A face could be the first hit
when its float64 t (formed whatever the signs of e) is not finite, or lies in [t_min - B_t, t_max + B_t] and not more than B_t beyond the
t of the nearest clearly hit face.  judge() asserts on decided rays: hit or miss exact; |t - t64| <= B_t; the returned face's float64 t is
within B_t of the minimum and the face is not clearly missed; bary within B_b of float64 on the returned face; side exact where the
returned face is clearly hit (its |cos| then exceeds the margin).  On undecided rays: every output is finite or the miss encoding, and a
reported hit's t is within B_t of the float64 t of some face that is not clearly missed -- or, for a face whose float64 t is not finite or
whose m_i exceed 1 (the ray lies in its plane: no t to compare with), within B_t of the range of its corners' parameters Az, Bz, Cz,
of which any computed t is a weighted mean.  Printed, not asserted: the number of rays whose t differs in bits from the float32 brute force.
MAX_UNDECIDED is a condition on the sets, not a measurement: tests/test_mesh_raycast_reference.py asserts it for the reference alone."""
import numpy as np

import mesh_sdf_reference as M

EPS = 2.0**-24
MAX_UNDECIDED = 0.02
MARGIN = 16.0
ANY_HIT, CULL_BACK, CULL_FRONT = 1, 2, 4


def ulp32(x):
    return M.ulp32(x)


def _pick(a, k):
    """a [..., 3], k int [n] (the leading axis of a) -> a[..., k]."""
    k = k.reshape(k.shape + (1,) * (a.ndim - k.ndim))
    return np.take_along_axis(a, np.broadcast_to(k, a.shape[:-1] + (1,)), -1)[..., 0]


def setup(o, d, T):
    """The per-ray constants of csrc/mesh_raycast.hip in the arithmetic T -> dict(o, kx, ky, kz, sx, sy, sz, valid)."""
    o, d = np.asarray(o, np.float32).astype(T), np.asarray(d, np.float32).astype(T)
    ad = np.abs(d)
    finite = np.isfinite(d).all(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        kz = np.zeros(len(d), np.int64)
        kz[ad[:, 1] > ad[:, 0]] = 1
        kz[ad[:, 2] > np.maximum(ad[:, 0], ad[:, 1])] = 2
        dz = _pick(d, kz)
        valid = finite & (np.abs(dz) > 0)
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        swap = dz < 0
        kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
        sx, sy, sz = _pick(d, kx) / dz, _pick(d, ky) / dz, T(1.0) / dz
    return dict(o=o, kx=kx, ky=ky, kz=kz, sx=sx, sy=sy, sz=sz, valid=valid)


def _rows(r, rows):
    return {k: v[rows] for k, v in r.items()}


def ray_face(r, a, b, c, T, cull=0, margins=False):
    """The per-face formula of csrc/mesh_raycast.hip: r = setup() of n rays, a, b, c [n,3] or [1 or n,F,3] -> dict(t: NaN where the face
    is rejected, t_raw: T / det whatever the signs, v, w, det); margins (float64): also e [..., 3], m [..., 3], zlo, zhi."""
    a, b, c = (np.asarray(x, np.float32).astype(T) for x in (a, b, c))
    ex = (lambda x: x[:, None]) if a.ndim == 3 else (lambda x: x)
    o = r["o"][:, None, :] if a.ndim == 3 else r["o"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        A, B, C = a - o, b - o, c - o
        sx, sy, sz = ex(r["sx"]), ex(r["sy"]), ex(r["sz"])
        akz, bkz, ckz = _pick(A, r["kz"]), _pick(B, r["kz"]), _pick(C, r["kz"])
        ax, ay = _pick(A, r["kx"]) - sx * akz, _pick(A, r["ky"]) - sy * akz
        bx, by = _pick(B, r["kx"]) - sx * bkz, _pick(B, r["ky"]) - sy * bkz
        cx, cy = _pick(C, r["kx"]) - sx * ckz, _pick(C, r["ky"]) - sy * ckz
        U, V, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
        if T is np.float32:
            zero = (U == 0) | (V == 0) | (W == 0)
            if zero.any():
                D = np.float64
                U = np.where(zero, (cx.astype(D) * by.astype(D) - cy.astype(D) * bx.astype(D)).astype(T), U)
                V = np.where(zero, (ax.astype(D) * cy.astype(D) - ay.astype(D) * cx.astype(D)).astype(T), V)
                W = np.where(zero, (bx.astype(D) * ay.astype(D) - by.astype(D) * ax.astype(D)).astype(T), W)
        det = (U + V) + W
        az, bz, cz = sz * akz, sz * bkz, sz * ckz
        t_raw = ((U * az + V * bz) + W * cz) / det
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        culled = (bool(cull & CULL_BACK) & (det < 0)) | (bool(cull & CULL_FRONT) & (det > 0))
        t = np.where(mixed | (det == 0) | culled | ~ex(r["valid"]), T(np.nan), t_raw)
        out = dict(t=t, t_raw=t_raw, v=V / det, w=W / det, det=det)
        if margins:
            rho = MARGIN * EPS * np.max(np.abs(np.stack([A, B, C], -1)), axis=(-1, -2))
            P = np.stack([np.stack([bx, by], -1), np.stack([cx, cy], -1), np.stack([ax, ay], -1)], -2)       # edge i runs from P[i] to Q[i],
            Q = np.roll(P, -1, axis=-2)                                                                        # opposite a, b, c: U, V, W
            E = Q - P
            length2 = (E * E).sum(-1)
            along = np.clip(np.nan_to_num(-(P * E).sum(-1) / length2), 0.0, 1.0)
            gap = np.sqrt(((P + along[..., None] * E)**2).sum(-1)).min(-1)                                     # the origin to the outline
            out["e"] = np.stack([U, V, W], -1) / det[..., None]
            out["m"] = rho[..., None] * np.sqrt(length2) / np.abs(det)[..., None]
            out["clear_miss"] = (mixed | (det == 0)) & (gap > rho)
            out["zlo"], out["zhi"] = np.minimum(np.minimum(az, bz), cz), np.maximum(np.maximum(az, bz), cz)
            out["culled"] = culled
    return out


def _accepted(t, t_min, t_max):
    with np.errstate(invalid="ignore"):
        return (t >= t_min) & (t <= t_max) & (t < np.inf)


def brute_force(o, d, vertices, faces, T, t_min=0.0, t_max=np.inf, cull=0, chunk=256):
    """Every ray against every face in T -> dict(t [n]: +inf on a miss, face [n]: the first of equal minima, -1, bary [n,2], side [n],
    count [n]: the number of accepted faces)."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    tri = np.asarray(vertices, np.float32)[np.asarray(faces, np.int64)]
    n = len(o)
    r = setup(o, d, T)
    t_min, t_max = T(t_min), T(t_max)
    t, face, count = np.full(n, np.inf, T), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for s in range(0, n, chunk):
        rows = slice(s, s + chunk)
        tt = ray_face(_rows(r, rows), tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], T, cull)["t"]
        acc = _accepted(tt, t_min, t_max) & bool(t_min <= t_max)
        tt = np.where(acc, tt, np.inf)
        k = tt.argmin(1)
        best = tt[np.arange(len(k)), k]
        t[rows], face[rows], count[rows] = best, np.where(best < np.inf, k, -1), acc.sum(1)
    hit = face >= 0
    own = ray_face(r, *(tri[np.maximum(face, 0), k] for k in range(3)), T, cull)
    bary = np.where(hit[:, None], np.stack([own["v"], own["w"]], -1), 0).astype(T)
    side = np.where(hit, np.where(own["det"] > 0, 1, -1), 0)
    return dict(t=t, face=face, bary=bary, side=side, count=count)


def pairs64(o, d, vertices, faces, t_min, t_max, cull, b_t, chunk=256):
    """Float64 over all (ray, face) pairs, by chunks of rays -> yields (rows, dict(t_raw, clear_hit, clear_miss, candidate, flat, zlo,
    zhi)), each [rows, F]; module docstring.  flat: no float64 t to compare with."""
    tri = np.asarray(vertices, np.float32)[np.asarray(faces, np.int64)]
    r = setup(o, d, np.float64)
    for s in range(0, len(o), chunk):
        rows = slice(s, s + chunk)
        p = ray_face(_rows(r, rows), tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], np.float64, cull, margins=True)
        with np.errstate(invalid="ignore"):
            t, e, m = p["t_raw"], p["e"], p["m"]
            clear_miss = p["clear_miss"]
            clear_hit = (e > m).all(-1) & (t >= t_min + b_t) & (t <= t_max - b_t) & (t < np.inf) & ~p["culled"]
            out_of_question = p["culled"] & (m.sum(-1) < 1)
            in_range = ~np.isfinite(t) | ((t >= t_min - b_t) & (t <= t_max + b_t))
            first = np.where(clear_hit, t, np.inf).min(1, keepdims=True)
            candidate = in_range & ~out_of_question & (~np.isfinite(t) | (t <= first + b_t))
            flat = ~np.isfinite(t) | ~(m.max(-1) <= 1)
        yield rows, dict(t_raw=t, clear_hit=clear_hit, clear_miss=clear_miss, candidate=candidate, flat=flat, zlo=p["zlo"], zhi=p["zhi"])


class Case:
    """A mesh, a ray set and a window [t_min, t_max] with both references, computed once."""

    def __init__(self, name, vertices, faces, o, d, t_min=0.0, t_max=np.inf, cull=0):
        self.name, self.vertices, self.faces = name, vertices, faces
        self.o, self.d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        self.t_min, self.t_max, self.cull = float(t_min), float(t_max), cull
        self._ref = None

    def ref(self):
        if self._ref is None:
            v, f, o, d = self.vertices, self.faces, self.o, self.d
            r32 = brute_force(o, d, v, f, np.float32, self.t_min, self.t_max, self.cull)
            r64 = brute_force(o, d, v, f, np.float64, self.t_min, self.t_max, self.cull)
            same = (r32["face"] == r64["face"]) & (r64["face"] >= 0)
            scale = float(r64["t"][r64["face"] >= 0].max()) if (r64["face"] >= 0).any() else 1.0
            e_t = max(float(np.abs(r32["t"][same].astype(np.float64) - r64["t"][same]).max()) if same.any() else 0.0, float(ulp32(scale)))
            hit32 = r32["face"] >= 0
            tri = np.asarray(v, np.float32)[np.asarray(f, np.int64)]
            own = ray_face(setup(o, d, np.float64), *(tri[np.maximum(r32["face"], 0), k] for k in range(3)), np.float64, self.cull)
            with np.errstate(invalid="ignore"):
                db = np.abs(r32["bary"].astype(np.float64) - np.stack([own["v"], own["w"]], -1))[hit32]
            db = db[np.isfinite(db)]
            e_b = max(float(db.max()) if db.size else 0.0, float(ulp32(1.0)))
            decided = np.ones(len(o), bool)
            for rows, p in pairs64(o, d, v, f, self.t_min, self.t_max, self.cull, 4 * e_t):
                decided[rows] = (~p["candidate"] | p["clear_hit"] | p["clear_miss"]).all(1)
            decided &= np.isfinite(o).all(1) & np.isfinite(d).all(1)
            self._ref = dict(r32=r32, r64=r64, e32_t=e_t, e32_b=e_b, decided=decided)
        return self._ref

    def undecided_fraction(self):
        return 1.0 - float(self.ref()["decided"].mean())


def judge(case, t, face, bary, side, any_face=False):
    """The standard assertion on one query's outputs (numpy arrays); returns the figures it printed.  any_face: the face need not be the
    first one (an any-hit query): only hit or miss is judged on decided rays, and t against the returned face."""
    R = case.ref()
    v, f = np.asarray(case.vertices, np.float32), np.asarray(case.faces, np.int64)
    r64, r32, b_t, b_b, dec = R["r64"], R["r32"], 4 * R["e32_t"], 4 * R["e32_b"], R["decided"]
    t, bary, face, side = np.asarray(t, np.float64), np.asarray(bary, np.float64), np.asarray(face, np.int64), np.asarray(side, np.int64)
    n = len(t)
    hit = face >= 0
    assert not np.isnan(t).any() and (np.isfinite(t) == hit).all() and (t[~hit] == np.inf).all(), case.name
    assert np.isfinite(bary).all() and (bary[~hit] == 0).all() and (side[~hit] == 0).all() and (np.abs(side[hit]) == 1).all(), case.name
    assert face.max(initial=-1) < len(f) and face.min(initial=0) >= -1, case.name
    bits = int((np.asarray(t, np.float32).view(np.uint32) != r32["t"].astype(np.float32).view(np.uint32)).sum())
    hit64 = r64["face"] >= 0
    wrong = int((hit != hit64)[dec].sum())
    print("%s: n=%d, %d hit, %d undecided (%.2f %%), %d decided rays with the wrong hit/miss, %d rays differ in bits from the float32 brute force"
          % (case.name, n, int(hit.sum()), int((~dec).sum()), 100.0 * (~dec).mean(), wrong, bits))
    assert wrong == 0, (case.name, wrong)
    tri = v[f]
    own = ray_face(setup(case.o, case.d, np.float64), *(tri[np.maximum(face, 0), k] for k in range(3)), np.float64, case.cull, margins=True)
    dh = dec & hit
    out = dict(undecided=int((~dec).sum()), bits=bits)
    if dh.any():
        with np.errstate(invalid="ignore"):
            err_own = np.abs(t - own["t_raw"])[dh].max()
            clear_miss = own["clear_miss"]
            clear_hit = (own["e"] > own["m"]).all(-1)
            err_b = np.abs(bary - np.stack([own["v"], own["w"]], -1))[dh].max()
        assert not clear_miss[dh].any(), (case.name, int(clear_miss[dh].sum()))
        assert err_own <= b_t, (case.name, err_own, b_t)
        if not any_face:
            err_t = np.abs(t[dh] - r64["t"][dh]).max()
            err_f = (own["t_raw"][dh] - r64["t"][dh]).max()
            print("%s: t err %.3g (%.2f x E32), returned face %.3g beyond the first, bound %.3g" % (case.name, err_t, err_t / R["e32_t"], err_f, b_t))
            assert err_t <= b_t and err_f <= b_t, (case.name, err_t, err_f, b_t)
            out["err_t"] = err_t
        print("%s: bary err %.3g (%.2f x E32), bound %.3g" % (case.name, err_b, err_b / R["e32_b"], b_b))
        assert err_b <= b_b, (case.name, err_b, b_b)
        sure = dh & clear_hit
        true_side = np.where(own["det"] > 0, 1, -1)
        assert (side[sure] == true_side[sure]).all(), (case.name, int((side[sure] != true_side[sure]).sum()))
        out["err_b"] = err_b
    uh = np.nonzero(~dec & hit)[0]
    if len(uh):
        ok = np.zeros(len(uh), bool)
        for rows, p in pairs64(case.o[uh], case.d[uh], v, f, case.t_min, case.t_max, case.cull, b_t):
            tt = t[uh][rows, None]
            with np.errstate(invalid="ignore"):
                near = ~p["clear_miss"] & (np.abs(tt - p["t_raw"]) <= b_t)
                in_plane = p["flat"] & ~p["clear_miss"] & (tt >= p["zlo"] - b_t) & (tt <= p["zhi"] + b_t)
            ok[rows] = (near | in_plane).any(1)
        assert ok.all(), (case.name, "undecided rays whose t belongs to no face", uh[~ok][:8])
    return out


# ---- ray sets -----------------------------------------------------------------------------------------------------------------------------
def _box(v):
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    return lo, hi, float(max((hi - lo).max(), 1e-3)), 0.5 * (lo + hi)


def _unit(rng, n):
    x = rng.standard_normal((n, 3))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def rays_outside_in(v, n, rng, distance=1.5, length=None):
    """Origins on a shell of `distance` diameters around the box, aimed at uniform points of the box; d = target - origin, or of the
    given length."""
    lo, hi, ext, c = _box(v)
    o = c + distance * ext * _unit(rng, n)
    d = rng.uniform(lo, hi, (n, 3)) - o
    if length is not None:
        d *= length / np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def rays_inside_out(v, n, rng, pad=0.25):
    """Origins uniform in the box padded by `pad` diameters on every side (a flat mesh has a flat box), unit directions."""
    lo, hi, ext, _ = _box(v)
    return rng.uniform(lo - pad * ext, hi + pad * ext, (n, 3)).astype(np.float32), _unit(rng, n).astype(np.float32)


def rays_grazing(v, f, n, rng, in_plane=4):
    """Through an interior point of a random face at 0.03 to 0.15 radians from its plane, from 0.75 diameters away; the last `in_plane`
    rays lie in the plane itself (up to the rounding of the inputs) and are undecided by construction.  The margin of a face grows as
    1 / sin(angle): shallower rays than these leave more than MAX_UNDECIDED of a set undecided."""
    _, _, ext, _ = _box(v)
    tri = v[f[rng.integers(0, len(f), n)]].astype(np.float64)
    p = (tri * rng.dirichlet((2.0, 2.0, 2.0), n)[:, :, None]).sum(1)
    e1 = tri[:, 1] - tri[:, 0]
    nrm = np.cross(e1, tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(nrm, e1)
    ang = rng.uniform(0, 2 * np.pi, n)
    tilt = rng.uniform(0.03, 0.15, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    tilt[n - in_plane:] = 0.0
    d = np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2 + tilt[:, None] * nrm
    return (p - 0.75 * ext * d).astype(np.float32), d.astype(np.float32)


def rays_far(v, f, n, rng, distance=1000.0):
    """Origins `distance` diameters away, each aimed at a point of a face drawn by area whose barycentrics are all >= 0.15, from the side the
    face's normal points to (within 80 degrees of it); d = target - origin, so t is about 1.  At this distance one float32 ulp of a
    coordinate is about a thousandth of an icosphere edge and the margin several hundredths of a barycentric: rays aimed at uniform
    points of the box would leave far more than MAX_UNDECIDED of a set undecided, whatever the arithmetic under test."""
    _, _, ext, c = _box(v)
    tri = v[f].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    tri = tri[rng.choice(len(f), n, p=area / area.sum())]                 # by area: an extraction's slivers are rarely aimed at
    p = (tri * (0.15 + 0.55 * rng.dirichlet((1.0, 1.0, 1.0), n))[:, :, None]).sum(1)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    u = nrm + 0.7 * _unit(rng, n)
    o = c + distance * ext * u / np.linalg.norm(u, axis=1, keepdims=True)
    return o.astype(np.float32), (p - o).astype(np.float32)


def watertight_targets(v, f, rng):
    """Every vertex, every edge midpoint and a random point of every edge of an indexed mesh (float64)."""
    v = v.astype(np.float64)
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    a, b = v[edges[:, 0]], v[edges[:, 1]]
    w = rng.uniform(0.05, 0.95, (len(edges), 1))
    return np.concatenate([v, 0.5 * (a + b), a + w * (b - a)])


def watertight_set(origin, seed=5, front_only=False):
    """Rays from `origin` aimed exactly at watertight_targets of the 1280-face icosphere -> (v, f, o, d); front_only keeps the targets
    whose outward normal n has n . (o - x) > 0.3 |o - x|."""
    v, f = M.icosphere()
    x = watertight_targets(v, f, np.random.default_rng(seed))
    o = np.broadcast_to(np.asarray(origin, np.float64), x.shape)
    if front_only:
        nrm = x - 0.5
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        keep = (nrm * (o - x)).sum(1) > 0.3 * np.linalg.norm(o - x, axis=1)
        x, o = x[keep], o[keep]
    o32 = o.astype(np.float32)
    return v, f, o32, (x.astype(np.float32) - o32)


INSIDE_ORIGINS = {"centre": (0.5, 0.5, 0.5), "off-centre": (0.58, 0.44, 0.63)}
OUTSIDE_DIRECTION = np.array([0.36, -0.48, 0.8])


def _mesh(name):
    if name == "open_quad":
        return M.open_quad()
    return M._mesh(name)


MESHES = ("triangle", "cube", "needle", "icosphere", "open_quad", "torus")
KINDS = ("outside_in", "inside_out", "grazing", "far1000", "short_d", "long_d")
CASES = ["%s/%s" % (m, k) for m in MESHES for k in KINDS]
N_RAYS = 512
_CASES = {}


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    mesh, kind = name.split("/")
    v, f = _mesh(mesh)
    if kind == "outside_in":
        o, d = rays_outside_in(v, N_RAYS, rng)
    elif kind == "inside_out":
        o, d = rays_inside_out(v, N_RAYS, rng)
    elif kind == "grazing":
        o, d = rays_grazing(v, f, N_RAYS, rng)
    elif kind == "far1000":
        o, d = rays_far(v, f, N_RAYS, rng)
    elif kind == "short_d":
        o, d = rays_outside_in(v, N_RAYS, rng, length=1e-3)
    elif kind == "long_d":
        o, d = rays_outside_in(v, N_RAYS, rng, length=1e3)
    else:
        raise KeyError(name)
    return Case(name, v, f, o, d)


def case(name):
    """The named case, built (and its references computed) once per process."""
    if name not in _CASES:
        _CASES[name] = _build(name)
    return _CASES[name]
