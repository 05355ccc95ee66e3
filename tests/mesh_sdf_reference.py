"""numpy reference of the distance-to-mesh contract (include/ngp_hip.h, "distance to a triangle mesh"; csrc/mesh_sdf.hip): a brute force
over ALL faces, no hierarchy, in two arithmetics that run the same code.

  np.float64   the truth
  np.float32   the kernel's formula restated operation for operation (numpy's float32 operations are IEEE binary32, one rounding
               each); it gives E32, the error a correct float32 evaluation has on a set

What is judged (judge(), the standard assertion of tests/test_gpu_mesh_sdf.py), with B = 4 x E32:
  distance   | |sdf| - d64 | <= B_d.  E32_d = max |d32 - d64| over the set, at least one float32 ulp of the largest distance or face
             diameter of the set (the floor tests/sdf_trace_reference.py uses: one ulp of the quantity's scale).
  face       the returned face is A nearest face: its float64 distance to the point is within B_d of the minimum (indices are not
             compared: the faces that share the nearest feature tie).
  closest    | closest - (the float64 closest point ON THE RETURNED FACE) | <= B_c per axis.  E32_c = the same quantity for the serial
             float32 run and its own face, at least one ulp of the largest coordinate.  Measured on the returned face because the
             nearest point of the whole mesh jumps where two faces are equally near, which no arithmetic can follow; that the face is
             a nearest one is judged separately.  Skipped, like the sign, on the sets named on_surface / equidistant.
  feature    the closest point lies on the feature the code names, in float64, within B_c + B_d.
  sign       exact on every DECIDED point.  A point is decided when every feature (vertex, edge, interior of any face) whose float64
             distance to the point is within B_d of the minimum (an edge: where the foot of the point lies on it, or within EDGE_END
             of its length past an end -- beyond that the vertex is the feature) gives n . (x - c) of the same sign and with
             |n . (x - c)| > SIGN_MARGIN x 2^-24 x N x (|x - c| + diameter of the face), N = |n| for an edge or a vertex and |ab| |ac|
             for the interior (whose normal the kernel forms from rounded differences): SIGN_MARGIN float32 roundings of the dot
             product, counting those of n and of r = x - c.
MAX_UNDECIDED is a condition on the sets, not a measurement: tests/test_mesh_sdf_reference.py asserts it for the reference alone."""
import numpy as np

EPS = 2.0**-24
MAX_UNDECIDED = 0.02                       # as tests/sdf_trace_reference.py and tests/resample_reference.py
SIGN_MARGIN = 16.0
EDGE_END = 1e-4                            # an edge counts as the nearest feature up to this share of its length past its ends
INTERIOR, EDGE_AB, EDGE_BC, EDGE_CA, VERTEX_A, VERTEX_B, VERTEX_C = range(7)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def closest_on_triangle(p, a, b, c, T):
    """Ericson 5.1.5 as csrc/mesh_sdf.hip states it, on broadcastable [..., 3] arrays in the arithmetic T -> dict(d2, feature, closest,
    r, n).  Every rule is evaluated and the first that holds is selected."""
    p, a, b, c = (np.asarray(x).astype(T) for x in (p, a, b, c))
    one, zero = T(1.0), T(0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        ab, ac = np.broadcast_arrays(ab, ac)
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = one / ((va + vb) + vc)
        v, w = vb * den, vc * den
        feature = np.zeros(v.shape, np.int32)
        e43, e56 = d4 - d3, d5 - d6

        def rule(cond, v_new, w_new, code):
            nonlocal v, w, feature
            v, w, feature = np.where(cond, v_new, v), np.where(cond, w_new, w), np.where(cond, np.int32(code), feature)

        w_bc = e43 / (e43 + e56)
        rule((va <= zero) & (e43 >= zero) & (e56 >= zero), one - w_bc, w_bc, EDGE_BC)
        rule((vb <= zero) & (d2 >= zero) & (d6 <= zero), zero, d2 / (d2 - d6), EDGE_CA)
        rule((d6 >= zero) & (d5 <= d6), zero, one, VERTEX_C)
        rule((vc <= zero) & (d1 >= zero) & (d3 <= zero), d1 / (d1 - d3), zero, EDGE_AB)
        rule((d3 >= zero) & (d4 <= d3), one, zero, VERTEX_B)
        rule((d1 <= zero) & (d2 <= zero), zero, zero, VERTEX_A)
        v, w = v.astype(T)[..., None], w.astype(T)[..., None]
        closest = (a + ab * v) + ac * w
        r = ap - (ab * v + ac * w)
        n = cross(ab, ac)
        area = (n[..., 0] != zero) | (n[..., 1] != zero) | (n[..., 2] != zero)
        dist2 = np.where(area, dot(r, r), T(np.nan))
    return dict(d2=dist2, feature=feature, closest=closest, r=r, n=np.broadcast_to(n, r.shape))


def brute_force(points, vertices, faces, T, chunk=128, near_tol=None):
    """Every point against every face in T -> dict(d2, d [n], face [n] (the first of equal minima), feature [n], closest, r, n [n,3]).
    A NaN distance never wins.  near_tol (float64 only): also `near` = (point, face) index pairs with d <= d_min + near_tol."""
    points = np.asarray(points, np.float32)
    tri = np.asarray(vertices, np.float32)[np.asarray(faces, np.int64)]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    face = np.zeros(len(points), np.int64)
    near = [[], []]
    for s in range(0, len(points), chunk):
        d2 = closest_on_triangle(points[s:s + chunk, None, :], a, b, c, T)["d2"]
        d2 = np.where(np.isnan(d2), np.inf, d2)
        face[s:s + chunk] = d2.argmin(1)
        if near_tol is not None:
            d = np.sqrt(d2)
            pi, fi = np.nonzero(d <= d.min(1, keepdims=True) + near_tol)
            near[0].append(pi + s)
            near[1].append(fi)
    out = closest_on_triangle(points, tri[face, 0], tri[face, 1], tri[face, 2], T)
    out["face"] = face
    out["d"] = np.sqrt(out["d2"])
    if near_tol is not None:
        out["near"] = (np.concatenate(near[0]), np.concatenate(near[1]))
    return out


# ---- pseudonormals (float64) and the sign -------------------------------------------------------------------------------------------------
def pseudonormals(vertices, faces):
    """(edge [T,3,3], vertex [V,3]) in float64, straight from the definition with python dictionaries: independent of the package's
    vectorised construction.  Edge e of a face: ab, bc, ca."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    unit = np.zeros((len(f), 3))
    for t, (i, j, k) in enumerate(f):
        n = np.cross(v[j] - v[i], v[k] - v[i])
        if np.linalg.norm(n) > 0:
            unit[t] = n / np.linalg.norm(n)
    edges, vertex = {}, np.zeros_like(v)
    for t, tri in enumerate(f):
        for e in range(3):
            i, j, k = tri[e], tri[(e + 1) % 3], tri[(e + 2) % 3]
            edges[(min(i, j), max(i, j))] = edges.get((min(i, j), max(i, j)), 0.0) + unit[t]
            e1, e2 = v[j] - v[i], v[k] - v[i]
            l1, l2 = np.linalg.norm(e1), np.linalg.norm(e2)
            if l1 > 0 and l2 > 0:
                vertex[i] += np.arccos(np.clip(e1 @ e2 / (l1 * l2), -1.0, 1.0)) * unit[t]
    edge = np.array([[edges[(min(tri[e], tri[(e + 1) % 3]), max(tri[e], tri[(e + 1) % 3]))] for e in range(3)] for tri in f]).reshape(-1, 3, 3)
    return edge, vertex


def feature_normal(hit, faces, edge_n, vertex_n):
    """The normal the sign rule uses for each row of a brute_force / closest_on_triangle result with `face` and `feature`."""
    f, code = hit["face"], hit["feature"]
    n = np.array(hit["n"], np.float64)
    e = (code >= 1) & (code <= 3)
    n[e] = edge_n[f[e], code[e] - 1]
    k = code >= 4
    n[k] = vertex_n[np.asarray(faces, np.int64)[f[k], code[k] - 4]]
    return n


def signed(hit, faces, edge_n, vertex_n):
    """+1 / -1 per point: n . r >= 0 (the arithmetic of the arrays given)."""
    return np.where(dot(feature_normal(hit, faces, edge_n, vertex_n), np.asarray(hit["r"], np.float64)) >= 0, 1.0, -1.0)


def face_normal_sign(hit):
    """The sign a nearest face WITHOUT pseudonormals would give: its own normal, whatever the feature."""
    return np.where(dot(np.asarray(hit["n"], np.float64), np.asarray(hit["r"], np.float64)) >= 0, 1.0, -1.0)


def _segment(x, p0, p1, return_t=False):
    """The nearest point of the segment p0 p1 (and the unclipped parameter along it)."""
    e = p1 - p0
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.nan_to_num(dot(x - p0, e) / dot(e, e))
    c = p0 + np.clip(t, 0.0, 1.0)[..., None] * e
    return (c, t) if return_t else c


def decide(points, vertices, faces, edge_n, vertex_n, ref64, tol):
    """bool [n]: the sign is decided (module docstring).  ref64: brute_force(..., np.float64, near_tol >= tol)."""
    x_all = np.asarray(points, np.float64)
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    pi, fi = ref64["near"]
    x, tri = x_all[pi], v[f[fi]]
    dmin = ref64["d"][pi]
    diam = np.max([np.linalg.norm(tri[:, i] - tri[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0))], 0)
    cand = []                                                      # (closest point, normal, scale of the normal) per feature
    for k in range(3):
        cand.append((tri[:, k], vertex_n[f[fi, k]], None))
        c, t = _segment(x, tri[:, k], tri[:, (k + 1) % 3], return_t=True)
        inside = (t >= -EDGE_END) & (t <= 1.0 + EDGE_END)          # past its end an edge is not the feature: the vertex is
        cand.append((np.where(inside[:, None], c, np.inf), edge_n[fi, k], None))
    inner = closest_on_triangle(x, tri[:, 0], tri[:, 1], tri[:, 2], np.float64)
    ab, ac = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cand.append((np.where((inner["feature"] == INTERIOR)[:, None], inner["closest"], np.inf), cross(ab, ac),
                 np.linalg.norm(ab, axis=1) * np.linalg.norm(ac, axis=1)))
    ok = np.ones(len(x_all), bool)
    pos, neg = np.zeros(len(x_all), bool), np.zeros(len(x_all), bool)
    for c, n, scale in cand:
        with np.errstate(invalid="ignore"):
            r = x - c
            dist = np.linalg.norm(r, axis=1)
            live = dist <= dmin + tol
            s = dot(n, np.where(live[:, None], r, 0.0))
        scale = np.linalg.norm(n, axis=1) if scale is None else scale
        good = np.abs(s) > SIGN_MARGIN * EPS * scale * (dist + diam)
        np.logical_and.at(ok, pi[live], good[live])
        np.logical_or.at(pos, pi[live], s[live] > 0)
        np.logical_or.at(neg, pi[live], s[live] < 0)
    return ok & (pos != neg)


# ---- meshes -------------------------------------------------------------------------------------------------------------------------------
def triangle():
    return np.array([[0.1, 0.2, 0.0], [0.9, 0.3, 0.1], [0.4, 0.8, -0.1]], np.float32), np.array([[0, 1, 2]], np.int32)


def cube(lo=0.25, hi=0.75):
    """The box [lo, hi]^3, 12 faces, counter-clockwise seen from the outside."""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float32)        # index 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]          # -x +x -y +y -z +z
    f = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v, np.array(f, np.int32)


def box_sdf(x, lo=0.25, hi=0.75):
    q = np.abs(np.asarray(x, np.float64) - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
    return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(1), 0.0)


def needle_tetrahedron():
    """A base triangle of circumradius 0.05 in z = 0 and an apex one unit above it: the three long faces meet at the apex at about 3
    degrees from the axis.  Outward orientation."""
    v = np.array([[0.05, 0.0, 0.0], [-0.025, 0.0433, 0.0], [-0.025, -0.0433, 0.0], [0.0, 0.0, 1.0]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return v, f


def icosphere(subdivisions=3, centre=(0.5, 0.5, 0.5), radius=0.35):
    """20 x 4^subdivisions faces (3: 1280), vertices on the sphere, outward orientation."""
    t = (1.0 + 5.0**0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return (np.asarray(centre) + radius * np.array(v)).astype(np.float32), np.array(f, np.int32)


def torus_sdf(x, R=0.2, r=0.07, centre=(0.5, 0.5, 0.5)):
    q = np.asarray(x, np.float64) - np.asarray(centre)
    return np.sqrt((np.sqrt(q[..., 0]**2 + q[..., 1]**2) - R)**2 + q[..., 2]**2) - r


def extracted_torus(resolution=32):
    """The torus as marching tetrahedra extract it from its analytic SDF on resolution^3 cells of the unit box (tests/mesh_reference.py,
    the numpy statement of csrc/mesh.hip): a closed mesh with the slivers an extraction makes."""
    import mesh_reference as mr
    a = np.linspace(0.0, 1.0, resolution + 1)
    field = torus_sdf(np.stack(np.meshgrid(a, a, a, indexing="ij"), -1)).astype(np.float32)
    m = mr.marching_tetrahedra(field, 0.0, -1, (0.0, 0.0, 0.0), (1.0 / resolution,) * 3)
    return m["vertices"].astype(np.float32), m["faces"].astype(np.int32)


def soup(n_faces, seed, size=0.08, same_centroid=False):
    """n_faces unconnected random triangles in the unit box (3 n_faces vertices); same_centroid: (c + u, c + v, c - u - v) around ONE
    point c, so that every centroid has the same Morton code."""
    rng = np.random.default_rng(seed)
    c = np.full((n_faces, 1, 3), 0.5) if same_centroid else rng.uniform(0.1, 0.9, (n_faces, 1, 3))
    off = rng.uniform(-size, size, (n_faces, 3, 3))
    if same_centroid:
        off[:, 2] = -off[:, 0] - off[:, 1]
    return (c + off).reshape(-1, 3).astype(np.float32), np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def open_quad():
    return np.array([[0.2, 0.2, 0.5], [0.8, 0.2, 0.5], [0.8, 0.8, 0.5], [0.2, 0.8, 0.5]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


# ---- point sets ---------------------------------------------------------------------------------------------------------------------------
def pts_uniform(v, n, rng, pad=0.25):
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    ext = (hi - lo).max()
    return rng.uniform(lo - pad * ext, hi + pad * ext, (n, 3)).astype(np.float32)


def pts_near(v, f, n, rng, sigma=0.01):
    t = v[f[rng.integers(0, len(f), n)]].astype(np.float64)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    return ((t * w[:, :, None]).sum(1) + sigma * rng.standard_normal((n, 3))).astype(np.float32)


def pts_far(v, n, rng, factor):
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    d = rng.standard_normal((n, 3))
    return (0.5 * (lo + hi) + factor * (hi - lo).max() * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def pts_triangle_regions(rng, per_region=24, in_plane=False):
    """Points of all seven Voronoi regions of triangle(): barycentric coordinates chosen per region, lifted off the plane to both sides
    or (in_plane, where no sign exists) left in it."""
    v, _ = triangle()
    a, b, c = v.astype(np.float64)
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    out = []
    for region in range(7):
        u = rng.uniform(0.1, 0.8, (per_region, 3))
        if region == 0:
            w = u / u.sum(1, keepdims=True)                         # inside
        elif region <= 3:                                           # beyond one edge: one negative coordinate
            w = u / u.sum(1, keepdims=True)
            k = (region + 1) % 3
            w[:, k] = -w[:, k]
            w /= w.sum(1, keepdims=True)
        else:                                                       # beyond a vertex: two negative coordinates
            w = -0.3 * u
            k = region - 4
            w[:, k] = 1.0 - (w.sum(1) - w[:, k])
        p = w[:, [0]] * a + w[:, [1]] * b + w[:, [2]] * c
        lift = np.zeros((per_region, 1)) if in_plane else np.repeat([0.3, -0.3, 0.02, -0.02], per_region // 4)[:, None]
        out.append(p + lift * n)
    return np.concatenate(out).astype(np.float32)


def pts_needle_apex(n, rng):
    """Points whose nearest feature is the apex or one of the three long edges of needle_tetrahedron(): a shell around the upper part."""
    z = rng.uniform(0.6, 1.15, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    rad = rng.uniform(0.03, 0.25, n)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), z], 1).astype(np.float32)


class Case:
    """A mesh and a point set with both references, computed once.  on_surface: the set is built to lie on the surface or at equal
    distance from several faces, so only the distance and |x - closest| are judged on it."""

    def __init__(self, name, vertices, faces, points, signed_mode=True, on_surface=False):
        self.name, self.vertices, self.faces, self.points = name, vertices, faces, np.ascontiguousarray(points, np.float32)
        self.signed_mode, self.on_surface = signed_mode, on_surface
        self._ref = None

    def ref(self):
        if self._ref is None:
            v, f, x = self.vertices, self.faces, self.points
            r32 = brute_force(x, v, f, np.float32)
            first = r64 = brute_force(x, v, f, np.float64, near_tol=1e-4 * float(np.abs(v).max()))      # decide() narrows `near` to B_d
            tri = v[f].astype(np.float64)
            diam = np.max([np.linalg.norm(tri[:, i] - tri[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0))])
            e_d = max(float(np.abs(r32["d"].astype(np.float64) - first["d"]).max()), float(ulp32(max(first["d"].max(), diam))))
            own = closest_on_triangle(x, *(v[f[r32["face"]]][:, k] for k in range(3)), np.float64)          # float64 on float32's face
            scale = max(float(np.abs(x).max()), float(np.abs(v).max()))
            e_c = max(float(np.abs(r32["closest"].astype(np.float64) - own["closest"]).max()), float(ulp32(scale)))
            edge_n, vertex_n = pseudonormals(v, f)
            sign = signed(r64, f, edge_n, vertex_n)
            decided = decide(x, v, f, edge_n, vertex_n, r64, 4 * e_d) if self.signed_mode and not self.on_surface else np.zeros(len(x), bool)
            self._ref = dict(r32=r32, r64=r64, e32_d=e_d, e32_c=e_c, edge_n=edge_n, vertex_n=vertex_n, sign=sign, decided=decided)
        return self._ref

    def undecided_fraction(self):
        return 1.0 - float(self.ref()["decided"].mean())


def judge(case, sdf, closest, face, feature):
    """The standard assertion on one query's outputs (numpy arrays); returns the figures it printed."""
    R = case.ref()
    v, f, x = case.vertices.astype(np.float64), case.faces.astype(np.int64), case.points.astype(np.float64)
    r64, b_d, b_c = R["r64"], 4 * R["e32_d"], 4 * R["e32_c"]
    sdf, closest = np.asarray(sdf, np.float64), np.asarray(closest, np.float64)
    assert np.isfinite(sdf).all() and np.isfinite(closest).all(), case.name
    assert face.min() >= 0 and face.max() < len(f) and feature.min() >= 0 and feature.max() <= 6, case.name
    err_d = np.abs(np.abs(sdf) - r64["d"]).max()
    err_x = np.abs(np.linalg.norm(x - closest, axis=1) - r64["d"]).max()
    own = closest_on_triangle(x, v[f[face, 0]], v[f[face, 1]], v[f[face, 2]], np.float64)
    err_f = (np.sqrt(own["d2"]) - r64["d"]).max()
    print("%s: n=%d |sdf| err %.3g (%.2f x E32), |x - closest| err %.3g, returned face %.3g above the minimum, bound %.3g"
          % (case.name, len(x), err_d, err_d / R["e32_d"], err_x, err_f, b_d))
    assert err_d <= b_d, (case.name, err_d, b_d)
    assert err_x <= b_d + b_c, (case.name, err_x, b_d + b_c)
    assert not np.isnan(own["d2"]).any() and err_f <= b_d, (case.name, err_f, b_d)
    # the feature: the returned closest point lies on it
    tri = v[f[face]]
    k = np.clip(feature - 4, 0, 2)
    e = np.clip(feature - 1, 0, 2)
    rows = np.arange(len(x))
    on_vertex = np.linalg.norm(closest - tri[rows, k], axis=1)
    on_edge = np.linalg.norm(closest - _segment(closest, tri[rows, e], tri[rows, (e + 1) % 3]), axis=1)
    on_face = np.sqrt(closest_on_triangle(closest, tri[:, 0], tri[:, 1], tri[:, 2], np.float64)["d2"])
    off = np.where(feature >= 4, on_vertex, np.where(feature >= 1, on_edge, on_face))
    print("%s: closest point off its feature by at most %.3g (bound %.3g)" % (case.name, off.max(), b_c + b_d))
    assert off.max() <= b_c + b_d, (case.name, off.max())
    if not case.signed_mode:
        assert (sdf >= 0).all(), case.name
    if case.on_surface:
        return dict(err_d=err_d)
    err_c = np.abs(closest - own["closest"]).max()
    print("%s: closest err %.3g (%.2f x E32)" % (case.name, err_c, err_c / R["e32_c"]))
    assert err_c <= b_c, (case.name, err_c, b_c)
    if case.signed_mode:
        dec = R["decided"]
        wrong = int((np.where(sdf[dec] < 0, -1.0, 1.0) != R["sign"][dec]).sum())
        print("%s: %d of %d points decided, %d wrong signs" % (case.name, int(dec.sum()), len(x), wrong))
        assert wrong == 0, (case.name, wrong)
    return dict(err_d=err_d, err_c=err_c)


_CASES = {}


def _mesh(name):
    return {"icosphere": icosphere, "torus": extracted_torus, "cube": cube, "needle": needle_tetrahedron, "triangle": triangle}[name]()


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    mesh, kind = name.split("/")
    v, f = _mesh(mesh)
    tri = v[f].astype(np.float64)
    if kind == "uniform":
        return Case(name, v, f, pts_uniform(v, 768, rng))
    if kind == "near":
        return Case(name, v, f, pts_near(v, f, 768, rng))
    if kind == "far10":
        return Case(name, v, f, pts_far(v, 256, rng, 10.0))
    if kind == "far1000":
        return Case(name, v, f, pts_far(v, 256, rng, 1000.0))
    if kind == "vertices":
        return Case(name, v, f, v[rng.permutation(len(v))[:384]], on_surface=True)
    if kind == "edge_midpoints":
        pick = rng.permutation(len(f))[:384]
        return Case(name, v, f, (0.5 * (tri[pick, 0] + tri[pick, 1])).astype(np.float32), on_surface=True)
    if kind == "centroids":
        return Case(name, v, f, tri[rng.permutation(len(f))[:384]].mean(1).astype(np.float32), on_surface=True)
    if kind == "regions":
        return Case(name, v, f, pts_triangle_regions(rng))
    if kind == "in_plane":
        return Case(name, v, f, pts_triangle_regions(rng, in_plane=True), on_surface=True)
    if kind == "regions_unsigned":
        return Case(name, v, f, pts_triangle_regions(rng), signed_mode=False)
    if kind == "apex":
        return Case(name, v, f, pts_needle_apex(768, rng))
    raise KeyError(name)


KINDS = ("uniform", "near", "far10", "far1000", "vertices", "edge_midpoints", "centroids")
CASES = ["triangle/regions", "triangle/in_plane", "triangle/regions_unsigned", "needle/apex", "needle/uniform", "cube/uniform", "cube/near"] \
    + ["%s/%s" % (m, k) for m in ("icosphere", "torus") for k in KINDS]
SIGNED_SETS = [c for c in CASES if c.split("/")[1] in ("uniform", "near", "far10", "far1000", "regions", "apex")]


def case(name):
    """The named case, built (and its references computed) once per process."""
    if name not in _CASES:
        _CASES[name] = _build(name)
    return _CASES[name]
