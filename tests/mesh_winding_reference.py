"""numpy reference of the winding-number contract (include/ngp_hip.h, "winding number of a triangle mesh"; csrc/mesh_winding.hip).

  exact(points, v, f)                      the float64 sum of the solid angles of ALL faces, no hierarchy: the truth
  moments(v, f, order, leaf_size, T)       the per-node moments of the tree, the kernels' formulas operation for operation in T
  tree(points, ..., beta, order_terms, T)  the preorder walk with the acceptance rule and the far-field terms, summed serially in walk
                                           order, for T = np.float64 and for T = np.float32 (numpy's float32 operations are IEEE
                                           binary32, one rounding each)
The boxes are those of csrc/mesh_sdf.hip, restated here bit for bit in float32 (boxes()): they are an INPUT of the moments in either
arithmetic.  What is judged per set (Case.ref), for one order of the faces, one beta and one number of far-field terms:
  decided   a point none of whose acceptance tests on the float64 walk has | |d| - beta r | <= NEAR_ACCEPT |d|: float32 takes the same
            decisions there, so it evaluates the same sum
  E32       max |tree32 - tree64| over the decided points of the set, at least one float32 ulp of 1 (the floor of
            mesh_sdf_reference.Case.ref: one ulp of the quantity's scale).  Where a point is undecided the two walks may differ by a whole
            node's approximation error, which is no rounding error: those points are left out, which only tightens the bound
  A_set     max |tree64 - exact|: the approximation error of the rule on that set
MAX_UNDECIDED is a condition on the sets, asserted for the reference alone (tests/test_mesh_winding_reference.py)."""
import numpy as np

import mesh_sdf_reference as M

ROW = 20
ULP1 = float(np.spacing(np.float32(1.0)))
NEAR_ACCEPT = 1e-5
MAX_UNDECIDED = 0.02
INV_4PI = 0.07957747154594767
INF = float("inf")


def solid_angle(q, A, B, C, T):
    """van Oosterom & Strackee as csrc/mesh_winding.hip states it, on broadcastable [..., 3] arrays in the arithmetic T."""
    q, A, B, C = (np.asarray(x).astype(T) for x in (q, A, B, C))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a, b, c = A - q, B - q, C - q
        la, lb, lc = np.sqrt(M.dot(a, a)), np.sqrt(M.dot(b, b)), np.sqrt(M.dot(c, c))
        num = M.dot(a, M.cross(b, c))
        den = (((la * lb) * lc + M.dot(a, b) * lc) + M.dot(b, c) * la) + M.dot(c, a) * lb
        return np.where(num == 0, T(0.0), T(2.0) * np.arctan2(num, den)).astype(T)


def exact(points, vertices, faces, chunk=256):
    """w [n] in float64: every point against every face."""
    x = np.asarray(points, np.float32)
    tri = np.asarray(vertices, np.float32)[np.asarray(faces, np.int64)]
    out = np.empty(len(x))
    for s in range(0, len(x), chunk):
        out[s:s + chunk] = solid_angle(x[s:s + chunk, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], np.float64).sum(1)
    return out * INV_4PI


# ---- the tree ----------------------------------------------------------------------------------------------------------------------------
def _spread21(x):
    x = x & 0x1fffff
    x = (x | (x << 32)) & 0x1f00000000ffff
    x = (x | (x << 16)) & 0x1f0000ff0000ff
    x = (x | (x << 8)) & 0x100f00f00f00f00f
    x = (x | (x << 4)) & 0x10c30c30c30c30c3
    x = (x | (x << 2)) & 0x1249249249249249
    return x


def morton_order(vertices, faces):
    """An order of the faces by the Morton code of their centroids, as ngp_hip.mesh_sdf.morton_order makes one.  The tests on the GPU
    pass the package's own order instead: a centroid that rounds differently may exchange two faces, and the tree is a function of the
    order."""
    v, f = np.asarray(vertices, np.float32), np.asarray(faces, np.int64)
    lo, hi = v.min(0), v.max(0)
    c = (v[f[:, 0]] + v[f[:, 1]] + v[f[:, 2]]) / np.float32(3.0)
    extent = np.maximum(hi - lo, np.finfo(np.float32).tiny)
    q = (np.clip((c - lo) / extent, 0.0, 1.0).astype(np.float64) * 2097151.0).astype(np.int64)
    code = _spread21(q[:, 0]) | (_spread21(q[:, 1]) << 1) | (_spread21(q[:, 2]) << 2)
    return np.argsort(code, kind="stable").astype(np.int32)


def shape(n_faces, leaf_size):
    """(P, depth): the padded number of leaves and log2 P."""
    leaves = (n_faces + leaf_size - 1) // leaf_size
    P, depth = 1, 0
    while P < leaves:
        P, depth = 2 * P, depth + 1
    return P, depth


def _leaf_faces(faces, order, leaf_size):
    """(corner indices [P, L, 3] int64, valid [P, L]): the faces of every leaf in sorted order; invalid slots repeat the last face."""
    n = len(order)
    P, _ = shape(n, leaf_size)
    pos = np.arange(P * leaf_size).reshape(P, leaf_size)
    return np.asarray(faces, np.int64)[np.asarray(order, np.int64)[np.minimum(pos, n - 1)]], pos < n


def boxes(vertices, faces, order, leaf_size):
    """f32 [2 P - 1, 6]: the boxes of ngp_mesh_bvh_build (csrc/mesh_sdf.hip, "THE TREE"), bit for bit."""
    v = np.asarray(vertices, np.float32)
    corners, valid = _leaf_faces(faces, order, leaf_size)
    P, depth = shape(len(order), leaf_size)
    xyz = v[corners]                                                                  # [P, L, 3 corners, 3 axes]
    mask = valid[:, :, None, None]
    lo = np.where(mask, xyz, np.float32(np.inf)).min((1, 2))
    hi = np.where(mask, xyz, np.float32(-np.inf)).max((1, 2))
    full = valid[:, 0]
    with np.errstate(invalid="ignore"):
        m = ((hi - lo).max(1) * np.float32(2.0**-18))[:, None]
        wide_lo, wide_hi = np.nextafter(lo - m, np.float32(-np.inf)), np.nextafter(hi + m, np.float32(np.inf))
    lo, hi = np.where(full[:, None], wide_lo, lo), np.where(full[:, None], wide_hi, hi)
    out = np.empty((2 * P - 1, 6), np.float32)
    out[P - 1:, :3], out[P - 1:, 3:] = lo, hi
    for d in range(depth - 1, -1, -1):
        i = np.arange(2**d - 1, 2**(d + 1) - 1)
        out[i, :3] = np.minimum(out[2 * i + 1, :3], out[2 * i + 2, :3])
        out[i, 3:] = np.maximum(out[2 * i + 1, 3:], out[2 * i + 2, 3:])
    return out


def _radius(box, p, T):
    m = np.maximum(p - box[:, :3], box[:, 3:] - p)
    return np.sqrt(M.dot(m, m)) * T(1.0 + 2.0**-21)


def _centre(box, T):
    return T(0.5) * box[:, :3] + T(0.5) * box[:, 3:]


def _outer(u, w):
    return u[:, :, None] * w[:, None, :]


def moments(vertices, faces, order, leaf_size, T, box32=None):
    """[2 P - 1, 20] in T: the rows of ngp_mesh_winding_build (columns: include/ngp_hip.h)."""
    box32 = boxes(vertices, faces, order, leaf_size) if box32 is None else box32
    box = box32.astype(T)
    v = np.asarray(vertices, np.float32).astype(T)
    corners, valid = _leaf_faces(faces, order, leaf_size)
    P, depth = shape(len(order), leaf_size)
    tri = v[corners]
    o = tri[:, 0, 0]
    A, S, N, To = np.zeros(P, T), np.zeros((P, 3), T), np.zeros((P, 3), T), np.zeros((P, 3, 3), T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for j in range(leaf_size):
            ok = valid[:, j]
            a, b, c = tri[:, j, 0], tri[:, j, 1], tri[:, j, 2]
            n2 = M.cross(b - a, c - a)
            an = T(0.5) * n2
            area = T(0.5) * np.sqrt(M.dot(n2, n2))
            cf = (((a - o) + (b - o)) + (c - o)) / T(3.0)
            A = np.where(ok, A + area, A)
            S = np.where(ok[:, None], S + cf * area[:, None], S)
            N = np.where(ok[:, None], N + an, N)
            To = np.where(ok[:, None, None], To + _outer(cf, an), To)
        leaf_box = box[P - 1:]
        centre = _centre(leaf_box, T)
        has_area = (A > 0)[:, None]
        pl = np.where(has_area, S / A[:, None], centre - o)
        p = np.where(has_area, o + pl, centre)
        Tm = To - _outer(pl, N)
        rows = np.zeros((2 * P - 1, ROW), T)
        rows[:, 3] = T(-1.0)
        full = valid[:, 0]

        def put(i, p, r, N, A, Tm):
            rows[i, 0:3], rows[i, 3], rows[i, 4:7], rows[i, 7], rows[i, 8:17], rows[i, 17] = p, r, N, A, Tm.reshape(-1, 9), T(1.0)
        put(np.arange(P - 1, 2 * P - 1)[full], p[full], _radius(leaf_box, p, T)[full], N[full], A[full], Tm[full])
        for d in range(depth - 1, -1, -1):
            i = np.arange(2**d - 1, 2**(d + 1) - 1)
            l, r = rows[2 * i + 1], rows[2 * i + 2]
            l_empty, r_empty = l[:, 3] < 0, r[:, 3] < 0
            lp, rp, lN, rN, lT, rT = l[:, 0:3], r[:, 0:3], l[:, 4:7], r[:, 4:7], l[:, 8:17].reshape(-1, 3, 3), r[:, 8:17].reshape(-1, 3, 3)
            A = l[:, 7] + r[:, 7]
            p = np.where((A > 0)[:, None], lp + (rp - lp) * (r[:, 7] / A)[:, None], _centre(box[i], T))
            N = lN + rN
            Tm = (lT + _outer(lp - p, lN)) + (rT + _outer(rp - p, rN))
            for empty, other in ((l_empty, r), (r_empty, l)):
                e1, e2, e3 = empty, empty[:, None], empty[:, None, None]
                p, N, A, Tm = np.where(e2, other[:, 0:3], p), np.where(e2, other[:, 4:7], N), np.where(e1, other[:, 7], A), \
                    np.where(e3, other[:, 8:17].reshape(-1, 3, 3), Tm)
            keep = ~(l_empty & r_empty)
            put(i[keep], p[keep], _radius(box[i], p, T)[keep], N[keep], A[keep], Tm[keep])
    return rows


def contributions(points, vertices, faces, order, leaf_size, rows, beta, order_terms, T):
    """The terms the walk of csrc/mesh_winding.hip adds for every point, found level by level -> (point index, key, term in T,
    undecided [n]).  key = the first sorted face position below the node (a face: its own position): the terms of one point come from
    disjoint subtrees, so sorting by key is the preorder in which the kernel meets them."""
    x = np.asarray(points, np.float32).astype(T)
    v = np.asarray(vertices, np.float32).astype(T)
    f, order = np.asarray(faces, np.int64), np.asarray(order, np.int64)
    n_faces = len(order)
    P, depth = shape(n_faces, leaf_size)
    rows = rows.astype(T)
    pi, node = np.arange(len(x)), np.zeros(len(x), np.int64)
    out_p, out_k, out_t = [], [], []
    undecided = np.zeros(len(x), bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for level in range(depth + 1):
            row = rows[node]
            q = x[pi]
            full = row[:, 3] >= 0
            d = row[:, 0:3] - q
            d2 = M.dot(d, d)
            br = T(beta) * row[:, 3]
            accept = full & (d2 > br * br)
            length = np.sqrt(d2)
            near = full & (np.abs(length - br) <= T(NEAR_ACCEPT) * length)
            undecided[pi[near]] = True
            i3 = T(1.0) / (d2 * length)
            term = M.dot(row[:, 4:7], d) * i3
            if order_terms >= 2:
                td = np.stack([M.dot(row[:, 8:11], d), M.dot(row[:, 11:14], d), M.dot(row[:, 14:17], d)], -1)
                trace = (row[:, 8] + row[:, 12]) + row[:, 16]
                i5 = i3 / d2
                term = term + (trace * i3 - (T(3.0) * M.dot(d, td)) * i5)
            span = 2**(depth - level) * leaf_size
            out_p.append(pi[accept]); out_k.append((node[accept] - (2**level - 1)) * span); out_t.append(term[accept])
            rest = full & ~accept
            pi, node = pi[rest], node[rest]
            if level == depth:
                for j in range(leaf_size):
                    s = (node - (P - 1)) * leaf_size + j
                    ok = s < n_faces
                    c = f[order[s[ok]]]
                    out_p.append(pi[ok]); out_k.append(s[ok])
                    out_t.append(solid_angle(x[pi[ok]], v[c[:, 0]], v[c[:, 1]], v[c[:, 2]], T))
            else:
                pi, node = np.repeat(pi, 2), np.stack([2 * node + 1, 2 * node + 2], 1).reshape(-1)
    return np.concatenate(out_p), np.concatenate(out_k), np.concatenate(out_t), undecided


def serial_sum(n, pi, key, term, T):
    """Per point the sum of its terms in the order of `key`, one rounding per addition in T, times 1 / 4 pi."""
    idx = np.lexsort((key, pi))
    pi, term = pi[idx], term[idx]
    count = np.bincount(pi, minlength=n)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    table = np.zeros((n, int(count.max()) if len(pi) else 0), T)
    table[pi, np.arange(len(pi)) - start[pi]] = term
    acc = np.zeros(n, T)
    for k in range(table.shape[1]):
        acc = acc + table[:, k]                               # a trailing 0 changes nothing
    return acc * T(INV_4PI), count


def tree(points, vertices, faces, order, leaf_size, beta, order_terms, T, rows=None, details=False):
    """w [n] in T through the tree (float64 result array for either T); details: also (undecided [n], terms per point [n])."""
    rows = moments(vertices, faces, order, leaf_size, T) if rows is None else rows
    pi, key, term, undecided = contributions(points, vertices, faces, order, leaf_size, rows, beta, order_terms, T)
    w, count = serial_sum(len(points), pi, key, term, T)
    bad = ~np.isfinite(np.asarray(points, np.float32)).all(1)
    w = np.where(bad, np.nan, w.astype(np.float64))
    return (w, undecided, count) if details else w


# ---- meshes and sets ---------------------------------------------------------------------------------------------------------------------
TWO_SPHERES_CENTRES = np.array([[0.375, 0.5, 0.5], [0.625, 0.5, 0.5]])
TWO_SPHERES_RADIUS = 0.2


def two_spheres():
    """Two icospheres at subdivision 2 (320 faces each), centres 0.25 apart, radius 0.2, concatenated unwelded: two overlapping closed
    shells."""
    parts = [M.icosphere(2, tuple(c), TWO_SPHERES_RADIUS) for c in TWO_SPHERES_CENTRES]
    return np.concatenate([p[0] for p in parts]), np.concatenate([parts[0][1], parts[1][1] + len(parts[0][0])]).astype(np.int32)


def two_spheres_sdf(x):
    """The signed distance to the UNION of the two analytic spheres wherever it is positive, and its sign everywhere."""
    x = np.asarray(x, np.float64)
    return np.min([np.linalg.norm(x - c, axis=1) for c in TWO_SPHERES_CENTRES], 0) - TWO_SPHERES_RADIUS


def two_spheres_judged(x):
    """bool [n]: farther than the sagitta of the icospheres plus 0.01 from both analytic spheres, so that the polyhedra and the spheres
    agree on inside."""
    v, f = M.icosphere(2, tuple(TWO_SPHERES_CENTRES[0]), TWO_SPHERES_RADIUS)
    tri = v[f].astype(np.float64)
    r_in = np.sqrt(np.nanmin(M.closest_on_triangle(TWO_SPHERES_CENTRES[:1], tri[:, 0], tri[:, 1], tri[:, 2], np.float64)["d2"]))
    margin = (TWO_SPHERES_RADIUS - float(r_in)) + 0.01
    x = np.asarray(x, np.float64)
    return np.all([np.abs(np.linalg.norm(x - c, axis=1) - TWO_SPHERES_RADIUS) > margin for c in TWO_SPHERES_CENTRES], 0)


HOLE_COS = 0.95                            # the cap around +z whose faces are removed: 2.5 % of the sphere as seen from the centre


def holed_sphere():
    """The icosphere (1280 faces) without the faces whose centroid lies within the cap cos(angle to +z) > HOLE_COS."""
    v, f = M.icosphere()
    c = v[f].astype(np.float64).mean(1) - 0.5
    keep = c[:, 2] / np.linalg.norm(c, axis=1) <= HOLE_COS
    return v, np.ascontiguousarray(f[keep])


def soup500():
    return M.soup(500, 3)


MESHES = {"cube": M.cube, "icosphere": M.icosphere, "torus": M.extracted_torus, "soup500": soup500, "open_quad": M.open_quad,
          "two_spheres": two_spheres, "holed_sphere": holed_sphere}
KINDS = ("uniform", "near", "far10", "far1000")
CASES = ["%s/%s" % (m, k) for m in MESHES for k in KINDS]


class Case:
    """A mesh and a point set; the references are computed once per (order of the faces, leaf size, beta, far-field terms)."""

    def __init__(self, name, vertices, faces, points, leaf_size=4):
        self.name, self.vertices, self.faces = name, np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(faces, np.int32)
        self.points, self.leaf_size = np.ascontiguousarray(points, np.float32), leaf_size
        self._exact, self._refs, self._moments = None, {}, {}

    def exact(self):
        if self._exact is None:
            self._exact = exact(self.points, self.vertices, self.faces)
        return self._exact

    def order(self):
        return morton_order(self.vertices, self.faces)

    def moments(self, order=None, leaf_size=None):
        """(boxes f32, moments float64, moments float32) of the tree over `order` (default: morton_order)."""
        order = self.order() if order is None else np.ascontiguousarray(order, np.int32)
        L = self.leaf_size if leaf_size is None else leaf_size
        key = (order.tobytes(), L)
        if key not in self._moments:
            box = boxes(self.vertices, self.faces, order, L)
            self._moments[key] = (box,) + tuple(moments(self.vertices, self.faces, order, L, T, box) for T in (np.float64, np.float32))
        return self._moments[key]

    def ref(self, beta=2.0, order_terms=2, order=None, leaf_size=None):
        """dict(exact, tree64, tree32, decided, e32, a_set, terms = the mean number of terms per point)."""
        order = self.order() if order is None else np.ascontiguousarray(order, np.int32)
        L = self.leaf_size if leaf_size is None else leaf_size
        key = (order.tobytes(), L, float(beta), order_terms)
        if key not in self._refs:
            _, m64, m32 = self.moments(order, L)
            args = (self.points, self.vertices, self.faces, order, L, beta, order_terms)
            t64, undecided, count = tree(*args, np.float64, m64, details=True)
            t32 = tree(*args, np.float32, m32)
            decided = ~undecided
            e32 = max(float(np.abs(t32 - t64)[decided].max()) if decided.any() else 0.0, ULP1)
            self._refs[key] = dict(exact=self.exact(), tree64=t64, tree32=t32, decided=decided, e32=e32,
                                   e32_all=max(float(np.abs(t32 - t64).max()), ULP1), a_set=float(np.abs(t64 - self.exact()).max()),
                                   terms=float(count.mean()))
        return self._refs[key]


_CASES = {}


def points_of(kind, v, f, rng):
    if kind == "uniform":
        return M.pts_uniform(v, 768, rng)
    if kind == "near":
        return M.pts_near(v, f, 768, rng)
    if kind == "far10":
        return M.pts_far(v, 256, rng, 10.0)
    if kind == "far1000":
        return M.pts_far(v, 256, rng, 1000.0)
    raise KeyError(kind)


def case(name):
    """The named case, built once per process."""
    if name not in _CASES:
        mesh, kind = name.split("/")
        v, f = MESHES[mesh]()
        _CASES[name] = Case(name, v, f, points_of(kind, v, f, np.random.default_rng(sum(map(ord, name)))))
    return _CASES[name]


def figures(beta=2.0):
    """Per named set and number of far-field terms: A_set, E32, the undecided fraction and the terms per point -- what
    profiles/microbench/mesh_winding.py writes to profiles/mesh_winding.json."""
    out = {}
    for name in CASES:
        c = case(name)
        for terms in (1, 2):
            r = c.ref(beta, terms)
            out["%s order %d" % (name, terms)] = {"a_set": r["a_set"], "mean_abs_error": float(np.abs(r["tree64"] - r["exact"]).mean()),
                                                  "e32": r["e32"], "undecided": 1.0 - float(r["decided"].mean()),
                                                  "terms_per_point": r["terms"], "faces": int(len(c.faces))}
    return out
