"""A serial numpy / Python statement of the simplification contract ("Simplification"; include/ngp_hip.h above
ngp_mesh_simplify_*; csrc/mesh_simplify.hip): vertex clustering on a grid with a quadric-optimal representative per cluster.

The contract.  vertices f32 [V,3], faces int32 [T,3]; the grid is lo[3], h[3] (f32), inv_h = float32(1) / h and n[3] <= 2^21 with n_x n_y n_z < 2^63.
q_k = floor((x_k - lo_k) * inv_h_k) in float32 (one subtraction, one multiplication), clamped to [0, n_k - 1] in float, key = q_x +
n_x (q_y + n_y q_z).  A vertex with a coordinate that is not finite is bad (no cluster); a face with an index outside [0, V) or a bad
vertex is bad (face_map -1).  Clusters are the distinct keys, numbered by increasing key.  A good face survives when its corners lie in
three distinct clusters; survivors keep their order and their corner order; output vertices are the clusters a survivor names, numbered
by increasing key.  Every good face with area adds its quadric, relative to the cell centre c = lo + (q + 1/2) h, once to each distinct
cluster among its corners (the faces that collapse included): with nn = (b - a) x (c' - a), w = |nn| / 2, n = nn / |nn|, d = -n . (a - c):
A += w n n^T, b += w d n, area vector += nn / 2.  mean = sum (v - c) / count over the cluster's vertices, mu = regularization tr(A),
y = (A + mu I)^-1 (-b + mu mean), y = mean when tr(A) = 0 or regularization = inf; y clamped to [-h / 2, h / 2]; x = float32(c + y).
The normal is the normalised area vector, zero where that is zero.  "Has area" is decided by |nn|^2 > 0 with nn formed in float64 as
u_1 w_2 - u_2 w_1 etc., every product, difference and sum a rounding of its own, (nn_0^2 + nn_1^2) + nn_2^2: device and reference run
the same operations, so the decision -- and with it every integer output -- is compared for EQUALITY.

FLOATS.  Here every sum is math.fsum (exact, rounded once) and the system is solved by numpy.linalg.solve in float64.  The device sums
in another order and solves by LDL^T.  With u = 2^-53, m the incidences of the cluster and p its vertices, the position bound is

    bound_k = min(E, h_k) + 2^-23 |x_k| + 2^-149
    E = 2 [ (sqrt(3) g S + (3 + eps) g tr(A) |y| + mu g_v |Y| + mu g |mean|) / mu  +  64 u ((1 + eps) / eps) |y| ]        (quadric)
    E = 2 g_v |Y|                                                                                                            (mean)
    g = (m + 32) 2^-52,  g_v = (p + 32) 2^-52,  S = sum_f w_f |a_f - c|,  Y_k = sum_v |v_k - c_k| / p,  eps = regularization

and y the unclamped solution.  Its parts:
(1) The sums.  Any order of adding m float64 terms is within m u sum |t| (1 + 2 m u) of the exact sum (Higham, Accuracy and Stability
of Numerical Algorithms, section 4.2); a term itself (differences, a cross product, a norm, a division, three or four products: under
thirty roundings) is within 32 u of its size bound on either side, together (2 m + 64) u = (m + 32) 2^-52 = g times the size bound.
The size bounds: |w n_i n_j| <= w, and the w sum to tr(A), so |dA_ij| <= g tr(A) and ||dA||_2 <= ||dA||_F <= 3 g tr(A);
|w d n_i| <= w |a - c| (d = -n . (a - c) and its own rounding error are both relative to |a - c|), so ||db||_2 <= sqrt(3) g S;
|d mean_k| <= g_v Y_k; |d mu| <= g mu.
(2) The system M y = r, M = A + mu I, r = -b + mu mean.  A is positive semi-definite with trace sum w, so the eigenvalues of M lie in
[mu, (1 + eps) tr(A)]: ||M^-1|| <= 1 / mu and the condition number is at most (1 + eps) / eps.  To first order
dy = M^-1 (dr - dM y) with ||dM|| <= (3 + eps) g tr(A) and ||dr|| <= sqrt(3) g S + mu g_v |Y| + mu g |mean|.
(3) The solvers.  Both (LU with partial pivoting here, LDL^T there) are backward stable for a 3 x 3 positive definite matrix: a relative
forward error below 64 u times the condition number on either side.
The factor 2 in front covers the second-order terms and the two sides (the reference's own sums are exact, so most of it is spare).
(4) The clamp is 1-Lipschitz, so it only shrinks the difference, and both sides end inside [-h / 2, h / 2]: min(E, h_k).  (For a cluster
whose faces reach 3e38 E says nothing and h_k is the bound.)
(5) x = float32(c + y): rounding is monotone, so two values E apart round to values at most E plus one float32 spacing (<= 2^-23 |x|,
2^-149 for a denormal) apart.  The float64 rounding of c and of c + y, 4 u (|c| + |y|), is added to E.
For an ordinary mesh E is about 10^-10 h and the float32 spacing dominates.

Normals: |dN_k| <= g tr(A) (|nn_k / 2| <= w), and normalising a vector N perturbed by dN moves it by at most 2 |dN| / |N|:
normal_bound = min(2, 2 * 2 sqrt(3) g tr(A) / |N|) + 2^-23 -- 2 where N cancels to (about) nothing: there one side may write the zero
vector and the other a unit vector."""
import math

import numpy as np

import mesh_sdf_reference as M

INT64_MAX = 2**63 - 1
INT_MIN = -2**31
U52 = 2.0**-52


# ---- the grid and the keys ------------------------------------------------------------------------------------------------------------
def _grid(lo, h, n):
    lo, h = np.asarray(lo, np.float32).reshape(3), np.asarray(h, np.float32).reshape(3)
    n = np.asarray(n, np.int64).reshape(3)
    assert np.isfinite(lo).all() and (h > 0).all() and np.isfinite(h).all() and (n >= 1).all() and (n <= 2**21).all() and int(n[0]) * int(n[1]) * int(n[2]) < 2**63
    return lo, h, np.float32(1.0) / h, n


def keys(vertices, lo, h, n):
    """-> (key int64 [V], INT64_MAX for a bad vertex; q int64 [V,3])"""
    lo, h, inv_h, n = _grid(lo, h, n)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    bad = ~np.isfinite(v).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((v - lo) * inv_h)                         # float32 throughout
        q = np.where(q > 0, q, np.float32(0))                  # the clamp, in float (a NaN of a bad vertex goes to 0 and is not used)
        q = np.where(q < (n - 1).astype(np.float32), q, (n - 1).astype(np.float32))
    assert q.dtype == np.float32
    q = q.astype(np.int64)
    key = q[:, 0] + n[0] * (q[:, 1] + n[1] * q[:, 2])
    return np.where(bad, INT64_MAX, key), q


def _area_vector(a, b, c):
    """float64 rows a, b, c -> (nn [.,3], |nn|^2), in the contract's order of operations"""
    u, w = b - a, c - a
    nn = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    return nn, (nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2]


# ---- the integer part -----------------------------------------------------------------------------------------------------------------
def count(vertices, faces, lo, h, n):
    """The count phase -> dict(vertex_cluster, vertex_map, face_map, faces (the output faces), n_clusters, n_vertices, n_faces,
    bad_vertices, bad_faces, cluster_key [C], out_cluster [V'], good [T])"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    key, _ = keys(v, lo, h, n)
    cluster_key = np.unique(key[key != INT64_MAX])             # sorted: numbered by increasing key
    vc = np.where(key != INT64_MAX, np.searchsorted(cluster_key, key), -1).astype(np.int32)
    in_range = ((f >= 0) & (f < V)).all(1) if len(f) else np.zeros(0, bool)
    fc = np.full((len(f), 3), -1, np.int64)
    fc[in_range] = vc[f[in_range]]
    good = in_range & (fc >= 0).all(1)
    survives = good & (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 2] != fc[:, 0])
    used = np.zeros(len(cluster_key), bool)
    used[fc[survives].reshape(-1)] = True
    cluster_out = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    vertex_map = (np.where(vc >= 0, cluster_out[np.maximum(vc, 0)], -1) if len(cluster_key) else np.full(V, -1)).astype(np.int32)
    face_map = np.where(survives, np.cumsum(survives) - 1, -1).astype(np.int32)
    return {"vertex_cluster": vc, "vertex_map": vertex_map, "face_map": face_map,
            "faces": cluster_out[fc[survives]].astype(np.int32).reshape(-1, 3), "n_clusters": int(len(cluster_key)),
            "n_vertices": int(used.sum()), "n_faces": int(survives.sum()), "bad_vertices": int((key == INT64_MAX).sum()),
            "bad_faces": int((~good).sum()), "cluster_key": cluster_key, "out_cluster": np.flatnonzero(used), "good": good,
            "face_cluster": fc}


# ---- the representatives ----------------------------------------------------------------------------------------------------------------
def _group_fsum(ids, rows, n_groups):
    """rows [m,k] float64 summed per id with math.fsum, column by column -> ([n_groups,k], members per group)"""
    order = np.argsort(ids, kind="stable")
    ids, rows = ids[order], rows[order]
    counts = np.bincount(ids, minlength=n_groups)
    start = np.concatenate([[0], np.cumsum(counts)])
    out = np.zeros((n_groups, rows.shape[1]))
    one = counts == 1
    out[one] = rows[start[:-1][one]]
    for g in np.flatnonzero(counts > 1).tolist():
        seg = rows[start[g]:start[g + 1]]
        out[g] = [math.fsum(seg[:, j]) for j in range(seg.shape[1])]
    return out, counts


def simplify(vertices, faces, lo, h, n, regularization=1e-3):
    """-> count()'s dict plus vertices f32 [V',3], normals f32 [V',3], bound [V',3], normal_bound [V'] (the module docstring)"""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lo32, h32, _, n3 = _grid(lo, h, n)
    out = count(v32, f, lo32, h32, n3)
    eps = float(regularization)
    assert eps > 0.0
    C, ck, h64 = out["n_clusters"], out["cluster_key"], h32.astype(np.float64)
    q = np.stack([ck % n3[0], ck // n3[0] % n3[1], ck // (n3[0] * n3[1])], 1).astype(np.float64) if C else np.zeros((0, 3))
    centre = lo32.astype(np.float64) + (q + 0.5) * h64
    # the incidences: one row per (face with area, distinct cluster among its corners):
    # w n n^T [6], w d n [3], nn / 2 [3], w, w |a - c|
    gf = np.flatnonzero(out["good"])
    with np.errstate(over="ignore", invalid="ignore"):
        a = v32[f[gf, 0]].astype(np.float64)
        nn, len2 = _area_vector(a, v32[f[gf, 1]].astype(np.float64), v32[f[gf, 2]].astype(np.float64))
    has = len2 > 0.0
    a, nn, cl = a[has], nn[has], out["face_cluster"][gf[has]]
    length = np.sqrt(len2[has])
    w, nrm = 0.5 * length, nn / length[:, None]
    ids, rows = [], []
    for k, first in enumerate((np.ones(len(cl), bool), cl[:, 1] != cl[:, 0], (cl[:, 2] != cl[:, 0]) & (cl[:, 2] != cl[:, 1]))):
        c_k = cl[first, k]
        rel = a[first] - centre[c_k]
        wk, nk = w[first], nrm[first]
        d = -(nk * rel).sum(1)
        ids.append(c_k)
        rows.append(np.concatenate([np.stack([wk * nk[:, 0] * nk[:, 0], wk * nk[:, 0] * nk[:, 1], wk * nk[:, 0] * nk[:, 2], wk * nk[:, 1] * nk[:, 1],
                                              wk * nk[:, 1] * nk[:, 2], wk * nk[:, 2] * nk[:, 2]], 1), (wk * d)[:, None] * nk, 0.5 * nn[first],
                                    wk[:, None], (wk * np.linalg.norm(rel, axis=1))[:, None]], 1))
    s, m = _group_fsum(np.concatenate(ids), np.concatenate(rows), C)
    live = np.flatnonzero(out["vertex_cluster"] >= 0)
    rel = v32[live].astype(np.float64) - centre[out["vertex_cluster"][live]]
    sv, p = _group_fsum(out["vertex_cluster"][live].astype(np.int64), np.concatenate([rel, np.abs(rel)], 1), C)
    oc = out["out_cluster"]                                     # from here on: the output vertices only
    s, m, sv, p, centre = s[oc], m[oc], sv[oc], p[oc][:, None].astype(np.float64), centre[oc]
    mean, Y = sv[:, :3] / p, sv[:, 3:] / p
    g, gv = (m + 32) * U52, (p[:, 0] + 32) * U52
    A = np.stack([s[:, [0, 1, 2]], s[:, [1, 3, 4]], s[:, [2, 4, 5]]], 1)
    bvec, N, trace, S = s[:, 6:9], s[:, 9:12], s[:, 12], s[:, 13]
    norm = lambda x: np.linalg.norm(x, axis=1)
    y = mean.copy()
    E = 2.0 * gv * norm(Y)
    solve = np.flatnonzero(trace > 0.0) if eps < math.inf else np.zeros(0, np.int64)
    if len(solve):
        mu = eps * trace[solve]
        ys = np.linalg.solve(A[solve] + mu[:, None, None] * np.eye(3), (-bvec[solve] + mu[:, None] * mean[solve])[:, :, None])[:, :, 0]
        y[solve] = ys
        E[solve] = 2.0 * ((math.sqrt(3.0) * g[solve] * S[solve] + (3.0 + eps) * g[solve] * trace[solve] * norm(ys) + mu * gv[solve] * norm(Y[solve])
                           + mu * g[solve] * norm(mean[solve])) / mu + 64 * 2.0**-53 * ((1.0 + eps) / eps) * norm(ys))
    with np.errstate(invalid="ignore"):
        E = np.where(np.isfinite(E), E, np.inf) + 4 * 2.0**-53 * (np.abs(centre).max(1, initial=0.0) + np.abs(y).max(1, initial=0.0))
    pos = (centre + np.clip(y, -0.5 * h64, 0.5 * h64)).astype(np.float32)
    bound = np.minimum(E[:, None], h64) + 2.0**-23 * np.abs(pos.astype(np.float64)) + 2.0**-149
    length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = np.where(length[:, None] > 0.0, N / length[:, None], 0.0).astype(np.float32)
        nbound = np.where(length > 0.0, np.minimum(2.0, 4.0 * math.sqrt(3.0) * g * trace / length), 2.0) + 2.0**-23
    out.update(vertices=pos, normals=normals, bound=bound, normal_bound=nbound)
    return out


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def tessellated_cube(k=24, lo=0.25, hi=0.75):
    """The box [lo, hi]^3 with k x k quads per side, welded, outward: 6 k^2 + 2 vertices, 12 k^2 faces."""
    index, verts, faces = {}, [], []

    def vid(i, j, l):
        if (i, j, l) not in index:
            index[(i, j, l)] = len(verts)
            verts.append([lo + (hi - lo) * i / k, lo + (hi - lo) * j / k, lo + (hi - lo) * l / k])
        return index[(i, j, l)]
    for axis in range(3):
        for side in (0, k):
            for s in range(k):
                for t in range(k):
                    def corner(ds, dt):
                        ijk = [0, 0, 0]
                        ijk[axis], ijk[(axis + 1) % 3], ijk[(axis + 2) % 3] = side, s + ds, t + dt
                        return vid(*ijk)
                    quad = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]      # counter-clockwise seen along +axis
                    if side == 0:
                        quad = quad[::-1]
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return np.array(verts, np.float32), np.array(faces, np.int32)


CUBE_CORNERS = np.array([[x, y, z] for x in (0.25, 0.75) for y in (0.25, 0.75) for z in (0.25, 0.75)], np.float64)


def volume(vertices, faces):
    t = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def corner_distance(vertices):
    """the farthest true cube corner to its nearest vertex"""
    d = np.linalg.norm(np.asarray(vertices, np.float64)[None] - CUBE_CORNERS[:, None], axis=2)
    return float(d.min(1).max())


def tilted_patch(k=20, seed=3):
    """A planar patch of 2 k^2 triangles in the plane z = x / 2 + y / 4 + 1 / 8, tilted against every axis.  x and y are jittered
    multiples of 2^-8, so every coordinate is a short binary fraction: the float32 vertices lie EXACTLY in the plane, and the face normals
    are exactly parallel.  -> (vertices, faces, unit normal f64, a point of the plane)"""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing="ij"), -1).reshape(-1, 2)
    xy = (8 * ij + rng.integers(-2, 3, ij.shape)) / 256.0
    v = np.concatenate([xy, 0.5 * xy[:, :1] + 0.25 * xy[:, 1:] + 0.125], 1)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    nrm = np.array([-0.5, -0.25, 1.0]) / np.linalg.norm([-0.5, -0.25, 1.0])
    idx = lambda i, j: i * (k + 1) + j
    f = [t for i in range(k) for j in range(k) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return v.astype(np.float32), np.array(f, np.int32), nrm, np.array([0.0, 0.0, 0.125])


def spaced_triangles(n, spacing=1.0, size=0.25):
    """n disjoint triangles whose 3 n vertices are pairwise at least `size` apart along x: alone in their cells for h < size"""
    i = np.arange(3 * n, dtype=np.float64)
    v = np.stack([size * i + spacing * (i // 3), (i % 3 == 1) * size, (i % 3 == 2) * size], 1)
    return v.astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def hub_fan(n_faces=10**4):
    """n_faces triangles around one hub: the hub's cluster owns an incidence of every face; the rim lies on a circle of radius 1"""
    t = 2 * np.pi * np.arange(n_faces) / n_faces
    v = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(t), np.sin(t), np.zeros(n_faces)], 1)]).astype(np.float32)
    k = np.arange(n_faces)
    return v, np.stack([np.zeros(n_faces, np.int64), 1 + k, 1 + (k + 1) % n_faces], 1).astype(np.int32)


def box_of(vertices):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    return (v.min(0), v.max(0)) if len(v) else (np.zeros(3, np.float32), np.zeros(3, np.float32))


NAMED = {"cube": M.cube, "icosphere": M.icosphere, "torus": M.extracted_torus, "open_quad": M.open_quad, "needle": M.needle_tetrahedron,
         "soup500": lambda: M.soup(500, 11)}
