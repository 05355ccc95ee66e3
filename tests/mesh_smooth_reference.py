"""The serial statement of the smoothing contract (include/ngp_hip.h, "mesh smoothing"; DESIGN.md section 3, "Smoothing"): the vertex
adjacency, one smoothing pass, the Taubin iteration and the area-weighted vertex normals, in numpy alone.  It imports neither the package
nor the oracle, and it does not sort the keys the device sorts: the adjacency is a dictionary of Python sets filled face by face.

THE CONTRACT IN SHORT.  A face is GOOD when its three indices lie in [0, V) and are distinct; a vertex is BAD when a coordinate is not
finite.  Every good face makes its three corners pairwise neighbours.  The multiplicity of an edge is the number of good faces that use
it in either orientation (cut at 255).  Vertex flags: 1 boundary (an incident edge of multiplicity 1), 2 non-manifold (one of
multiplicity >= 3), 4 unused (no good face), 8 bad.  A pass moves vertex i, unless it is bad, unused, pinned, without a neighbour that
counts, or a boundary vertex in "fixed" mode, to
    s = sum of x_j over N(i) in ascending j (f64, serial);  m = s / |N(i)|;  y = x_i + factor (m - x_i);  x' = float32(y);
    lo = x0_i - max_move, hi = x0_i + max_move (float32);  x' = lo if x' < lo;  x' = hi if x' > hi
where N(i) leaves out bad neighbours and, for a boundary vertex in "curve" mode, every neighbour across an edge of multiplicity != 1.

THE COMPARISON BOUNDS.
  One pass.  The device and this file perform the same IEEE operations on the same float32 inputs in the same order: conversions to
  float64 (exact), a serial float64 sum, one division, one subtraction, one multiplication, one addition (the library is compiled without
  contraction), one rounding to float32 and two float32 comparisons.  Every one of these is correctly rounded on both sides, so the
  result is expected to be BIT-IDENTICAL.  The bound the tests assert is nevertheless one float32 spacing of the result per coordinate:
  a different evaluation of y that is off by a few float64 roundings can change the float32 rounding by one step at most.
  k passes.  If the inputs of a pass differ by at most e in every coordinate, the means differ by at most e, so y differs by at most
  (|1 - factor| + |factor|) e, and the rounding adds one spacing u of the result (|fl(a) - fl(b)| <= |a - b| + u); the clamp is
  monotone and 1-Lipschitz and adds nothing.  Hence e_0 = 0, e_p = (|1 - f_p| + |f_p|) e_(p-1) + u_p with u_p the float32 spacing of the
  largest finite |coordinate| after pass p.  smooth() returns e_k as `bound`; the float64 roundings (2^-53 relative) are covered by
  taking u_p whole where half of it would do.
  Normals.  The float64 sum of d area vectors has the error (d + 4) 2^-53 A at most, A the sum of the absolute products that enter it;
  dividing by the length L turns that into a direction error of at most 2 (d + 4) 2^-53 A / L, the normalisation adds 4 x 2^-53, and the
  rounding of the three components to float32 adds sqrt(3) 2^-24 between two results.  vertex_normals() returns
  normal_bound = sqrt(3) 2^-24 + 4 (d + 4) 2^-53 A / L per vertex (Euclidean); where L is 0 or not finite the normal is exactly 0 and
  the bound is the rounding term alone.  Again the operations are the same on both sides and bit identity is expected.
The tests print the worst ratio to these bounds and how many cases were bit-identical."""
import math

import numpy as np

import mesh_components_reference as C
import mesh_sdf_reference as M
import mesh_simplify_reference as S

BOUNDARY, NONMANIFOLD, UNUSED, BAD = 1, 2, 4, 8
MAX_MULTIPLICITY = 255
PASS_BAND = 0.1
MODES = ("fixed", "curve", "free")


def taubin_mu(lam, pass_band=PASS_BAND):
    return 1.0 / (pass_band - 1.0 / lam)


def good_faces(faces, n_vertices):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < n_vertices)).all(1)
    distinct = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    return inside & distinct


def adjacency(vertices, faces):
    """-> dict(row_start int32 [V + 1], neighbours int32 [E2], multiplicity uint8 [E2], vertex_flags uint8 [V], counts = (E2, bad faces,
    bad vertices, boundary vertices)).  Sets and a dictionary, face by face."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n_vertices = len(v)
    good = good_faces(f, n_vertices)
    rows = [set() for _ in range(n_vertices)]
    uses = {}
    for a, b, c in f[good].tolist():
        for u, w in ((a, b), (b, c), (c, a)):
            rows[u].add(w); rows[w].add(u)
            e = (u, w) if u < w else (w, u)
            uses[e] = uses.get(e, 0) + 1
    row_start = np.zeros(n_vertices + 1, np.int64)
    neighbours, multiplicity = [], []
    flags = np.zeros(n_vertices, np.uint8)
    bad = ~np.isfinite(v).all(1)
    for u in range(n_vertices):
        nb = sorted(rows[u])
        mult = [uses[(u, w) if u < w else (w, u)] for w in nb]
        neighbours += nb
        multiplicity += [min(m, MAX_MULTIPLICITY) for m in mult]
        row_start[u + 1] = len(neighbours)
        flags[u] = (BOUNDARY if 1 in mult else 0) | (NONMANIFOLD if any(m >= 3 for m in mult) else 0) | (0 if nb else UNUSED) | (BAD if bad[u] else 0)
    counts = (len(neighbours), int((~good).sum()), int(bad.sum()), int(((flags & BOUNDARY) != 0).sum()))
    return {"row_start": row_start.astype(np.int32), "neighbours": np.asarray(neighbours, np.int32).reshape(-1),
            "multiplicity": np.asarray(multiplicity, np.uint8).reshape(-1), "vertex_flags": flags, "counts": counts}


def brute_force_adjacency(vertices, faces):
    """The same dictionary by the O(T V) definition: for every vertex, every face is looked at."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3).tolist()
    n_vertices = len(v)
    ok = [all(0 <= i < n_vertices for i in t) and len(set(t)) == 3 for t in f]
    row_start, neighbours, multiplicity, flags = [0], [], [], []
    for u in range(n_vertices):
        nb = sorted({w for t, g in zip(f, ok) if g and u in t for w in t if w != u})
        mult = [sum(1 for t, g in zip(f, ok) if g and u in t and w in t) for w in nb]
        neighbours += nb
        multiplicity += [min(m, MAX_MULTIPLICITY) for m in mult]
        row_start.append(len(neighbours))
        flags.append((BOUNDARY if 1 in mult else 0) | (NONMANIFOLD if any(m >= 3 for m in mult) else 0) | (0 if nb else UNUSED)
                     | (0 if np.isfinite(v[u]).all() else BAD))
    flags = np.asarray(flags, np.uint8).reshape(-1)
    counts = (len(neighbours), len(f) - sum(ok), int((~np.isfinite(v).all(1)).sum()), int(((flags & BOUNDARY) != 0).sum()))
    return {"row_start": np.asarray(row_start, np.int32), "neighbours": np.asarray(neighbours, np.int32).reshape(-1),
            "multiplicity": np.asarray(multiplicity, np.uint8).reshape(-1), "vertex_flags": flags, "counts": counts}


def _ranked(row_of, keep):
    """The kept entries of a CSR grouped by their rank within their row: [(rows, entries)] for rank 0, 1, ...; adding group after group
    is the serial sum of every row in ascending entry order."""
    idx = np.flatnonzero(keep)
    if not len(idx):
        return [], np.zeros(0, np.int64)
    rows = row_of[idx]
    first = np.r_[True, rows[1:] != rows[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(len(idx)), 0))
    rank = np.arange(len(idx)) - start
    order = np.argsort(rank, kind="stable")
    cuts = np.flatnonzero(np.diff(rank[order])) + 1
    return [(rows[g], idx[g]) for g in np.split(order, cuts)], rows


def smooth_pass(x_in, x0, adj, factor, mode="fixed", fixed=None, max_move=None):
    """One pass -> float32 [V,3].  x_in, x0 float32; max_move None or three float32 values."""
    assert mode in MODES
    x = np.asarray(x_in, np.float32).reshape(-1, 3)
    n_vertices = len(x)
    flags, nb, mult = adj["vertex_flags"], adj["neighbours"].astype(np.int64), adj["multiplicity"]
    row_start = adj["row_start"].astype(np.int64)
    row_of = np.repeat(np.arange(n_vertices), np.diff(row_start))
    boundary = (flags & BOUNDARY) != 0
    keep = (flags[nb] & BAD) == 0
    if mode == "curve":
        keep &= ~boundary[row_of] | (mult == 1)
    groups, rows = _ranked(row_of, keep)
    s = np.zeros((n_vertices, 3), np.float64)
    for r, e in groups:                                        # rank by rank: every row's sum is serial, in ascending neighbour
        s[r] += x[nb[e]].astype(np.float64)
    count = np.bincount(rows, minlength=n_vertices)
    moves = ((flags & (UNUSED | BAD)) == 0) & (count > 0)
    if fixed is not None:
        moves &= np.asarray(fixed).reshape(-1) == 0
    if mode == "fixed":
        moves &= ~boundary
    out = x.copy()
    i = np.flatnonzero(moves)
    with np.errstate(all="ignore"):
        xi = x[i].astype(np.float64)
        m = s[i] / count[i, None].astype(np.float64)
        d = m - xi
        p = np.float64(factor) * d
        y = xi + p
        r = y.astype(np.float32)
        if max_move is not None:
            mm = np.broadcast_to(np.asarray(max_move, np.float32).reshape(-1), (3,))
            o = np.asarray(x0, np.float32).reshape(-1, 3)[i]
            lo, hi = o - mm, o + mm                            # float32
            r = np.where(r < lo, lo, r)
            r = np.where(r > hi, hi, r)
    out[i] = r
    return out


def _spacing(x):
    a = np.abs(x[np.isfinite(x)])
    return float(np.spacing(np.float32(a.max()))) if a.size else 0.0


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", fixed=None, max_move=None, adj=None):
    """The Taubin iteration -> dict(vertices float32 [V,3], bound: the module docstring's e_k, passes, adjacency)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    adj = adjacency(v, faces) if adj is None else adj
    if mu is None:
        mu = taubin_mu(lam)
    factors = [lam] if mu == 0.0 else [lam, mu]
    x, bound, passes = v.copy(), 0.0, 0
    for _ in range(int(iterations)):
        for f in factors:
            x = smooth_pass(x, v, adj, f, boundary, fixed, max_move)
            bound = (abs(1.0 - f) + abs(f)) * bound + _spacing(x)
            passes += 1
    return {"vertices": x, "bound": bound, "passes": passes, "adjacency": adj}


def vertex_normals(vertices, faces):
    """-> (normals float32 [V,3], normal_bound f64 [V]).  The incidence slots 3 f + k of the good faces, taken vertex by vertex in
    ascending slot order."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n_vertices = len(v)
    if n_vertices == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.float64)
    good = good_faces(f, n_vertices)
    slots = np.flatnonzero(np.repeat(good, 3))
    vert = f.reshape(-1)[slots]
    order = np.argsort(vert, kind="stable")                    # by vertex, then by slot
    slots, vert = slots[order], vert[order]
    face = slots // 3
    with np.errstate(all="ignore"):
        fa = good_or_zero(f, good)
        a = v[fa[:, 0]].astype(np.float64)
        u = v[fa[:, 1]].astype(np.float64) - a
        w = v[fa[:, 2]].astype(np.float64) - a
        p, q = u[:, [1, 2, 0]] * w[:, [2, 0, 1]], u[:, [2, 0, 1]] * w[:, [1, 2, 0]]
        area = 0.5 * (p - q)                                   # [T,3]; rows of bad faces are not used
        mag = 0.5 * (np.abs(p) + np.abs(q)).sum(1)
        s = np.zeros((n_vertices, 3), np.float64)
        big = np.zeros(n_vertices, np.float64)
        groups, _ = _ranked(vert, np.ones(len(vert), bool))
        for r, e in groups:
            s[r] += area[face[e]]
            big[r] += mag[face[e]]
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = (length > 0.0) & (length < np.inf)
        n = np.where(ok[:, None], s / np.where(ok, length, 1.0)[:, None], 0.0).astype(np.float32)
        degree = np.bincount(vert, minlength=n_vertices)
        bound = math.sqrt(3.0) * 2.0**-24 + np.where(ok, 4.0 * (degree + 4) * 2.0**-53 * big / np.where(ok, length, 1.0), 0.0)
    return n, bound


def good_or_zero(f, good):
    """The faces with the bad ones replaced by (0, 0, 0) -- so that they can be gathered; their rows are never used."""
    return np.where(good[:, None], f, 0)


# ---- measures ---------------------------------------------------------------------------------------------------------------------------
volume = S.volume


def radial_rms(vertices, centre, radius):
    r = np.linalg.norm(np.asarray(vertices, np.float64) - np.asarray(centre, np.float64), axis=1)
    return float(np.sqrt(np.mean((r - radius) ** 2)))


def max_move_holds(x, x0, max_move):
    """The guarantee as the contract's clamp states it, in float32: fl(x0 - max_move) <= x <= fl(x0 + max_move) on every coordinate
    (so |x - x0| <= max_move up to the one rounding of the bound itself, half a spacing of |x0| + max_move) -> the share of
    coordinates that sit on a bound."""
    x, x0 = np.asarray(x, np.float32), np.asarray(x0, np.float32)
    mm = np.broadcast_to(np.asarray(max_move, np.float32).reshape(-1), (3,))
    lo, hi = x0 - mm, x0 + mm
    assert lo.dtype == np.float32 and (x >= lo).all() and (x <= hi).all()
    slack = 0.5 * np.spacing(np.abs(x0) + mm).astype(np.float64)
    assert (np.abs(x.astype(np.float64) - x0.astype(np.float64)) <= mm.astype(np.float64) + slack).all()
    return float(((x == lo) | (x == hi)).mean())


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
disjoint_triangles, strip = C.disjoint_triangles, C.strip
hub_fan, tessellated_cube = S.hub_fan, S.tessellated_cube


def octahedron():
    """The regular octahedron with the vertices +-e_k, outward.  The neighbours of +-e_k are the four vertices of the other two axes,
    whose mean is 0: a pass with the factor f scales the shape by exactly 1 - f."""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def dyadic_patch(k=8):
    """A square patch of (k + 1)^2 grid points with the coordinates (i, j, 0) / 8, every quad split along the same diagonal: an interior
    vertex has six neighbours placed symmetrically around it, so their sum is exactly six times the vertex."""
    idx = lambda i, j: i * (k + 1) + j
    v = np.array([[i / 8.0, j / 8.0, 0.0] for i in range(k + 1) for j in range(k + 1)], np.float32)
    f = [t for i in range(k) for j in range(k) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return v, np.array(f, np.int32)


def open_cylinder(n_around=48, n_along=12, radius=0.25, length=1.0, noise=0.004, seed=5):
    """An open cylinder around the z axis, n_along + 1 rings of n_around vertices, with seeded noise on every coordinate; ring r is the
    vertices r n_around .. (r + 1) n_around - 1, the two boundary rings are the first and the last.  -> (vertices, faces, clean vertices)"""
    t = 2 * np.pi * np.arange(n_around) / n_around
    rings = [np.stack([radius * np.cos(t), radius * np.sin(t), np.full(n_around, length * r / n_along)], 1) for r in range(n_along + 1)]
    clean = np.concatenate(rings)
    v = clean + np.random.default_rng(seed).normal(0.0, noise, clean.shape)
    idx = lambda r, a: r * n_around + a % n_around
    f = [t for r in range(n_along) for a in range(n_around)
         for t in ((idx(r, a), idx(r, a + 1), idx(r + 1, a + 1)), (idx(r, a), idx(r + 1, a + 1), idx(r + 1, a)))]
    return v.astype(np.float32), np.array(f, np.int32), clean


def noisy_icosphere(subdivisions=3, amplitude=0.01, seed=1, centre=(0.5, 0.5, 0.5), radius=0.35):
    """M.icosphere with seeded radial noise of the standard deviation `amplitude`."""
    v, f = M.icosphere(subdivisions, centre=centre, radius=radius)
    d = v.astype(np.float64) - np.asarray(centre)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = radius + np.random.default_rng(seed).normal(0.0, amplitude, len(v))
    return (np.asarray(centre) + d * r[:, None]).astype(np.float32), f


def messy(duplicates=3):
    """Everything the adjacency has to survive in one mesh of 12 vertices: a face listed `duplicates` times, a face in both
    orientations, an edge shared by three faces, indices out of range, repeated indices, an isolated vertex (10) and a NaN vertex (11,
    named by a good face).  duplicates >= 256 takes the duplicated face's edges past the multiplicity's cut."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.25], [0.5, 0.5, 1], [2, 0, 0], [2, 1, 0.5], [0, 2, 0], [1, 2, 0.5], [3, 3, 3],
                  [9, 9, 9], [np.nan, 0, 0]], np.float32)
    f = [[0, 1, 2]] * duplicates + [[1, 3, 2], [2, 3, 1],                   # both orientations
                                    [0, 1, 4], [1, 0, 5],                    # the edge 0-1: the duplicates, and two more
                                    [1, 5, 6], [2, 7, 8], [3, 8, 9],
                                    [0, 1, 12], [-1, 2, 3], [2 ** 31 - 1, 0, 1],      # out of range
                                    [4, 4, 5], [6, 7, 6], [8, 8, 8],         # repeated
                                    [5, 6, 11], [6, 9, 11]]                  # the NaN vertex, in good faces
    return v, np.array(f, np.int32)


def cancelling():
    """Vertex 0 lies in two faces that are each other's mirror image in orientation: its area vectors cancel exactly, its normal is 0;
    vertex 3 has one face of its own."""
    v = np.array([[0.25, 0.5, 0.125], [1, 0, 0], [0, 1, 0.5], [2, 2, 2], [3, 2, 2], [2, 3, 2]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 1], [3, 4, 5]], np.int32)


CLOSED = {"cube": M.cube, "icosphere": M.icosphere, "torus": M.extracted_torus, "needle": M.needle_tetrahedron,
          "tessellated_cube": lambda: tessellated_cube(6), "octahedron": octahedron, "noisy_icosphere": noisy_icosphere}
OPEN = {"patch": dyadic_patch, "cylinder": lambda: open_cylinder()[:2], "fan": lambda: hub_fan(10**4), "open_quad": M.open_quad}
_CACHE = {}


def case(name):
    """(vertices, faces, adjacency) of a named mesh, computed once; callers must not modify them."""
    if name not in _CACHE:
        v, f = (CLOSED.get(name) or OPEN[name])()
        _CACHE[name] = (v, f, adjacency(v, f))
    return _CACHE[name]
