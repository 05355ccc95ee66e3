"""A serial numpy / Python statement of the connected-components contract ("Connected components";
csrc/mesh_components.hip): a plain union-find, the numbering rule, the per-component table, the selection and the rule of clean_mesh.

The contract.  faces int32 [T,3] over V vertices.  Two vertices are connected when some face names both.  A face with an index outside
[0, V) is bad: it joins nothing, has component -1 and is counted; a face that repeats an index still joins its vertices.  A vertex named
by no good face is unused: component -1, counted.  Components are numbered 0 .. C - 1 by increasing smallest vertex index.
Edges are the distinct undirected pairs of the good faces with three distinct indices; an edge used once is a boundary edge, one used
three or more times a non-manifold edge; euler = vertices - edges + faces.  The box is the exact minimum and maximum of the coordinates
of the component's vertices, -0 ordered below +0.

FLOATS.  The truth for area and volume is: the per-face term in numpy float64 from the float32 coordinates, summed per component with
math.fsum (the exact sum of the terms, rounded once).  With u = 2^-53, the bound for a component of n faces is

    (n + 16) 2^-52 sum_f m_f  =  (2 n + 32) u sum_f m_f,    m_f = |b - a| |c - a| / 2 (area),   m_f = |a| |b| |c| / 6 (volume),

m_f being what the size of the term t_f cannot pass (|x cross y| <= |x||y|, |a . (b cross c)| <= |a||b||c|).  It has two parts.
(1) The sum.  Any order of adding n float64 numbers is off the exact sum by at most gamma_(n-1) sum |t_f| with gamma_k = k u / (1 - k u)
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), below n u sum m_f (1 + 2 n u); fsum itself adds one rounding of
the result, u |sum| <= u sum m_f.  That is the `n` of the factor, counted in units of 2 u, with half of it to spare.
(2) The terms.  The device and numpy may round a term differently (operation order; both without fused multiply-adds), each at most
16 u m_f away from the exact term: area -- three differences (u each, relative), six products and three differences of a cross product
(each component within 3 u (|x_j y_k| + |x_k y_j|), and the vector of those bounds is at most sqrt(2) |x||y| long), three squares, two
sums, a square root and a halving (together below 4 u relative): under (3 sqrt(2) + 3 + 4) u m_f < 12 u m_f; volume -- the cross
product as before (3 sqrt(2) u |b||c|), three products and two sums of the dot product (3 u) and the division (u): under
(3 sqrt(2) + 4) sqrt(2) u m_f < 12 u m_f.  Two sides: 2 x 16 u = the `16` of the factor in units of 2 u.
Everything else is compared for equality."""
import math

import numpy as np

import mesh_sdf_reference as M

INT_MIN = -2**31


# ---- labelling ------------------------------------------------------------------------------------------------------------------------
def label(faces, n_vertices):
    """-> dict(vertex_component int32 [V], face_component int32 [T], n, bad_faces, unused_vertices)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    good = ((faces >= 0) & (faces < n_vertices)).all(1) if len(faces) else np.zeros(0, bool)
    parent = list(range(n_vertices))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    used = np.zeros(n_vertices, bool)
    for a, b, c in faces[good].tolist():
        used[a] = used[b] = used[c] = True
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)              # the root is the smallest vertex of its set
    root = np.array([find(v) for v in range(n_vertices)], np.int64)
    is_root = used & (root == np.arange(n_vertices))
    number = np.cumsum(is_root) - 1                             # by increasing smallest vertex index
    vc = np.where(used, number[root] if n_vertices else 0, -1).astype(np.int32)
    fc = np.full(len(faces), -1, np.int32)
    if good.any():
        fc[good] = vc[faces[good, 0]]
    return {"vertex_component": vc, "face_component": fc, "n": int(is_root.sum()), "bad_faces": int((~good).sum()),
            "unused_vertices": int((~used).sum())}


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def _key(x):
    """float32 -> int32 that orders like the float, -0 below +0; its own inverse on the bits"""
    bits = np.ascontiguousarray(x, np.float32).view(np.int32)
    return bits ^ ((bits >> 31) & 0x7fffffff)


def face_terms(vertices, faces):
    """Per face, float64: (area term, volume term, m_area, m_volume)"""
    tri = np.asarray(vertices, np.float32)[np.asarray(faces, np.int64)].astype(np.float64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    volume = np.einsum("ij,ij->i", a, np.cross(b, c)) / 6.0
    n = lambda x: np.linalg.norm(x, axis=1)
    return area, volume, 0.5 * n(b - a) * n(c - a), n(a) * n(b) * n(c) / 6.0


def table(vertices, faces, lab):
    """-> dict of [C] arrays: the ComponentStats fields, plus area_bound and volume_bound (module docstring)"""
    vertices, faces = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    V, C, vc, fc = len(vertices), lab["n"], lab["vertex_component"], lab["face_component"]
    out = {"vertices": np.bincount(vc[vc >= 0], minlength=C).astype(np.int32),
           "faces": np.bincount(fc[fc >= 0], minlength=C).astype(np.int32)}
    f = faces[fc >= 0]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
    uses = {}
    for x, y in np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).tolist():
        e = (x, y) if x < y else (y, x)
        uses[e] = uses.get(e, 0) + 1
    comp = np.array([vc[e[0]] for e in uses], np.int64)
    n_uses = np.array(list(uses.values()), np.int64)
    out["edges"] = np.bincount(comp, minlength=C).astype(np.int32)
    out["boundary_edges"] = np.bincount(comp[n_uses == 1], minlength=C).astype(np.int32)
    out["nonmanifold_edges"] = np.bincount(comp[n_uses >= 3], minlength=C).astype(np.int32)
    out["euler"] = out["vertices"] - out["edges"] + out["faces"]
    good = np.flatnonzero(fc >= 0)
    t_area, t_vol, m_area, m_vol = face_terms(vertices, faces[good])
    order = np.argsort(fc[good], kind="stable")
    cuts = np.cumsum(out["faces"])[:-1] if C else []
    for name, t, m in (("area", t_area, m_area), ("volume", t_vol, m_vol)):
        out[name] = np.array([math.fsum(x) for x in np.split(t[order], cuts)] if C else [], np.float64)
        out[name + "_bound"] = np.array([(len(x) + 16) * 2.0**-52 * math.fsum(x) for x in np.split(m[order], cuts)] if C else [], np.float64)
    lo, hi = np.full((C, 3), 2**31 - 1, np.int64), np.full((C, 3), INT_MIN, np.int64)
    live = vc >= 0
    np.minimum.at(lo, vc[live], _key(vertices[live]).astype(np.int64))
    np.maximum.at(hi, vc[live], _key(vertices[live]).astype(np.int64))
    unkey = lambda k: (lambda b: b ^ ((b >> 31) & 0x7fffffff))(k.astype(np.int32)).view(np.float32)
    out["lo"], out["hi"] = unkey(lo), unkey(hi)
    return out


INT_FIELDS = ("vertices", "faces", "edges", "boundary_edges", "nonmanifold_edges", "euler")


# ---- selection ------------------------------------------------------------------------------------------------------------------------
def select(vertices, normals, faces, lab, keep):
    """-> dict(vertices, normals, faces, vertex_map, face_map)"""
    keep = np.asarray(keep, bool)
    vc, fc = lab["vertex_component"], lab["face_component"]
    kv = (vc >= 0) & keep[np.maximum(vc, 0)] if len(keep) else np.zeros(len(vc), bool)
    kf = (fc >= 0) & keep[np.maximum(fc, 0)] if len(keep) else np.zeros(len(fc), bool)
    vmap = np.where(kv, np.cumsum(kv) - 1, -1).astype(np.int32)
    fmap = np.where(kf, np.cumsum(kf) - 1, -1).astype(np.int32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return {"vertices": np.asarray(vertices, np.float32)[kv], "normals": None if normals is None else np.asarray(normals, np.float32)[kv],
            "faces": vmap[faces[kf]].astype(np.int32).reshape(-1, 3), "vertex_map": vmap, "face_map": fmap}


def rule(tab, keep_largest=None, min_faces=0, min_area_fraction=0.0, closed_only=False, by="area"):
    """clean_mesh's rule: the filters, then of the survivors the keep_largest greatest by `by`, ties to the lower number -> bool [C]"""
    C = len(tab["faces"])
    total = float(np.sum(tab["area"]))
    ok = [bool(tab["faces"][c] >= min_faces and (min_area_fraction <= 0.0 or tab["area"][c] >= min_area_fraction * total)
               and (not closed_only or tab["boundary_edges"][c] == 0)) for c in range(C)]
    if keep_largest is not None:
        size = {"area": tab["area"], "faces": tab["faces"], "volume": np.abs(tab["volume"])}[by]
        best = sorted([c for c in range(C) if ok[c]], key=lambda c: (-float(size[c]), c))[:keep_largest]
        ok = [c in best for c in range(C)]
    return np.array(ok, bool)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def join(*meshes):
    """Disjoint union: the vertices one after the other."""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32)); fs.append(np.asarray(f, np.int32) + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def disjoint_triangles(n, seed=0):
    return M.soup(n, seed) if n else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))


def renumber(v, f, perm):
    """Vertex i becomes vertex perm[i]."""
    perm = np.asarray(perm, np.int64)
    out = np.empty_like(v)
    out[perm] = v
    return out, perm[np.asarray(f, np.int64)].astype(np.int32)


def strip(n_faces, numbering="ascending", seed=0):
    """A strip of n_faces triangles (i, i + 1, i + 2) over n_faces + 2 vertices in a zigzag, alternately flipped to one orientation:
    the longest chain a mesh of this size can be.  numbering: ascending, descending or random (seeded)."""
    i = np.arange(n_faces + 2)
    v = np.stack([0.5 * i, (i % 2).astype(np.float64), np.zeros(len(i))], 1).astype(np.float32)
    k = np.arange(n_faces)
    f = np.stack([k, np.where(k % 2 == 0, k + 1, k + 2), np.where(k % 2 == 0, k + 2, k + 1)], 1).astype(np.int32)
    if numbering == "ascending":
        return v, f
    perm = i[::-1].copy() if numbering == "descending" else np.random.default_rng(seed).permutation(len(i))
    return renumber(v, f, perm)


def fan(n_faces, hub=0):
    """n_faces triangles around one hub vertex: (hub, r_k, r_(k+1)) on a circle, closed."""
    t = 2 * np.pi * np.arange(n_faces) / n_faces
    ring = np.stack([np.cos(t), np.sin(t), np.zeros(n_faces)], 1)
    v = np.concatenate([ring[:hub], [[0.0, 0.0, 0.3]], ring[hub:]]).astype(np.float32)
    idx = lambda k: np.where(k < hub, k, k + 1)
    k = np.arange(n_faces)
    return v, np.stack([np.full(n_faces, hub), idx(k), idx((k + 1) % n_faces)], 1).astype(np.int32)


def tetrahedron(centre=(0.0, 0.0, 0.0), size=1.0):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * size + np.asarray(centre)
    return v.astype(np.float32), np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)      # outward


def two_tetrahedra_apart():
    return join(tetrahedron((0, 0, 0), 0.1), tetrahedron((1, 0, 0), 0.2))


def two_tetrahedra_sharing_a_vertex():
    """The second tetrahedron's first vertex IS the first one's vertex 0: 7 vertices, one component, euler 3."""
    v1, f1 = tetrahedron((0, 0, 0), 0.1)
    v2, f2 = tetrahedron((0.2, 0.2, 0.2), 0.1)                  # its vertex 3 = (0.1, 0.1, 0.3); vertex 0 of v1 = (0.1, 0.1, 0.1)
    v2 = v2 + (v1[0] - v2[3])
    remap = np.array([4, 5, 6, 0])
    return np.concatenate([v1, v2[:3]]).astype(np.float32), np.concatenate([f1, remap[f2]]).astype(np.int32)


def three_faces_on_one_edge():
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [-0.5, 1, 0.5], [-0.5, -1, 0.5]], np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32)


def icospheres(k, subdivisions=1):
    """k disjoint icospheres of different radii along a line."""
    return join(*[M.icosphere(subdivisions, centre=(float(i), 0.25 * i, -0.5 * i), radius=0.2 + 0.03 * i) for i in range(k)])


def sphere_and_floaters(n_floaters=200):
    """One icosphere (320 faces) and n_floaters tiny tetrahedra around it."""
    rng = np.random.default_rng(7)
    centres = rng.uniform(-1.0, 2.0, (2 * n_floaters, 3))
    centres = centres[np.linalg.norm(centres - 0.5, axis=1) > 0.5][:n_floaters]
    parts = [tetrahedron(c, 0.004) for c in centres[:len(centres) // 2]] + [M.icosphere(2)] + [tetrahedron(c, 0.004) for c in centres[len(centres) // 2:]]
    return join(*parts), len(centres)


def three_rankings():
    """Three pieces that area, faces and |volume| rank differently: a coarse big sphere (the volume), a fine small sphere (the faces),
    a large open quad (the area) in a plane through the origin (the cones from the origin to its faces have no volume)."""
    quad_v = np.array([[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0]], np.float32)
    return join(M.icosphere(1, radius=0.6), M.icosphere(3, centre=(2.0, 0.0, 0.0), radius=0.1), (quad_v, M.open_quad()[1]))


SPHERES = [((0.22, 0.2, 0.2), 0.12), ((0.8, 0.2, 0.25), 0.1), ((0.2, 0.8, 0.3), 0.14), ((0.78, 0.78, 0.7), 0.11), ((0.5, 0.5, 0.55), 0.13)]
CUT_SPHERE = ((0.5, 0.15, 0.0), 0.1)                            # centred on the grid's z = 0 face: extracted open


def spheres_field(resolution=32, cut=False):
    """min over the sphere SDFs on (resolution + 1)^3 points of the unit box, float32: what marching tetrahedra extracts with iso 0,
    sign -1, lo 0, h 1 / resolution"""
    a = np.linspace(0.0, 1.0, resolution + 1)
    x = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1)
    d = [np.linalg.norm(x - np.asarray(c), axis=-1) - r for c, r in SPHERES + ([CUT_SPHERE] if cut else [])]
    return np.min(d, 0).astype(np.float32)


NAMED = {"cube": M.cube, "icosphere": M.icosphere, "needle": M.needle_tetrahedron, "open_quad": M.open_quad,
         "soup500": lambda: M.soup(500, 11), "two_apart": two_tetrahedra_apart, "two_sharing": two_tetrahedra_sharing_a_vertex,
         "three_on_edge": three_faces_on_one_edge, "icospheres4": lambda: icospheres(4), "torus": M.extracted_torus,
         "three_rankings": three_rankings}
_CACHE = {}


def case(name):
    """(vertices, faces, label, table) of a named mesh, computed once; callers must not modify them."""
    if name not in _CACHE:
        v, f = NAMED[name]()
        lab = label(f, len(v))
        _CACHE[name] = (v, f, lab, table(v, f, lab))
    return _CACHE[name]
