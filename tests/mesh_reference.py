"""Independent numpy statement of the marching-tetrahedra contract ("Isosurface extraction").

Not a test module: the CPU tier pins it (test_mesh_reference.py) and the GPU tier compares the kernels of csrc/mesh.hip with it
(test_gpu_mesh.py).  Vectorised over points and cells; float64 by default, `dtype=np.float32` repeats the kernel's arithmetic operation
by operation (numpy rounds every elementwise f32 operation on its own, so the vectorised form is the serial one).

The winding of every triangle is decided GEOMETRICALLY on the unit lattice -- edge midpoints, the sign of (q1 - q0) x (q2 - q0) against
the vector from the centroid of the inside corners to the centroid of the outside corners -- which is exact in floating point (all
coordinates are multiples of 1/6 well inside the mantissa after scaling) and shares nothing with the kernel's case table."""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))          # lexicographic: (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y), (z,y,x)
_BIT = (4, 2, 1)                                        # offset code of a unit step along x, y, z: d = 4 dx + 2 dy + dz


def _offs(perm):
    return (0, _BIT[perm[0]], _BIT[perm[0]] | _BIT[perm[1]], 7)


def _code_xyz(code):
    return np.array([(code >> 2) & 1, (code >> 1) & 1, code & 1], dtype=np.int64)


def _tri_rule(case):
    """Triangles of a tetrahedron whose inside bits are `case` (bit n = local corner n), as lists of three corner pairs, in the
    contract's listed order (before the winding fix)."""
    ins = [n for n in range(4) if case >> n & 1]
    out = [n for n in range(4) if not case >> n & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1 or len(out) == 1:
        a = ins[0] if len(ins) == 1 else out[0]
        o = [n for n in range(4) if n != a]
        return [[(a, o[0]), (a, o[1]), (a, o[2])]]
    A, B = ins
    C, D = out
    return [[(A, C), (A, D), (B, D)], [(A, C), (B, D), (B, C)]]


def _wind(tri, offs, case):
    """Counter-clockwise seen from the outside: decided on the edge midpoints of the unit cell (exact: sixths of small integers)."""
    corners = [_code_xyz(o).astype(np.float64) for o in offs]
    q = [(corners[a] + corners[b]) / 2 for a, b in tri]
    n = np.cross(q[1] - q[0], q[2] - q[0])
    ins = [corners[k] for k in range(4) if case >> k & 1]
    out = [corners[k] for k in range(4) if not case >> k & 1]
    s = float(np.dot(n, np.mean(out, 0) - np.mean(ins, 0)))
    assert s != 0.0
    return tri if s > 0 else [tri[0], tri[2], tri[1]]


def inside_mask(values, iso, sign):
    v = np.asarray(values, dtype=np.float32)
    iso = np.float32(iso)
    with np.errstate(invalid="ignore"):
        return (v > iso) if sign > 0 else (v < iso)


def gradient(values, h, dtype=np.float64):
    """Central differences, one-sided on the boundary faces: [Nx, Ny, Nz, 3]."""
    v = np.asarray(values, dtype=np.float32).astype(dtype)
    g = np.empty(v.shape + (3,), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            vk = np.moveaxis(v, k, 0)
            gk = np.empty_like(vk)
            hk = dtype(h[k])
            gk[1:-1] = (vk[2:] - vk[:-2]) / (dtype(2) * hk)
            gk[0] = (vk[1] - vk[0]) / hk
            gk[-1] = (vk[-1] - vk[-2]) / hk
            g[..., k] = np.moveaxis(gk, 0, k)
    return g


def marching_tetrahedra(values, iso, sign=1, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0), normals=False, dtype=np.float64):
    """-> dict(vertices [V,3] dtype, faces [T,3] int32, and with normals=True: normals [V,3] (unit, or 0 where the gradient is zero or
    not finite) and grad [V,3], the interpolated gradient times -sign before normalisation)."""
    v32 = np.ascontiguousarray(values, dtype=np.float32)
    nx, ny, nz = v32.shape
    assert min(nx, ny, nz) >= 2 and sign in (1, -1)
    n = nx * ny * nz
    ins = inside_mask(v32, iso, sign)
    ins_flat = ins.ravel()
    vflat = v32.ravel().astype(dtype)
    lin = np.arange(n, dtype=np.int64).reshape(nx, ny, nz)
    off_lin = [int(((c >> 2) & 1) * ny * nz + ((c >> 1) & 1) * nz + (c & 1)) for c in range(8)]

    # ---- vertices: edge type e of owner p <-> slot p * 7 + e - 1; ids ascend in (owner, e)
    has = np.zeros((n, 7), dtype=bool)
    for e in range(1, 8):
        dx, dy, dz = (e >> 2) & 1, (e >> 1) & 1, e & 1
        a = ins[:nx - dx, :ny - dy, :nz - dz]
        b = ins[dx:, dy:, dz:]
        has[lin[:nx - dx, :ny - dy, :nz - dz][a != b], e - 1] = True
    slots = np.flatnonzero(has.ravel())
    vid = np.full(n * 7, -1, dtype=np.int64)
    vid[slots] = np.arange(slots.size)
    owner, e = slots // 7, slots % 7 + 1
    d = np.stack([(e >> 2) & 1, (e >> 1) & 1, e & 1], 1)
    ijk = np.stack([owner // (ny * nz), owner // nz % ny, owner % nz], 1)
    other = owner + d[:, 0] * ny * nz + d[:, 1] * nz + d[:, 2]
    iso_t = dtype(np.float32(iso))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (iso_t - vflat[owner]) / (vflat[other] - vflat[owner])
        t = np.where((t >= 0) & (t <= 1), t, dtype(0.5)).astype(dtype)
    lo_t, h_t = np.asarray(lo, dtype=np.float32).astype(dtype), np.asarray(h, dtype=np.float32).astype(dtype)
    verts = lo_t[None, :] + (ijk.astype(dtype) + t[:, None] * d.astype(dtype)) * h_t[None, :]
    out = {"vertices": verts.astype(dtype), "t": t}
    if normals:
        g = gradient(v32, np.asarray(h, dtype=np.float32), dtype).reshape(n, 3)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            gi = (g[owner] + t[:, None] * (g[other] - g[owner])) * dtype(-sign)
            ln = np.sqrt((gi * gi).sum(1))
            nn = gi / ln[:, None]
        bad = ~(np.isfinite(nn).all(1) & (ln > 0))
        nn[bad] = 0
        out["grad"], out["normals"] = gi, nn.astype(dtype)

    # ---- faces: cell order, then the six tetrahedra, then the listed order
    cell = lin[:nx - 1, :ny - 1, :nz - 1].ravel()
    keys, tris = [], []
    for ti, perm in enumerate(PERMS):
        offs = _offs(perm)
        m = sum(ins_flat[cell + off_lin[o]].astype(np.int64) << k for k, o in enumerate(offs))
        for case in range(1, 15):
            sel = cell[m == case]
            if not sel.size:
                continue
            for r, tri in enumerate(_tri_rule(case)):
                ids = []
                for a, b in _wind(tri, offs, case):
                    p, q = min(a, b), max(a, b)                       # the edge's owner is its lower corner: offs[p] is a subset of offs[q]
                    ids.append(vid[(sel + off_lin[offs[p]]) * 7 + (offs[q] ^ offs[p]) - 1])
                keys.append((sel * 6 + ti) * 2 + r)
                tris.append(np.stack(ids, 1))
    if keys:
        keys, tris = np.concatenate(keys), np.concatenate(tris)
        faces = tris[np.argsort(keys, kind="stable")]
    else:
        faces = np.zeros((0, 3), dtype=np.int64)
    assert (faces >= 0).all()
    out["faces"] = faces.astype(np.int32)
    return out


# ---- mesh invariants -------------------------------------------------------------------------------------------------------------
def edge_topology(faces):
    """Directed and undirected edge counts of a triangle list: dict(directed {(a, b): count}, undirected {(min, max): count},
    boundary = sorted undirected edges used once, closed = every undirected edge in exactly two faces, once in each direction)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    de, dc = np.unique(e, axis=0, return_counts=True) if len(e) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    ue, uc = np.unique(np.sort(e, 1), axis=0, return_counts=True) if len(e) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    return {"directed": {tuple(k): int(c) for k, c in zip(de.tolist(), dc)},
            "undirected": {tuple(k): int(c) for k, c in zip(ue.tolist(), uc)},
            "n_edges": int(len(ue)),
            "boundary": [tuple(k) for k in ue[uc == 1].tolist()],
            "closed": bool(len(ue) > 0 and (uc == 2).all() and (dc == 1).all())}


def euler(n_vertices, faces):
    return int(n_vertices) - edge_topology(faces)["n_edges"] + int(np.asarray(faces).reshape(-1, 3).shape[0])


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---- the fields the tests share ----------------------------------------------------------------------------------------------------
def unit_grid(n):
    """Points of an n^3 grid over [0, 1]^3 as [n, n, n, 3] float64 and its spacing."""
    a = np.linspace(0.0, 1.0, n)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1), 1.0 / (n - 1)


def sphere_sdf(pts, centre=(0.5, 0.47, 0.52), r=0.3):
    return (np.linalg.norm(pts - np.asarray(centre), axis=-1) - r).astype(np.float32)


def torus_sdf(pts, centre=(0.5, 0.47, 0.52), R=0.3, r=0.12):
    p = pts - np.asarray(centre)
    return (np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R) ** 2 + p[..., 2] ** 2) - r).astype(np.float32)


def padded_random(seed=0, shape=(7, 6, 5)):
    """A normal field padded with -1 on every side: with sign +1 the surface cannot reach the grid boundary."""
    f = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return np.pad(f, 1, constant_values=-1.0)


def nonfinite_field():
    f = padded_random()
    f[3, 3, 3], f[4, 2, 3], f[2, 4, 2], f[5, 3, 4] = np.nan, np.inf, -np.inf, 0.0      # the last equals iso = 0
    return f
