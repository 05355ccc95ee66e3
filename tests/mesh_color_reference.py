"""numpy reference of the vertex-colour contract (include/ngp_hip.h, "vertex colours from posed images"; csrc/mesh_color.hip), independent
of the package, in two arithmetics that run the same code.

  np.float64   the contract: the f32 inputs (cos_min, near and eps included: the kernel receives them as f32) taken to float64
  np.float32   the kernel's projection restated operation for operation (numpy's float32 operations are IEEE binary32, one rounding
               each, dots as (x + y) + z), its occlusion the float32 brute force of tests/mesh_raycast_reference.py over ALL faces

Behind the projection both run the kernel's f64 sums in the kernel's order: the bilinear mean as two rows and the mean between them, the
cameras in ascending index, w rgb and w added one rounded operation each, one division, one rounding to f32 (float64 keeps its f64).

DECIDED.  A (vertex, camera) pair makes four choices: cos > cos_min, p.z > near, the sample inside the frame, the segment free.  It is
decided when float64 and float32 make the same four (the fourth where both accept the pair).  A vertex is decided when all its pairs
are; mode "best" picks a winner, a fifth choice, and a vertex is then decided only if both arithmetics pick the same camera.
MAX_UNDECIDED is a condition on the named sets, asserted for the reference alone in tests/test_mesh_color_reference.py.

E32_c = max |colors32 - colors64| over the decided vertices with a view, at least one float32 ulp of the largest |colour| of the set (the
device rounds its result to f32 once, whatever else it does); E32_w the same for the weight.  Bounds: B = 4 x E32, per set, no constant.

judge() asserts on decided vertices: views exact, filled (0 or 255 before any fill) exact, colours and weight within B of float64."""
import numpy as np

import mesh_raycast_reference as RR
import mesh_sdf_reference as M

MAX_UNDECIDED = 0.02
UNCOLOURED = 255
F32, F64 = np.float32, np.float64


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ---- cameras, meshes, images --------------------------------------------------------------------------------------------------------------
def look_at(position, target=(0.5, 0.5, 0.5)):
    """c2w f32 [3,4] = (right, down, front | position) of a camera at `position` looking at `target`, z up (y up where it looks along z)."""
    p, t = np.asarray(position, F64), np.asarray(target, F64)
    front = (t - p) / np.linalg.norm(t - p)
    up = np.array([0.0, 0.0, 1.0]) if abs(front[2]) < 0.99 else np.array([0.0, 1.0, 0.0])
    right = np.cross(front, up)
    right /= np.linalg.norm(right)
    down = np.cross(front, right)
    return np.concatenate([np.stack([right, down, front], 1), p[:, None]], 1).astype(F32)


def intrinsics(width, height, focal):
    return np.array([[focal, 0, width / 2], [0, focal, height / 2], [0, 0, 1]], F32)


def pixel_rays(K, c2w, width, height):
    """The rays of get_ray_directions / get_rays in float64: origins [H,W,3], directions [H,W,3] (not normalised) through the pixel centres."""
    K, c2w = np.asarray(K, F64), np.asarray(c2w, F64)
    y, x = np.meshgrid(np.arange(height, dtype=F64), np.arange(width, dtype=F64), indexing="ij")
    d = np.stack([(x - K[0, 2] + 0.5) / K[0, 0], (y - K[1, 2] + 0.5) / K[1, 1], np.ones_like(x)], -1)
    return np.broadcast_to(c2w[:, 3], d.shape), d @ c2w[:, :3].T


def grid_square(z, lo=0.2, hi=0.8, n=3):
    """n x n vertices on the plane of height z, 2 (n - 1)^2 faces counter-clockwise seen from +z -> (v f32, f int32, normals f32)."""
    s = np.linspace(lo, hi, n)
    v = np.array([[x, y, z] for y in s for x in s], F32)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            f += [(a, a + 1, a + n + 1), (a, a + n + 1, a + n)]
    return v, np.array(f, np.int32), np.tile(np.array([[0, 0, 1]], F32), (len(v), 1))


def sphere_normals(v, centre=(0.5, 0.5, 0.5)):
    n = np.asarray(v, F64) - np.asarray(centre)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)


def smooth_images(n, height, width, channels=3):
    """A smooth function of the pixel position, different in every view and channel, inside (0.05, 0.95)."""
    j, y, x, c = np.meshgrid(np.arange(n), np.arange(height), np.arange(width), np.arange(channels), indexing="ij")
    return (0.5 + 0.45 * np.sin(0.37 * x * (c + 1) / 2 + 0.23 * y + 1.3 * j + c)).astype(F32)


def default_eps(vertices):
    """bake_image_colors' default: 1e-3 x the diagonal of the box of the finite vertices, f64 squares and sum, one rounding to f32."""
    v = np.asarray(vertices, F32)
    v = v[np.isfinite(v).all(1)].astype(F64)
    d = v.max(0) - v.min(0)
    return F32(1e-3 * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


# ---- the contract --------------------------------------------------------------------------------------------------------------------------
def project(vertices, normals, K, c2w, wh, eps, cos_min=0.1, near=1e-6, two_sided=False, T=F64):
    """Every (camera, vertex) pair in the arithmetic T -> dict of [N,V] arrays: cos, a, b (the sample position), weight, the three
    choices cos_ok, depth_ok, frame_ok, accept; o, d [N,V,3]: the occlusion segment (0 where rejected)."""
    v, n = np.asarray(vertices, F32).astype(T)[None], np.asarray(normals, F32).astype(T)[None]
    c2w = np.asarray(c2w, F32).astype(T)
    K = np.broadcast_to(np.asarray(K, F32).astype(T), (len(c2w), 3, 3))
    right, down, front, c = (c2w[:, None, :, k] for k in range(4))
    fx, fy, cx, cy = (K[:, i, j][:, None] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    eps, cos_min, near = T(F32(eps)), T(F32(cos_min)), T(F32(near))
    w_max, h_max = T(wh[0] - 1), T(wh[1] - 1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        finite = np.isfinite(v).all(-1) & np.isfinite(n).all(-1)
        d = c - v
        nd = dot(n, d)
        flip = bool(two_sided) & (nd < 0)
        n = np.where(flip[..., None], -n, n)
        nd = np.where(flip, -nd, nd)
        cos = nd / np.sqrt(dot(d, d))
        q = v - c
        px, py, pz = dot(right, q), dot(down, q), dot(front, q)
        a, b = (fx * px / pz + cx) - T(0.5), (fy * py / pz + cy) - T(0.5)
        cos_ok = finite & (cos > cos_min)
        depth_ok = finite & (pz > near)
        frame_ok = finite & (a >= 0) & (a <= w_max) & (b >= 0) & (b <= h_max)
        accept = cos_ok & depth_ok & frame_ok
        o = v + n * eps
        dd = c - o
    z = lambda x: np.where(accept, x, T(0))
    return dict(cos=z(cos), a=z(a), b=z(b), weight=z(cos * cos), cos_ok=cos_ok, depth_ok=depth_ok, frame_ok=frame_ok, accept=accept,
                o=np.where(accept[..., None], o, T(0)), d=np.where(accept[..., None], dd, T(0)))


def occluded(p, vertices, faces, T):
    """[N,V] bool: some face is met on the segment of an accepted pair, t in [0, 1] -- the brute force over all faces in T, on the
    segment rounded to f32 (the form in which a ray cast receives it)."""
    out = np.zeros(p["accept"].shape, bool)
    if len(faces) and p["accept"].any():
        hit = RR.brute_force(p["o"][p["accept"]], p["d"][p["accept"]], vertices, faces, T, t_min=0.0, t_max=1.0)
        out[p["accept"]] = hit["count"] > 0
    return out


def texels(a, b, width, height, T):
    """The kernel's four texel indices and the two fractions (f64) of sample positions a, b in T."""
    x0 = np.clip(np.floor(a), 0, width - 1).astype(np.int64)
    y0 = np.clip(np.floor(b), 0, height - 1).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, width - 1), np.minimum(y0 + 1, height - 1)
    return x0, y0, x1, y1, (a - x0.astype(T)).astype(F64), (b - y0.astype(T)).astype(F64)


def accumulate(images, p, counts, mode, T):
    """The accumulate and finish launches on the pairs that count -> dict(colors [V,3], weight [V] (T; float64 unrounded), views [V],
    filled [V]: 0 or 255, winner [V]: the camera mode "best" kept, -1)."""
    img = np.asarray(images, F32).astype(F64)
    n, height, width = img.shape[:3]
    n_v = counts.shape[1]
    acc, views, best, winner = np.zeros((n_v, 4)), np.zeros(n_v, np.int32), np.zeros(n_v, T), np.full(n_v, -1)
    for j in range(n):                                                           # ascending camera index
        m = counts[j] & (p["weight"][j] > 0)
        if mode == "best":
            m = m & (p["cos"][j] > best)
        if not m.any():
            continue
        x0, y0, x1, y1, fx, fy = (x[m] for x in texels(p["a"][j], p["b"][j], width, height, T))
        fx, fy = fx[:, None], fy[:, None]
        top = (1.0 - fx) * img[j, y0, x0, :3] + fx * img[j, y0, x1, :3]
        bottom = (1.0 - fx) * img[j, y1, x0, :3] + fx * img[j, y1, x1, :3]
        rgb = (1.0 - fy) * top + fy * bottom
        dw = p["weight"][j][m].astype(F64)
        if mode == "best":
            acc[m, :3], acc[m, 3], views[m], best[m], winner[m] = dw[:, None] * rgb, dw, 1, p["cos"][j][m], j
        else:
            acc[m, :3] += dw[:, None] * rgb
            acc[m, 3] += dw
            views[m] += 1
    seen = views > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        colors = np.where(seen[:, None], acc[:, :3] / acc[:, 3:], 0.0)
    weight = np.where(seen, acc[:, 3], 0.0)
    if T is F32:
        colors, weight = colors.astype(F32), weight.astype(F32)
    return dict(colors=colors, weight=weight, views=views, filled=np.where(seen, 0, UNCOLOURED).astype(np.uint8), winner=winner)


def bake(vertices, faces, normals, images, K, c2w, eps, cos_min=0.1, near=1e-6, two_sided=False, mode="blend", T=F64):
    """The whole contract before the fill, in T -> accumulate()'s dict + project = the pairs, counts [N,V]."""
    images = np.asarray(images, F32)
    p = project(vertices, normals, K, c2w, (images.shape[2], images.shape[1]), eps, cos_min, near, two_sided, T)
    occ = occluded(p, np.asarray(vertices, F32), np.asarray(faces, np.int64).reshape(-1, 3), T)
    counts = p["accept"] & ~occ
    return dict(accumulate(images, p, counts, mode, T), project=p, occluded=occ, counts=counts)


def neighbours(faces, n_vertices):
    """The rows of the adjacency: per vertex its distinct neighbours over the good faces (indices in range, no repeated index), ascending."""
    rows = [set() for _ in range(n_vertices)]
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        if min(a, b, c) < 0 or max(a, b, c) >= n_vertices or a == b or b == c or c == a:
            continue
        rows[a] |= {b, c}; rows[b] |= {a, c}; rows[c] |= {a, b}
    return [sorted(r) for r in rows]


def fill(colors, filled, faces, rounds, default=(0.5, 0.5, 0.5)):
    """`rounds` Jacobi rounds, serially: colors f32 [V,3] and filled uint8 [V] (0 / 255) -> (colors, filled) after them; what is still 255
    gets the default colour."""
    colors, filled = np.array(colors, F32), np.array(filled, np.uint8)
    rows = neighbours(faces, len(filled))
    for r in range(1, rounds + 1):
        before = filled.copy()
        for v in np.flatnonzero(before == UNCOLOURED):
            s, count = [0.0, 0.0, 0.0], 0
            for j in rows[v]:                                                    # ascending
                if before[j] == UNCOLOURED:
                    continue
                for k in range(3):
                    s[k] += float(colors[j, k])
                count += 1
            if count:
                colors[v] = [F32(s[k] / count) for k in range(3)]
                filled[v] = r
    colors[filled == UNCOLOURED] = np.asarray(default, F32)
    return colors, filled


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
class Case:
    """A mesh, its normals, an image set and the options, with both references computed once."""

    def __init__(self, name, vertices, faces, normals, images, K, c2w, eps=None, **options):
        self.name = name
        self.vertices, self.faces = np.ascontiguousarray(vertices, F32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        self.normals, self.images = np.ascontiguousarray(normals, F32).reshape(-1, 3), np.ascontiguousarray(images, F32)
        self.K, self.c2w = np.ascontiguousarray(K, F32), np.ascontiguousarray(c2w, F32)
        self.eps = float(default_eps(self.vertices) if eps is None else F32(eps))
        self.options = options                                                   # cos_min, near, two_sided, mode
        self._ref = None

    def ref(self):
        if self._ref is None:
            args = (self.vertices, self.faces, self.normals, self.images, self.K, self.c2w, self.eps)
            r32, r64 = bake(*args, T=F32, **self.options), bake(*args, T=F64, **self.options)
            p32, p64 = r32["project"], r64["project"]
            pairs = np.ones(p32["accept"].shape, bool)
            for k in ("cos_ok", "depth_ok", "frame_ok"):
                pairs &= p32[k] == p64[k]
            both = p32["accept"] & p64["accept"]
            pairs &= ~both | (r32["occluded"] == r64["occluded"])
            decided = pairs.all(0) if pairs.shape[0] else np.ones(pairs.shape[1], bool)
            if self.options.get("mode") == "best":
                decided &= r32["winner"] == r64["winner"]
            seen = decided & (r64["views"] > 0)

            def e32(key):
                scale = float(np.abs(r64[key]).max()) if r64[key].size else 0.0
                err = float(np.abs(r32[key].astype(F64) - r64[key])[seen].max()) if seen.any() else 0.0
                return max(err, float(M.ulp32(max(scale, float(np.finfo(F32).tiny)))))
            self._ref = dict(r32=r32, r64=r64, decided_pairs=pairs, decided=decided, e32_c=e32("colors"), e32_w=e32("weight"))
        return self._ref

    def undecided_fraction(self):
        pairs = self.ref()["decided_pairs"]
        return 1.0 - float(pairs.mean()) if pairs.size else 0.0


def judge(case, colors, weight, views, filled):
    """The standard assertion on a bake WITHOUT fill rounds (numpy arrays); default-coloured vertices are judged by `filled` alone.
    Returns the figures it printed."""
    R = case.ref()
    r64, dec = R["r64"], R["decided"]
    colors, weight = np.asarray(colors, F64), np.asarray(weight, F64)
    views, filled = np.asarray(views, np.int64), np.asarray(filled, np.int64)
    n_v = len(case.vertices)
    assert colors.shape == (n_v, 3) and weight.shape == (n_v,) and views.shape == (n_v,) and filled.shape == (n_v,), case.name
    assert np.isfinite(colors).all() and np.isfinite(weight).all() and (views >= 0).all(), case.name
    assert ((filled == 0) == (views > 0)).all() and np.isin(filled, (0, UNCOLOURED)).all() and (weight[views == 0] == 0).all(), case.name
    wrong = int((views != r64["views"])[dec].sum())
    seen = dec & (r64["views"] > 0)
    err_c = float(np.abs(colors - r64["colors"])[seen].max()) if seen.any() else 0.0
    err_w = float(np.abs(weight - r64["weight"])[seen].max()) if seen.any() else 0.0
    had = views > 0                                                              # elsewhere the colour is the caller's default
    bits = int((np.asarray(colors, F32).view(np.uint32) != R["r32"]["colors"].view(np.uint32)).any(1)[had].sum()) if n_v else 0
    print("%s: V %d, %d pairs, %d undecided pairs (%.2f %%), %d undecided vertices, %d decided vertices with the wrong views; colour err %.3g "
          "(%.2f x E32, bound %.3g), weight err %.3g (%.2f x E32, bound %.3g); %d coloured vertices differ in bits from the float32 restatement"
          % (case.name, n_v, R["decided_pairs"].size, int((~R["decided_pairs"]).sum()), 100 * case.undecided_fraction(), int((~dec).sum()),
             wrong, err_c, err_c / R["e32_c"], 4 * R["e32_c"], err_w, err_w / R["e32_w"], 4 * R["e32_w"], bits))
    assert wrong == 0, (case.name, wrong)
    assert err_c <= 4 * R["e32_c"], (case.name, err_c, R["e32_c"])
    assert err_w <= 4 * R["e32_w"], (case.name, err_w, R["e32_w"])
    return dict(err_c=err_c, err_w=err_w, bits=bits)


# ---- the named sets ------------------------------------------------------------------------------------------------------------------------
CENTRE = np.array([0.5, 0.5, 0.5])
AROUND = np.array([(1, .2, .3), (-1, .3, -.2), (.2, 1, .1), (-.3, -1, .2), (.1, .3, 1), (.2, -.1, -1), (.7, -.6, .4)], F64)
ABOVE = np.array([(.3, .1, 1), (-.4, .3, .8), (.1, -.5, .9)], F64)
WH = (32, 32)


def cameras(directions, distance=2.0, target=CENTRE):
    d = np.asarray(directions, F64)
    return np.stack([look_at(target + distance * x / np.linalg.norm(x), target) for x in d])


def submesh(v, f, n_vertices):
    """The first n_vertices vertices and the faces among them."""
    f = np.asarray(f).reshape(-1, 3)
    return v[:n_vertices], f[(f < n_vertices).all(1)] if len(f) else f


def linear_colour(x):
    """The closed loop's true function: affine in the position, inside (0, 1) on the unit box."""
    A = np.array([[0.5, 0.2, -0.1], [-0.2, 0.6, 0.1], [0.1, -0.3, 0.5]])
    return np.asarray(x, F64) @ A.T + np.array([0.2, 0.25, 0.3]), A


def closed_loop_images(v, f, K, c2w, wh, background=0.0):
    """Images of the mesh coloured by linear_colour: the float64 brute-force ray cast per pixel, the function at the hit, `background` on
    a miss -> (images f32 [N,H,W,3], hit masks [N,H,W])."""
    images, masks = [], []
    for pose in c2w:
        o, d = pixel_rays(K, pose, *wh)
        hit = RR.brute_force(o.reshape(-1, 3).astype(F32), d.reshape(-1, 3).astype(F32), v, f, F64)
        x = o.reshape(-1, 3).astype(F32).astype(F64) + np.where(hit["face"] >= 0, hit["t"], 0.0)[:, None] * d.reshape(-1, 3).astype(F32).astype(F64)
        rgb = np.where((hit["face"] >= 0)[:, None], linear_colour(x)[0], background)
        images.append(rgb.reshape(wh[1], wh[0], 3))
        masks.append((hit["face"] >= 0).reshape(wh[1], wh[0]))
    return np.stack(images).astype(F32), np.stack(masks)


def _build(name):
    v, f = M.icosphere(2)                                                        # 162 vertices, 320 faces
    n = sphere_normals(v)
    K = intrinsics(*WH, 70.0)
    if name in ("convex", "best"):
        c2w = cameras(AROUND[:6])
        return Case(name, v, f, n, smooth_images(6, WH[1], WH[0]), K, c2w, mode="best" if name == "best" else "blend")
    if name == "per_camera_K":                                                   # a K per camera, four channels
        c2w = cameras(AROUND[:6])
        Ks = np.stack([intrinsics(*WH, 60.0 + 4 * j) + np.array([[0, 0, 0.3 * j], [0, 0, -0.2 * j], [0, 0, 0]], F32) for j in range(6)])
        return Case(name, v, f, n, smooth_images(6, WH[1], WH[0], 4), Ks, c2w)
    if name == "seven":                                                          # the chunking case
        return Case(name, v, f, n, smooth_images(7, WH[1], WH[0]), K, cameras(AROUND))
    if name == "one_camera":
        return Case(name, v, f, n, smooth_images(1, WH[1], WH[0]), K, cameras(AROUND[:1]))
    if name in ("flipped", "flipped_one_sided"):                                 # inward normals: two_sided turns them, one-sided sees nothing
        return Case(name, v, f, -n, smooth_images(6, WH[1], WH[0]), K, cameras(AROUND[:6]), two_sided=name == "flipped")
    if name in ("v1", "v65"):
        sv, sf = submesh(v, f, int(name[1:]))
        return Case(name, sv, sf, n[:len(sv)], smooth_images(6, WH[1], WH[0]), K, cameras(AROUND[:6]), eps=default_eps(v))
    if name == "cap":                                                            # every camera above: the lower cap is seen by none
        return Case(name, v, f, n, smooth_images(3, WH[1], WH[0]), K, cameras(ABOVE))
    if name == "occluder":
        # two parallel squares facing +z; camera A straight above looks at the far (lower) one past the near one, whose extent
        # [0.45, 0.95]^2 covers the four far vertices with x, y in {0.5, 0.8} (a far vertex (x, y) is seen through (0.5 + 0.864 (x - 0.5),
        # ...) of the near plane); camera B stands at the side, its segments pass the near plane at x >= 1.25, and sees them all
        v0, f0, n0 = grid_square(0.3, 0.2, 0.8)
        v1, f1, n1 = grid_square(0.6, 0.45, 0.95)
        vv, ff, nn = np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)]), np.concatenate([n0, n1])
        c2w = np.stack([look_at((0.5, 0.5, 2.5), (0.5, 0.5, 0.3)), look_at((2.3, 0.5, 0.9), (0.5, 0.5, 0.3))])
        return Case(name, vv, ff, nn, smooth_images(2, WH[1], WH[0]), intrinsics(*WH, 60.0), c2w, eps=1e-3)
    if name == "tie":
        # one square facing +z, two cameras mirrored in the plane x = 0.5: for the vertices of the middle column d differs in the sign
        # of x alone, so cos has the same bits in both views and "best" must keep camera 0
        vv, ff, nn = grid_square(0.5, 0.25, 0.75)
        c2w = np.stack([look_at((0.5 - 0.75, 0.5, 2.0), (0.5, 0.5, 0.5)), look_at((0.5 + 0.75, 0.5, 2.0), (0.5, 0.5, 0.5))])
        return Case(name, vv, ff, nn, smooth_images(2, WH[1], WH[0]), intrinsics(*WH, 60.0), c2w, eps=1e-3, mode="best")
    if name == "closed_loop":
        c2w = cameras(AROUND[:6])
        images, _ = closed_loop_images(v, f, K, c2w, WH)
        return Case(name, v, f, n, images, K, c2w, cos_min=0.7)
    raise KeyError(name)


SETS = ("convex", "best", "per_camera_K", "seven", "one_camera", "flipped", "flipped_one_sided", "v1", "v65", "cap", "occluder", "tie",
        "closed_loop")
_CASES = {}


def case(name):
    """The named case, built (and its references computed) once per process."""
    if name not in _CASES:
        _CASES[name] = _build(name)
    return _CASES[name]
