"""Signed distance to a triangle mesh: the ground truth for everything here that produces or consumes a signed-distance field.

    target = MeshSDF.from_mesh(read_ply("scene.ply"))                 # builds the box hierarchy on the device (csrc/mesh_sdf.hip)
    d = target(points)                                                 # MeshDistance(sdf, closest, face, feature), one launch
    x = target.sample(2**16, sigma=0.01, uniform_fraction=0.25, generator=g)     # training points: near the surface + in the box
    surface_distance(mesh_a, mesh_b, 2**16)                            # how far two surfaces are apart, both ways
    hit = target.raycast(rays_o, rays_d)                               # MeshRayHit(t, face, bary, side): the first face along each ray
    target.visible(a, b)                                               # bool [n]: nothing of the mesh between a and b
    w = target.winding(points)                                         # [n]: the generalized winding number, 1 inside, 0 outside
    target.inside(points)                                              # bool [n]: w >= 0.5
    MeshSDF.from_mesh(scan, sign="winding")                            # the sign of the distance from the winding number
    render_mesh(target, K, c2w, (W, H))                                # depth, normal, mask and face images from a camera

The sign follows the angle-weighted pseudonormal of the nearest feature (Baerentzen & Aanaes 2005), which is exact for a closed,
consistently oriented 2-manifold whatever the dihedral angles.  On an open mesh it is the side of the nearest feature, and on a
self-intersecting mesh, overlapping closed shells or an unwelded soup it is wrong without a warning wherever the nearest face belongs to
a part that lies inside another.  For those, sign="winding" takes the sign from the generalized winding number of the whole mesh
(csrc/mesh_winding.hip: negative where w >= 0.5), which degrades gracefully with holes and counts overlapping shells as their union.
The contract is DESIGN.md section 3, "Distance to a triangle mesh" and "Winding number of a triangle mesh"."""
from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .mesh import Mesh


class _MeshDistance(NamedTuple):
    sdf: torch.Tensor            # [n] f32: sign * distance (unsigned mode: the distance)
    closest: torch.Tensor        # [n,3] f32: the nearest point of the mesh
    face: torch.Tensor           # [n] int32: a nearest face, a row of the faces MeshSDF was given
    feature: torch.Tensor        # [n] int32: 0 interior, 1 / 2 / 3 edge ab / bc / ca, 4 / 5 / 6 vertex a / b / c of that face


class MeshDistance(_MeshDistance):
    """What MeshSDF.__call__ returns; unpacks as (sdf, closest, face, feature).  All detached: the query has no gradients."""

    def __new__(cls, sdf, closest, face, feature, points=None):
        self = super().__new__(cls, sdf, closest, face, feature)
        self.points = points
        return self

    def normal(self, points=None):
        """[n,3]: sign * (x - closest) / |x - closest|, the gradient of the signed distance wherever it has one; 0 where the distance is 0."""
        x = self.points if points is None else points
        r = x - self.closest
        length = torch.linalg.norm(r, dim=1, keepdim=True)
        sign = torch.where(self.sdf < 0, -1.0, 1.0).to(r.dtype)[:, None]
        return torch.where(length > 0, sign * r / length.clamp_min(torch.finfo(r.dtype).tiny), torch.zeros_like(r))


class _MeshRayHit(NamedTuple):
    t: torch.Tensor              # [n] f32: the ray parameter of the hit in units of |d|; +inf on a miss
    face: torch.Tensor           # [n] int32: the face hit, a row of the faces MeshSDF was given; -1 on a miss
    bary: torch.Tensor           # [n,2] f32: (v, w), the hit point is a + v (b - a) + w (c - a); 0 on a miss
    side: torch.Tensor           # [n] int32: +1 the front of the face (d . cross(b - a, c - a) < 0), -1 its back, 0 a miss


class MeshRayHit(_MeshRayHit):
    """What MeshSDF.raycast returns; unpacks as (t, face, bary, side).  All detached: the query has no gradients."""

    def __new__(cls, t, face, bary, side, mesh=None):
        self = super().__new__(cls, t, face, bary, side)
        self.mesh = mesh
        return self

    @property
    def hit(self):
        """bool [n]: the ray met the mesh."""
        return torch.isfinite(self.t)

    def points(self, rays_o, rays_d):
        """[n,3]: o + t d; the origin on a miss."""
        return rays_o + torch.where(self.hit, self.t, torch.zeros_like(self.t))[:, None] * rays_d

    def normals(self, smooth=None):
        """[n,3] unit normals at the hit points, turned towards the ray's origin; 0 on a miss.  The geometric normal of the face, or,
        with smooth = per-vertex normals [V,3] (a Mesh's), those of the face's corners interpolated by `bary`.  Needs details=True."""
        if self.face is None:
            raise ValueError("normals() needs the face, bary and side of a raycast with details=True")
        hit = self.face >= 0
        corners = self.mesh.faces[self.face.clamp_min(0).long()].long()                  # [n,3] vertex indices
        a, b, c = (self.mesh.vertices[corners[:, k]] for k in range(3))
        geometric = torch.cross(b - a, c - a, dim=1)
        front = (self.side > 0)[:, None]
        if smooth is None:
            n = torch.where(front, geometric, -geometric)
        else:
            sn = torch.as_tensor(smooth, dtype=torch.float32, device=a.device)
            if tuple(sn.shape) != tuple(self.mesh.vertices.shape):
                raise ValueError("smooth must hold one normal per vertex, %s, got %s" % (tuple(self.mesh.vertices.shape), tuple(sn.shape)))
            v, w = self.bary[:, :1], self.bary[:, 1:]
            n = sn[corners[:, 0]] * (1.0 - v - w) + sn[corners[:, 1]] * v + sn[corners[:, 2]] * w
            agrees = ((n * geometric).sum(1, keepdim=True) >= 0) == front                  # the interpolated normal, on the side that was hit
            n = torch.where(agrees, n, -n)
        length = torch.linalg.norm(n, dim=1, keepdim=True)
        return torch.where(hit[:, None] & (length > 0), n / length.clamp_min(torch.finfo(n.dtype).tiny), torch.zeros_like(n))


# ---- per-mesh data, on the host in float64 -----------------------------------------------------------------------------------------------
def weld_vertices(vertices):
    """Merge vertices with bit-identical positions -> (unique vertices [U,3] f32 in order of first appearance, index [V] of each old
    vertex among them)."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    keys = v.view(np.uint32).astype(np.uint64)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))            # unique sorts by key: renumber by first appearance
    return v[np.sort(first)], rank[inverse.reshape(-1)]


def pseudonormals(vertices, faces):
    """Angle-weighted pseudonormals of an indexed mesh, float64 -> (edge [T,3,3]: per face and edge ab / bc / ca the sum of the unit
    normals of ALL faces that use the edge (by vertex indices, either direction); vertex [V,3]: the sum over the faces at the vertex of
    (interior angle there) x (unit normal)).  A zero-area face contributes nothing.  Deterministic: np.add.at adds in face order."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(b - a, c - a)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where(length > 0, n / length, 0.0)
    lo, hi = np.minimum(f, f[:, [1, 2, 0]]), np.maximum(f, f[:, [1, 2, 0]])               # [T,3]: edge e = (f[e], f[e + 1])
    _, inverse = np.unique((lo * max(len(v), 1) + hi).reshape(-1), return_inverse=True)
    sums = np.zeros((int(inverse.max()) + 1 if len(f) else 0, 3))
    np.add.at(sums, inverse.reshape(-1), np.repeat(unit, 3, axis=0))
    edge = sums[inverse.reshape(-1)].reshape(-1, 3, 3)
    vertex = np.zeros_like(v)
    corners = (a, b, c)
    for k in range(3):
        e1, e2 = corners[(k + 1) % 3] - corners[k], corners[(k + 2) % 3] - corners[k]
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = (e1 * e2).sum(1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
        angle = np.where(np.isfinite(cos), np.arccos(np.clip(cos, -1.0, 1.0)), 0.0)
        np.add.at(vertex, f[:, k], angle[:, None] * unit)
    return edge, vertex


def _spread21(x):
    """Bits 0..20 of an int64 tensor moved to every third position."""
    x = x & 0x1fffff
    x = (x | (x << 32)) & 0x1f00000000ffff
    x = (x | (x << 16)) & 0x1f0000ff0000ff
    x = (x | (x << 8)) & 0x100f00f00f00f00f
    x = (x | (x << 4)) & 0x10c30c30c30c30c3
    x = (x | (x << 2)) & 0x1249249249249249
    return x


def morton_order(points, lo, hi):
    """Stable argsort of points [n,3] by the 63-bit Morton code of their position in the box [lo, hi] (21 bits per axis)."""
    extent = (hi - lo).clamp_min(torch.finfo(torch.float32).tiny)
    q = (((points - lo) / extent).clamp(0.0, 1.0).to(torch.float64) * 2097151.0).to(torch.int64)
    code = _spread21(q[:, 0]) | (_spread21(q[:, 1]) << 1) | (_spread21(q[:, 2]) << 2)
    return torch.argsort(code, stable=True)


def sample_surface(vertices, faces, n, generator=None):
    """n points on the faces, a face picked in proportion to its area (inverse CDF in float64), uniform barycentrics -> (points [n,3]
    f32, face index [n] int64).  Plain torch on the device of `vertices`; the random numbers are drawn on the generator's device (the
    CPU without one), so a generator fixes the result."""
    dev = vertices.device
    rdev = generator.device if generator is not None else torch.device("cpu")
    f = faces.long()
    a, b, c = vertices[f[:, 0]], vertices[f[:, 1]], vertices[f[:, 2]]
    area = torch.linalg.norm(torch.cross((b - a).double(), (c - a).double(), dim=1), dim=1)
    cdf = torch.cumsum(area, 0)
    if not (len(f) and float(cdf[-1]) > 0):
        raise ValueError("the mesh has no area to sample")
    u = torch.rand(n, 3, generator=generator, device=rdev, dtype=torch.float64).to(dev)
    idx = torch.searchsorted(cdf, u[:, 0] * cdf[-1], right=True).clamp_max(len(f) - 1)
    s = u[:, 1].sqrt()
    w0, w1, w2 = (1.0 - s).float()[:, None], (s * (1.0 - u[:, 2])).float()[:, None], (s * u[:, 2]).float()[:, None]
    return a[idx] * w0 + b[idx] * w1 + c[idx] * w2, idx


def _as_numpy(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


class MeshSDF:
    """Distance queries against one triangle mesh.

    vertices [V,3] float32, faces [T,3] int32 / int64 (tensors on any device, or arrays).  signed: the sign by pseudonormals (a closed,
    consistently oriented mesh: negative inside), else the plain distance.  weld: merge vertices with bit-identical positions first -- a
    triangle soup otherwise has one-face edges everywhere and the edge and vertex normals are those of single faces.  leaf_size: faces
    per leaf of the hierarchy, 1..8.  Raises ValueError for a wrong shape or dtype, an index outside [0, V) or a mesh without a face
    that has three different indices, all before any launch.  Faces with two equal indices are dropped (`n_dropped`); the `face` a query
    returns still counts rows of the `faces` given here.  sign (with signed=True): "pseudonormal", or "winding" -- negative where the
    generalized winding number is at least 0.5 (beta 2, order 2), right for open, overlapping and unwelded meshes; no pseudonormals are
    then computed."""

    def __init__(self, vertices, faces, signed=True, weld=False, leaf_size=4, device="cuda", sign="pseudonormal"):
        if sign not in ("pseudonormal", "winding"):
            raise ValueError("sign must be 'pseudonormal' or 'winding', got %r" % (sign,))
        v, f = _as_numpy(vertices), _as_numpy(faces)
        if v.ndim != 2 or v.shape[1] != 3 or v.dtype != np.float32:
            raise ValueError("vertices must be float32 [V,3], got %s %s" % (v.dtype, v.shape))
        if f.ndim != 2 or f.shape[1] != 3 or f.dtype not in (np.int32, np.int64):
            raise ValueError("faces must be int32 or int64 [T,3], got %s %s" % (f.dtype, f.shape))
        if not 1 <= int(leaf_size) <= ops.MESH_SDF_MAX_LEAF:
            raise ValueError("leaf_size must be in 1..%d, got %r" % (ops.MESH_SDF_MAX_LEAF, leaf_size))
        if len(f) == 0 or len(v) == 0:
            raise ValueError("the mesh is empty: %d vertices, %d faces" % (len(v), len(f)))
        if f.min() < 0 or f.max() >= len(v):
            raise ValueError("face indices must lie in [0, %d), got %d .. %d" % (len(v), f.min(), f.max()))
        if not np.isfinite(v).all():
            raise ValueError("vertices must be finite")
        f = f.astype(np.int64)
        if weld:
            v, index = weld_vertices(v)
            f = index[f]
        keep = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
        self.n_dropped = int((~keep).sum())
        if not keep.any():
            raise ValueError("every face of the mesh uses a vertex twice: nothing to measure a distance to")
        kept = np.nonzero(keep)[0]
        self.signed, self.leaf_size, self.sign = bool(signed), int(leaf_size), sign
        self._moments = None
        self.vertices = torch.from_numpy(np.ascontiguousarray(v)).to(device)
        self.faces = torch.from_numpy(np.ascontiguousarray(f.astype(np.int32))).to(device)
        self.edge_normals = self.vertex_normals = None
        if signed and sign == "pseudonormal":
            en = np.zeros((len(f), 3, 3))
            en[kept], vn = pseudonormals(v, f[kept])
            self.edge_normals = torch.from_numpy(en.astype(np.float32)).to(device)
            self.vertex_normals = torch.from_numpy(vn.astype(np.float32)).to(device)
        self.lo, self.hi = self.vertices.min(0).values, self.vertices.max(0).values
        kept_t = torch.from_numpy(kept).to(device)
        centroid = self.vertices[self.faces[kept_t].long()].mean(1)
        self.order = kept_t[morton_order(centroid, self.lo, self.hi)].to(torch.int32).contiguous()
        self.boxes = ops.mesh_bvh_build(self.vertices, self.faces, self.order, self.leaf_size)

    @classmethod
    def from_mesh(cls, mesh, **kw):
        """From a Mesh (extract_mesh, marching_tetrahedra, read_ply, read_obj); its vertex normals are not used."""
        return cls(mesh.vertices, mesh.faces, **kw)

    @property
    def n_faces(self):
        return int(self.order.shape[0])

    def __call__(self, points, details=True):
        """points [n,3] f32 on the device -> MeshDistance(sdf [n], closest [n,3], face [n], feature [n]); details=False fills only sdf.
        There are no gradients, neither to the points nor to the mesh: the outputs are detached (use MeshDistance.normal() for the
        direction of steepest ascent)."""
        x = points.detach()
        out = ops.mesh_sdf_query(x, self.vertices, self.faces, self.order, self.boxes, self.leaf_size, self.edge_normals,
                                 self.vertex_normals, details=details)
        if self.signed and self.sign == "winding":
            out = (torch.where(self.winding(x) >= 0.5, -out[0], out[0]),) + tuple(out[1:])
        return MeshDistance(*out, points=x)

    @property
    def moments(self):
        """f32 [2 P - 1, 20]: the per-node moments of the winding number (csrc/mesh_winding.hip), built on first use."""
        if self._moments is None:
            self._moments = ops.mesh_winding_build(self.vertices, self.faces, self.order, self.boxes, self.leaf_size)
        return self._moments

    def winding(self, points, beta=2.0, order=2):
        """points [n,3] f32 on the device -> the generalized winding number [n] f32 (csrc/mesh_winding.hip): 1 inside a closed mesh whose
        faces are counter-clockwise seen from outside, 0 outside, fractional near a hole, the number of enclosing shells where closed
        parts overlap.  A node of the hierarchy farther than beta x its radius is replaced by its expansion of `order` terms (1 or 2);
        beta = inf sums every face.  Detached: there are no gradients.  Works with signed=False."""
        x = points.detach()                         # checked here as ops would: before the first use builds the moments
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError("points must be [n,3], got %s" % (tuple(x.shape),))
        if not float(beta) >= 1.0:
            raise ValueError("beta must be at least 1, got %r" % (beta,))
        if order not in (1, 2):
            raise ValueError("order must be 1 or 2, got %r" % (order,))
        ops._dev(x, torch.float32, "points")
        return ops.mesh_winding_query(x, self.vertices, self.faces, self.order, self.moments, self.leaf_size, beta=beta, order_terms=order)

    def inside(self, points, **kw):
        """bool [n]: winding(points, **kw) >= 0.5."""
        return self.winding(points, **kw) >= 0.5

    def raycast(self, rays_o, rays_d, t_min=0.0, t_max=float("inf"), any_hit=False, cull=None, details=True):
        """rays_o, rays_d [n,3] f32 on the device (directions need not be normalised) -> MeshRayHit(t [n], face [n], bary [n,2], side [n]):
        the first face along o + t d with t in [t_min, t_max] (csrc/mesh_raycast.hip: the watertight test, no ray slips between two faces
        that share an edge or a vertex); details=False fills only t.  any_hit: stop at the first face met, the occlusion query -- t and
        face are then those of SOME face in range.  cull: None, "back" or "front" (a face shows its front where d . cross(b - a, c - a)
        < 0).  There are no gradients: the outputs are detached.  Works with signed=False: the pseudonormals are not used."""
        out = ops.mesh_raycast(rays_o.detach(), rays_d.detach(), self.vertices, self.faces, self.order, self.boxes, self.leaf_size,
                               t_min=t_min, t_max=t_max, any_hit=any_hit, cull=cull, details=details)
        return MeshRayHit(*out, mesh=self)

    def visible(self, a, b, eps=1e-4):
        """bool [n]: the open segment from a [n,3] to b [n,3] meets no face -- any-hit along d = b - a with t in [eps, 1 - eps]."""
        a = a.detach()
        d = (b.detach() - a).contiguous()
        return ~self.raycast(a, d, t_min=float(eps), t_max=1.0 - float(eps), any_hit=True, details=False).hit

    def sample(self, n, sigma=0.01, uniform_fraction=0.25, generator=None, pad=0.1):
        """Training points [n,3] f32: round(n (1 - uniform_fraction)) on the surface (area-weighted faces, uniform barycentrics) moved by a
        normal-distributed offset of scale sigma per axis, then the rest uniform in the bounding box padded by `pad` x its longest side
        on every face.  Plain torch, deterministic for a given generator."""
        n_uniform = int(round(n * float(uniform_fraction)))
        if not 0 <= n_uniform <= n:
            raise ValueError("uniform_fraction must lie in [0, 1]")
        rdev = generator.device if generator is not None else torch.device("cpu")
        dev = self.vertices.device
        near, _ = sample_surface(self.vertices, self.faces[self.order.long()], n - n_uniform, generator)
        near = near + float(sigma) * torch.randn(n - n_uniform, 3, generator=generator, device=rdev).to(dev)
        margin = float(pad) * (self.hi - self.lo).max()
        u = torch.rand(n_uniform, 3, generator=generator, device=rdev).to(dev)
        return torch.cat([near, (self.lo - margin) + u * ((self.hi - self.lo) + 2 * margin)]).contiguous()


def surface_distance(mesh_a, mesh_b, n=65536, generator=None, leaf_size=4):
    """How far apart two surfaces are: n area-weighted samples of a measured against b and n of b against a, unsigned ->
    dict(a_to_b_mean, a_to_b_max, b_to_a_mean, b_to_a_max, mean = the average of the two means, max = the larger maximum: the
    sampled Hausdorff distance)."""
    a = MeshSDF(mesh_a.vertices, mesh_a.faces, signed=False, leaf_size=leaf_size)
    b = MeshSDF(mesh_b.vertices, mesh_b.faces, signed=False, leaf_size=leaf_size)
    out = {}
    for name, src, dst in (("a_to_b", a, b), ("b_to_a", b, a)):
        x, _ = sample_surface(src.vertices, src.faces[src.order.long()], n, generator)
        d = dst(x.contiguous(), details=False).sdf
        out[name + "_mean"], out[name + "_max"] = float(d.mean()), float(d.max())
    out["mean"] = 0.5 * (out["a_to_b_mean"] + out["b_to_a_mean"])
    out["max"] = max(out["a_to_b_max"], out["b_to_a_max"])
    return out


def render_mesh(target, K, c2w, img_wh, cull=None, smooth=None, colors=None):
    """Depth, normal, mask and face images of a mesh seen from one camera: target a MeshSDF or a Mesh (a hierarchy is then built here,
    unsigned), K [3,3] intrinsics, c2w [3,4] (right, down, front | position), img_wh = (W, H) -> dict(depth [H,W] f32, normal [H,W,3]
    f32, mask [H,W] bool, face [H,W] int32).  The rays are those of get_ray_directions / get_rays, their directions normalised as
    render_surface_traced normalises them: depth is the EUCLIDEAN DISTANCE from the camera centre along the pixel's ray -- what
    render_surface_traced reports as `depth` and trace_surface as `t`, and what render() reports for unit directions -- so the images
    subtract directly where both hit.  Where the ray misses, depth is +inf (the traced renderers write 0 there): mask = isfinite(depth).
    normal: unit, towards the camera, the face's own or, with smooth = True (a Mesh's vertex normals) or a [V,3] tensor, interpolated;
    0 on a miss.  cull as MeshSDF.raycast.  colors: per-vertex colours [V,3] (bake_image_colors, bake_field_colors); the result then
    also holds rgb [H,W,3] f32, the colours of the hit face's corners a, b, c interpolated as a (1 - v - w) + b v + c w at the hit's
    barycentrics, 0 on a miss."""
    from .rays import get_ray_directions, get_rays
    mesh_normals = getattr(target, "normals", None)
    if not isinstance(target, MeshSDF):
        target = MeshSDF(target.vertices, target.faces, signed=False)
    if smooth is True:
        if mesh_normals is None or callable(mesh_normals):
            raise ValueError("smooth=True needs a Mesh with vertex normals; pass the normals [V,3] instead")
        smooth = mesh_normals
    w, h = int(img_wh[0]), int(img_wh[1])
    dev = target.vertices.device
    K = torch.as_tensor(K, dtype=torch.float32)
    directions = get_ray_directions(h, w, K, device=dev)
    rays_o, rays_d = get_rays(directions, torch.as_tensor(c2w, dtype=torch.float32).to(dev))
    rays_d = (rays_d / torch.linalg.norm(rays_d, dim=1, keepdim=True)).contiguous()
    hit = target.raycast(rays_o.contiguous(), rays_d, cull=cull)
    out = {"depth": hit.t.view(h, w), "normal": hit.normals(smooth).view(h, w, 3), "mask": hit.hit.view(h, w), "face": hit.face.view(h, w)}
    if colors is not None:
        col = torch.as_tensor(colors, dtype=torch.float32, device=dev)
        if tuple(col.shape) != tuple(target.vertices.shape):
            raise ValueError("colors must hold one rgb triple per vertex, %s, got %s" % (tuple(target.vertices.shape), tuple(col.shape)))
        corners = target.faces[hit.face.clamp_min(0).long()].long()
        v, wb = hit.bary[:, :1], hit.bary[:, 1:]
        rgb = col[corners[:, 0]] * (1.0 - v - wb) + col[corners[:, 1]] * v + col[corners[:, 2]] * wb
        out["rgb"] = torch.where((hit.face >= 0)[:, None], rgb, torch.zeros_like(rgb)).view(h, w, 3)
    return out


__all__ = ["Mesh", "MeshDistance", "MeshRayHit", "MeshSDF", "morton_order", "pseudonormals", "render_mesh", "sample_surface", "surface_distance",
           "weld_vertices"]
