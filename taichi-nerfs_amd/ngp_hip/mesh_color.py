"""Vertex colours for a mesh: baked from posed images (csrc/mesh_color.hip, with the occlusion query of csrc/mesh_raycast.hip) or
read off a radiance field at the vertices.

    mesh = smooth_mesh(clean_mesh(extract_mesh(model, 256, thr))[0]).mesh          # bake LAST: colours belong to the final vertices
    vc = bake_image_colors(mesh, images, K, c2w)                                   # VertexColors(colors, weight, views, filled)
    rgb = bake_field_colors(model, mesh)                                           # [V,3]: the model's colour looking down the normal
    write_ply("scene.ply", mesh, colors=vc.colors)
    render_mesh(mesh, K, pose, (W, H), colors=vc.colors)["rgb"]

bake_image_colors projects every vertex into every view, asks the mesh itself whether anything lies between the vertex and the camera,
and blends what the unoccluded views show with the weight cos^2 of the angle between the normal and the view direction (mode="best":
the most frontal view alone).  Vertices no view shows take the mean of their coloured neighbours, ring by ring.  The contract is
DESIGN.md section 3, "Vertex colours"; the result is deterministic and has the same bits for every workspace size."""
from typing import NamedTuple

import torch

from . import ops
from .mesh_sdf import MeshSDF


class VertexColors(NamedTuple):
    colors: torch.Tensor                    # [V,3] f32
    weight: torch.Tensor                    # [V] f32: the sum of the weights cos^2 of the views that count; "best": the winner's; 0 where none
    views: torch.Tensor                     # [V] int32: the views that count ("best": 1 where there is one)
    filled: torch.Tensor                    # [V] uint8: 0 baked, r filled from the neighbours in round r, 255 the default colour


def _occluder(mesh):
    """The unsigned MeshSDF of a mesh for the occlusion query, or None if no face is left.  A face that names a vertex that is not
    finite occludes nothing; such vertices are placed at 0 for the hierarchy's sake (no kept face names them).  Host work, as every
    MeshSDF construction: pass target= to bake_image_colors to avoid it."""
    v, f = mesh[0].detach(), mesh[1].detach()
    if v.shape[0] == 0 or f.shape[0] == 0:
        return None
    finite = torch.isfinite(v).all(1)
    in_range = ((f >= 0) & (f < v.shape[0])).all(1)
    keep = in_range & finite[f.clamp(0, v.shape[0] - 1).long()].all(1)
    keep &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    if not bool(keep.any()):
        return None
    return MeshSDF(torch.where(finite[:, None], v, torch.zeros_like(v)), f[keep], signed=False, device=v.device)


def _default_eps(lo, hi):
    """1e-3 x the diagonal of the box [lo, hi], f32 [1] on the device: the squares and their sum in f64, one rounding to f32."""
    d = (hi.double() - lo.double())
    return (1e-3 * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).sqrt()).to(torch.float32).reshape(1)


def bake_image_colors(mesh, images, K, c2w, normals=None, mode="blend", eps=None, cos_min=0.1, near=1e-6, two_sided=False, fill_rounds=8,
                      default_color=(0.5, 0.5, 0.5), target=None, workspace_bytes=256 << 20):
    """Vertex colours from posed images -> VertexColors.  mesh: a Mesh or (vertices f32 [V,3], faces int32 [T,3]) on the device; images
    f32 [N,H,W,C >= 3] on the device (the first three channels); K [3,3] shared or [N,3,3]; c2w [N,3,4] (or [N,4,4]) in render_mesh's
    convention (right, down, front | position), pixel centres at (i + 0.5, j + 0.5) as get_ray_directions.
    normals: unit normals [V,3], default mesh.normals, else vertex_normals(mesh).  A view counts for a vertex when the cosine between the
    normal and the direction to the camera exceeds cos_min (two_sided: the normal is first turned towards the camera), the vertex lies
    farther than `near` in front of the camera, its bilinear sample position lies inside the image, and the segment from v + eps n to the
    camera meets no face.  eps: default 1e-3 x the diagonal of the mesh's box.  mode "blend": the mean of the views that count with the
    weights cos^2; "best": the view with the largest cosine alone (the lowest index of equal ones).
    fill_rounds (0..254): a vertex without a view takes the mean of its coloured neighbours, one ring per round; what is still
    uncoloured afterwards gets default_color and filled = 255.
    target: a MeshSDF of this same mesh, to reuse its hierarchy; without one a hierarchy is built here (host work, as always).  The
    cameras are cut into chunks whose per-pair buffers stay below workspace_bytes (at least one camera per chunk); the result does not
    depend on the cut.  With target given nothing is read back from the device."""
    vertices, faces = mesh[0], mesh[1]
    n_faces, n_vertices = ops._mesh_arrays(vertices, faces)
    dev = vertices.device
    if mode not in ops.MESH_COLOR_MODES:
        raise ValueError('mode must be "blend" or "best", got %r' % (mode,))
    fill_rounds = int(fill_rounds)
    if not 0 <= fill_rounds < ops.MESH_COLOR_UNCOLOURED:
        raise ValueError("fill_rounds must be in 0..254, got %r" % (fill_rounds,))
    if not float(cos_min) >= 0.0 or not float(near) >= 0.0:
        raise ValueError("cos_min and near must be >= 0, got %r and %r" % (cos_min, near))
    images = ops._dev(images, torch.float32, "images")
    if images.dim() != 4 or images.shape[3] < 3:
        raise ValueError("images must be [N,H,W,C] with C >= 3, got %s" % (tuple(images.shape),))
    n_cameras, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    K = torch.as_tensor(K, dtype=torch.float32).to(dev).contiguous()
    c2w = torch.as_tensor(c2w, dtype=torch.float32).to(dev)
    if c2w.dim() == 3 and tuple(c2w.shape[1:]) == (4, 4):
        c2w = c2w[:, :3, :]
    c2w = c2w.contiguous()
    if tuple(c2w.shape) != (n_cameras, 3, 4) or tuple(K.shape) not in ((3, 3), (n_cameras, 3, 3)):
        raise ValueError("c2w must be [N,3,4] and K [3,3] or [N,3,3] for the %d images, got %s and %s" % (n_cameras, tuple(c2w.shape), tuple(K.shape)))
    if normals is None:
        normals = getattr(mesh, "normals", None)
    if normals is None:
        normals = ops.mesh_vertex_normals(vertices, faces)
    normals = ops._dev(normals.detach(), torch.float32, "normals")
    if len(tuple(default_color)) != 3:
        raise ValueError("default_color must hold three values")
    default = torch.cat([torch.full((1,), float(x), device=dev, dtype=torch.float32) for x in default_color])     # fills: no copy to wait for
    accum = torch.zeros(n_vertices, 4, device=dev, dtype=torch.float64)
    views = torch.zeros(n_vertices, device=dev, dtype=torch.int32)
    best_cos = torch.zeros(n_vertices, device=dev, dtype=torch.float32) if mode == "best" else None
    if target is None:
        target = _occluder(mesh)
    elif not isinstance(target, MeshSDF):
        raise TypeError("target must be a MeshSDF of this mesh")
    if n_vertices and n_cameras and w and h:
        if eps is None:
            finite = torch.isfinite(vertices).all(1, keepdim=True)
            inf = torch.full((1, 3), float("inf"), device=dev)
            lo = torch.cat([torch.where(finite, vertices, inf), inf]).amin(0)
            hi = torch.cat([torch.where(finite, vertices, -inf), -inf]).amax(0)
            eps_t = _default_eps(lo, hi)
        else:
            eps_t = torch.full((1,), float(eps), device=dev, dtype=torch.float32)
        per_chunk = max(1, min(n_cameras, int(workspace_bytes) // (ops.MESH_COLOR_PAIR_BYTES * n_vertices), (2**31 - 1) // n_vertices))
        for n0 in range(0, n_cameras, per_chunk):
            n1 = min(n0 + per_chunk, n_cameras)
            rays_o, rays_d, sample, weight, cosv = ops.mesh_color_project(vertices, normals, K if K.dim() == 2 else K[n0:n1], c2w[n0:n1], (w, h),
                                                                          eps_t, cos_min, near, two_sided)
            if target is not None:
                t = target.raycast(rays_o, rays_d, t_min=0.0, t_max=1.0, any_hit=True, details=False).t
            else:                                                          # no face: nothing occludes
                t = torch.full_like(weight, float("inf"))
            ops.mesh_color_accumulate(images[n0:n1], sample, weight, cosv, t, accum, views, best_cos, mode)
    colors, weight, filled = ops.mesh_color_finish(accum, views)
    if fill_rounds and n_faces and n_vertices:
        row_start, neighbours = ops.mesh_adjacency(vertices, faces)[:2]    # the raw arrays: no host read
        filled = ops.mesh_color_fill(colors, filled, row_start, neighbours, fill_rounds)
    colors = torch.where((filled == ops.MESH_COLOR_UNCOLOURED)[:, None], default, colors)
    return VertexColors(colors, weight, views, filled)


def bake_field_colors(model, mesh, normals=None, offset=0.0, chunk=2**20):
    """The colour a radiance field shows at the vertices, looking down the normal -> [V,3] f32: x = v + offset n, d = -n, evaluated
    under torch.no_grad() in the caller's autocast state, `chunk` vertices per call.  model: an NGP or VoxelGrid (model(x, d) -> (sigmas,
    rgbs)), an SDFField (sdf_and_grad, then color(feature, unit gradient, d)), or any callable (x, d) -> rgb [n,3].  normals: default
    mesh.normals, else vertex_normals(mesh)."""
    vertices, faces = mesh[0], mesh[1]
    if normals is None:
        normals = getattr(mesh, "normals", None)
    if normals is None:
        normals = ops.mesh_vertex_normals(vertices, faces)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive")
    n_vertices = int(vertices.shape[0])
    out = torch.empty(n_vertices, 3, device=vertices.device, dtype=torch.float32)
    with torch.no_grad():
        for start in range(0, n_vertices, chunk):
            n = normals[start:start + chunk]
            x = (vertices[start:start + chunk] + float(offset) * n).contiguous()
            d = (-n).contiguous()
            if hasattr(model, "sdf_and_grad") and hasattr(model, "color"):
                _, feature, grad = model.sdf_and_grad(x)
                rgb = model.color(feature, grad / torch.linalg.norm(grad, dim=1).clamp_min(1e-12)[:, None], d)     # as render_surface_traced
            else:
                rgb = model(x, d)
                if isinstance(rgb, (tuple, list)):
                    rgb = rgb[1]
            if tuple(rgb.shape) != (x.shape[0], 3):
                raise ValueError("the model must return one rgb triple per point, got %s for %d points" % (tuple(rgb.shape), x.shape[0]))
            out[start:start + chunk] = rgb.to(torch.float32)
    return out


__all__ = ["VertexColors", "bake_field_colors", "bake_image_colors"]
