"""Fit a signed-distance field to a triangle mesh: supervision from geometry instead of from images, and a mesh -> field -> mesh round trip
that is measured at both ends.  Needs no data file.

    python examples/fit_sdf_mesh.py
    python examples/fit_sdf_mesh.py --steps 200 --n 4096 --log2_T 14 --levels 8 --max_res 128 --target_resolution 32 --resolution 48
    python examples/fit_sdf_mesh.py --target two_spheres --sign winding

The target is made here: a torus (R 0.25, r 0.1, centred in [-0.5, 0.5]^3), extracted with marching tetrahedra from its analytic SDF at
--target_resolution cells per axis.  MeshSDF answers the distance to THAT MESH (BVH closest-point query, csrc/mesh_sdf.hip) at the
points MeshSDF.sample draws every step: most near the surface, the rest uniform in the padded bounding box.  SDFField (hash encoder,
twice differentiable, + MLP, starting as a sphere of radius 0.25) is fitted with
    loss = mean |f - sdf_mesh| + eikonal_weight * mean (|grad_x f| - 1)^2
as in fit_sdf_eikonal.py, and its zero set is extracted again at --resolution.  One JSON line reports the SDF loss first / last, the
eikonal error, surface_distance between the target and the result (and the untrained sphere) in units of the extraction cell, topology()
of both meshes and the time of the distance query per step.

--target two_spheres replaces the torus by two overlapping icospheres (radius 0.2, centres 0.25 apart, concatenated as they are: two
closed shells, one inside the other in part).  With --sign pseudonormal (the default) the distance is negative only where the NEAREST
face says so, so the part of each sphere inside the other keeps a spurious wall and the field is fitted to it; --sign winding takes
the sign from the generalized winding number (csrc/mesh_winding.hip) and the target is the union.  `sign_disagreement` in the report is
the share of one batch of training points on which the two signs differ, and `sign_wrong` the share on which the chosen sign differs
from the analytic union of the two spheres (two_spheres only; points nearer to either sphere than 0.02 are left out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

BOUNDS = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))


def torus_sdf(x, R=0.25, r=0.1):
    return torch.sqrt((torch.linalg.norm(x[:, :2], dim=1) - R) ** 2 + x[:, 2] ** 2) - r


TWO_SPHERES = (((-0.125, 0.0, 0.0), (0.125, 0.0, 0.0)), 0.2)


def icosphere(subdivisions, centre, radius):
    """(vertices [V,3] f32, faces [T,3] int32) of a subdivided icosahedron, counter-clockwise seen from outside."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [torch.tensor(x, dtype=torch.float64) / (1.0 + t * t) ** 0.5 for x in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / torch.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return (torch.tensor(centre, dtype=torch.float64) + radius * torch.stack(v)).float(), torch.tensor(f, dtype=torch.int32)


def two_spheres(subdivisions, device):
    """The built-in target on which the two signs differ: two overlapping closed shells in one face list, unwelded."""
    from ngp_hip.mesh import Mesh
    centres, radius = TWO_SPHERES
    parts = [icosphere(subdivisions, c, radius) for c in centres]
    vertices = torch.cat([p[0] for p in parts])
    faces = torch.cat([parts[0][1], parts[1][1] + parts[0][0].shape[0]])
    return Mesh(vertices.to(device), faces.to(device), None)


def two_spheres_sdf(x):
    centres, radius = TWO_SPHERES
    return torch.stack([torch.linalg.norm(x - torch.tensor(c, device=x.device), dim=1) for c in centres]).min(0).values - radius


def fit(field, target_sdf, steps, n, sigma, uniform_fraction, lr, eikonal_weight, gen):
    """The fitting loop (examples/render_mesh.py runs it too): `steps` Adam steps of |f - sdf_mesh| + eikonal_weight (|grad f| - 1)^2 on
    the points target_sdf.sample draws from `gen` -> ([(sdf loss, eikonal error) of the first and the last step], the summed time of the
    distance queries in ms)."""
    opt = torch.optim.Adam(field.geo_layers.parameters(), lr=lr, eps=1e-15)
    opt.add_param_group({"params": field.pos_encoder.parameters()})
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hist, query_ms = [], 0.0
    for step in range(steps):
        x = target_sdf.sample(n, sigma, uniform_fraction, gen).clamp_(-0.5, 0.5)
        t0.record()
        d = target_sdf(x, details=False).sdf
        t1.record()
        f, _, grad = field.sdf_and_grad(x.requires_grad_(), create_graph=True)
        norm = torch.linalg.norm(grad, dim=1)
        sdf_loss = (f - d).abs().mean()
        loss = sdf_loss + eikonal_weight * ((norm - 1.0) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        t1.synchronize()
        query_ms += t0.elapsed_time(t1)
        if step in (0, steps - 1):
            hist.append((float(sdf_loss.detach()), float((norm.detach() - 1.0).abs().mean())))
    torch.cuda.synchronize()
    return hist, query_ms


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--n", type=int, default=16384, help="points per step")
    ap.add_argument("--log2_T", type=int, default=19)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--max_res", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--eikonal_weight", type=float, default=0.05)
    ap.add_argument("--sigma", type=float, default=0.02, help="scale of the offset of the near-surface samples")
    ap.add_argument("--uniform_fraction", type=float, default=0.25)
    ap.add_argument("--target_resolution", type=int, default=128, help="cells per axis of the target's extraction")
    ap.add_argument("--resolution", type=int, default=128, help="cells per axis of the result's extraction")
    ap.add_argument("--compare_n", type=int, default=65536, help="samples per direction of surface_distance")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--target", choices=("torus", "two_spheres"), default="torus")
    ap.add_argument("--sign", choices=("pseudonormal", "winding"), default="pseudonormal", help="where the sign of the distance comes from")
    ap.add_argument("--subdivisions", type=int, default=4, help="two_spheres: subdivisions of each icosphere (4: 5120 faces each)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this example needs the GPU: libngp_hip has no CPU path")
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    from ngp_hip import MeshSDF, SDFField, surface_distance
    from ngp_hip.mesh import extract_mesh, topology

    if args.target == "torus":
        target = extract_mesh(torus_sdf, args.target_resolution, 0.0, bounds=BOUNDS, sign=-1, normals=None, device=dev)
    else:
        target = two_spheres(args.subdivisions, dev)
    target_sdf = MeshSDF.from_mesh(target, sign=args.sign)
    other = MeshSDF.from_mesh(target, sign="winding" if args.sign == "pseudonormal" else "pseudonormal")
    probe = target_sdf.sample(args.n, args.sigma, args.uniform_fraction, torch.Generator().manual_seed(args.seed + 1)).clamp_(-0.5, 0.5)
    chosen = target_sdf(probe, details=False).sdf
    signs = {"sign_disagreement": float(((chosen < 0) != (other(probe, details=False).sdf < 0)).float().mean())}
    if args.target == "two_spheres":
        truth = two_spheres_sdf(probe)
        clear = torch.stack([(torch.linalg.norm(probe - torch.tensor(c, device=dev), dim=1) - TWO_SPHERES[1]).abs() for c in TWO_SPHERES[0]]).min(0).values > 0.02
        signs["sign_wrong"] = float(((chosen < 0) != (truth < 0))[clear].float().mean())
    field = SDFField(scale=0.5, levels=args.levels, log2_T=args.log2_T, max_res=args.max_res).to(dev)
    cell = 1.0 / args.resolution

    def extract():
        return extract_mesh(field.sdf, args.resolution, 0.0, bounds=BOUNDS, sign=-1, normals=None, device=dev)

    def compare(mesh):
        if mesh.faces.shape[0] == 0:
            return None
        sd = surface_distance(target, mesh, args.compare_n, torch.Generator().manual_seed(args.seed))
        return {"mean_cells": sd["mean"] / cell, "max_cells": sd["max"] / cell}

    untrained = compare(extract())
    hist, query_ms = fit(field, target_sdf, args.steps, args.n, args.sigma, args.uniform_fraction, args.lr, args.eikonal_weight,
                         torch.Generator().manual_seed(args.seed))
    result = extract()
    info = {"steps": args.steps, "points_per_step": args.n, "levels": args.levels, "log2_T": args.log2_T, "max_res": args.max_res,
            "target_resolution": args.target_resolution, "resolution": args.resolution, "target_faces": int(target.faces.shape[0]),
            "target_name": args.target, "sign": args.sign, **signs,
            "sdf_loss_first": hist[0][0], "sdf_loss_last": hist[-1][0], "eikonal_error_first": hist[0][1], "eikonal_error_last": hist[-1][1],
            "surface_distance_untrained": untrained, "surface_distance": compare(result),
            "topology_target": topology(target), "topology_result": topology(result),
            "query_ms_per_step": query_ms / max(args.steps, 1)}
    print(json.dumps(info))
    return dict(info, target=target, result=result, field=field)


if __name__ == "__main__":
    main()
