"""Look at a triangle mesh from a ring of cameras: depth, normal and mask images by ray casting (MeshSDF.raycast through render_mesh,
csrc/mesh_raycast.hip), and -- the image-space counterpart of surface_distance -- the same views of a signed-distance field fitted to the
mesh, sphere-traced and compared pixel by pixel.  Needs no data file.

    python examples/render_mesh.py                                  # the torus target of fit_sdf_mesh.py
    python examples/render_mesh.py scene.ply --views 12 --wh 400    # a mesh read with read_ply / read_obj, fitted into [-0.4, 0.4]^3
    python examples/render_mesh.py --against-field 1000 --json profiles/mesh_raycast_fit.json

Per view it writes <out>/view_XX_depth.png (near is bright), _normal.png ((n + 1) / 2) and _mask.png through the compat image writer,
and the raw depth as .npy.  With --against-field STEPS an SDFField is fitted to the mesh with the loop of fit_sdf_mesh.py (imported, not
copied); the views are sphere-traced with trace_surface before and after the fit, and one JSON line reports, for each of the two
fields, the share of pixels where the field's mask differs from the mesh's and the mean and maximum |t_trace - t_mesh| on the pixels both
hit -- plus the mean on the pixels that the mesh and BOTH fields hit, so the two figures can be compared."""
import argparse
import importlib.util
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fit_sdf_mesh  # noqa: E402


def ring(n, radius, height, device):
    """n cameras on a circle of `radius` at `height` above the origin's plane, looking at the origin -> c2w [n,3,4] (right, down, front)."""
    phi = 2 * math.pi * torch.arange(n, dtype=torch.float32) / n
    pos = torch.stack([radius * torch.cos(phi), radius * torch.sin(phi), torch.full_like(phi, height)], -1)
    fwd = torch.nn.functional.normalize(-pos, dim=-1)
    right = torch.nn.functional.normalize(torch.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd), dim=-1), dim=-1)
    down = torch.cross(fwd, right, dim=-1)
    return torch.cat([torch.stack([right, down, fwd], -1), pos[..., None]], -1).to(device)


def _image_writer():
    spec = importlib.util.spec_from_file_location("compat_imageio", os.path.join(ROOT, "taichi-nerfs_amd", "compat", "imageio.py"))
    imageio = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(imageio)
    return imageio.imwrite


def write_views(views, out_dir):
    """The three images of every view (and the depth as .npy) -> the list of files written."""
    os.makedirs(out_dir, exist_ok=True)
    written = []
    try:
        imwrite = _image_writer()
    except Exception:                                               # no PIL: the .npy files are the result
        imwrite = None
    for i, v in enumerate(views):
        depth, mask = v["depth"].cpu().numpy(), v["mask"].cpu().numpy()
        base = os.path.join(out_dir, "view_%02d" % i)
        np.save(base + "_depth.npy", depth)
        written.append(base + "_depth.npy")
        if imwrite is None:
            continue
        near, far = (depth[mask].min(), depth[mask].max()) if mask.any() else (0.0, 1.0)
        shade = np.where(mask, 1.0 - 0.8 * (np.where(mask, depth, near) - near) / max(far - near, 1e-12), 0.0)
        for name, img in (("depth", shade), ("normal", np.where(mask[..., None], 0.5 * (v["normal"].cpu().numpy() + 1.0), 0.0)), ("mask", mask.astype(np.float32))):
            imwrite("%s_%s.png" % (base, name), (np.clip(img, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8))
            written.append("%s_%s.png" % (base, name))
    return written


def trace_views(field, K, poses, wh):
    """trace_surface of the field for the cameras render_mesh used (the same rays) -> [(t [wh,wh], hit [wh,wh] bool)]."""
    from ngp_hip import trace_surface
    from ngp_hip.rays import get_ray_directions, get_rays
    directions = get_ray_directions(wh, wh, K, device=poses.device)
    out = []
    field.density_bitfield.fill_(255)                               # every cell may hold surface: the trace needs no trained occupancy
    for c2w in poses:
        rays_o, rays_d = get_rays(directions, c2w)
        rays_d = (rays_d / torch.linalg.norm(rays_d, dim=1, keepdim=True)).contiguous()
        tr = trace_surface(field, rays_o.contiguous(), rays_d)
        out.append((tr["t"].view(wh, wh), ((tr["status"] == 1) | (tr["status"] == 2)).view(wh, wh)))
    return out


def image_distance(views, traced, also=None):
    """Masks and hit parameters of the mesh's views against a field's -> dict(mask_differs: share of pixels, t_mean, t_max: |t_trace -
    t_mesh| over the pixels both hit, pixels: their number; with `also` (another field's traces) t_mean_common over the pixels all
    three hit)."""
    differs = pixels = n = 0
    total, worst, common_total, common_n = 0.0, 0.0, 0.0, 0
    for i, (v, (t, hit)) in enumerate(zip(views, traced)):
        both = hit & v["mask"]
        err = (t - v["depth"]).abs()
        differs += int((hit != v["mask"]).sum())
        pixels += hit.numel()
        n += int(both.sum())
        total += float(err[both].sum())
        worst = max(worst, float(err[both].max()) if both.any() else 0.0)
        if also is not None:
            common = both & also[i][1]
            common_total += float(err[common].sum())
            common_n += int(common.sum())
    out = {"mask_differs": differs / max(pixels, 1), "t_mean": total / max(n, 1), "t_max": worst, "pixels": n}
    if also is not None:
        out.update(t_mean_common=common_total / max(common_n, 1), pixels_common=common_n)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default=None, help=".ply or .obj; without one, the torus of fit_sdf_mesh.py")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--wh", type=int, default=200)
    ap.add_argument("--radius", type=float, default=1.5)
    ap.add_argument("--height", type=float, default=0.8)
    ap.add_argument("--out", default="render_mesh_out")
    ap.add_argument("--target_resolution", type=int, default=128, help="cells per axis of the torus' extraction")
    ap.add_argument("--smooth", action="store_true", help="interpolate the mesh's vertex normals where it has them")
    ap.add_argument("--against-field", dest="against_field", type=int, default=0, metavar="STEPS")
    ap.add_argument("--n", type=int, default=16384, help="points per fitting step")
    ap.add_argument("--log2_T", type=int, default=19)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--max_res", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--eikonal_weight", type=float, default=0.05)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--uniform_fraction", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this example needs the GPU: libngp_hip has no CPU path")
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    from ngp_hip import MeshSDF, SDFField, read_obj, read_ply, render_mesh
    from ngp_hip.mesh import Mesh, extract_mesh

    if args.mesh is None:
        mesh = extract_mesh(fit_sdf_mesh.torus_sdf, args.target_resolution, 0.0, bounds=fit_sdf_mesh.BOUNDS, sign=-1, normals="grid" if args.smooth else None,
                            device=dev)
    else:
        mesh = (read_ply if args.mesh.lower().endswith(".ply") else read_obj)(args.mesh)
        v = mesh.vertices.float()
        lo, hi = v.min(0).values, v.max(0).values
        mesh = Mesh(((v - 0.5 * (lo + hi)) * (0.8 / float((hi - lo).max()))).contiguous(), mesh.faces, mesh.normals)    # into [-0.4, 0.4]^3
    target = MeshSDF.from_mesh(mesh, signed=args.against_field > 0)
    K = torch.tensor([[1.2 * args.wh, 0.0, args.wh / 2], [0.0, 1.2 * args.wh, args.wh / 2], [0.0, 0.0, 1.0]])
    poses = ring(args.views, args.radius, args.height, dev)
    smooth = mesh.normals.to(dev) if args.smooth and mesh.normals is not None else None
    views = [render_mesh(target, K, c2w, (args.wh, args.wh), smooth=smooth) for c2w in poses]
    torch.cuda.synchronize()
    info = {"faces": target.n_faces, "views": args.views, "image_wh": args.wh, "covered": float(torch.stack([v["mask"] for v in views]).float().mean()),
            "out": write_views(views, args.out)}
    if args.against_field > 0:
        field = SDFField(scale=0.5, levels=args.levels, log2_T=args.log2_T, max_res=args.max_res).to(dev)
        before = trace_views(field, K.to(dev), poses, args.wh)
        hist, _ = fit_sdf_mesh.fit(field, target, args.against_field, args.n, args.sigma, args.uniform_fraction, args.lr, args.eikonal_weight,
                                   torch.Generator().manual_seed(args.seed))
        after = trace_views(field, K.to(dev), poses, args.wh)
        info.update(steps=args.against_field, points_per_step=args.n, levels=args.levels, log2_T=args.log2_T, max_res=args.max_res,
                    sdf_loss_first=hist[0][0], sdf_loss_last=hist[-1][0],
                    untrained=image_distance(views, before, also=after), trained=image_distance(views, after, also=before))
    print(json.dumps(info))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({k: v for k, v in info.items() if k != "out"}, fh, indent=1)
            fh.write("\n")
    return dict(info, views=views, mesh=mesh)


if __name__ == "__main__":
    main()
