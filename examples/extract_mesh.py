"""Save a mesh: sample a field on a regular grid and extract its isosurface by marching tetrahedra on the GPU (ngp_hip/mesh.py).

    python examples/extract_mesh.py --sdf --steps 500 --out sphere.ply                   # fit the sphere SDF, extract f = 0
    python examples/extract_mesh.py --train_steps 1000 --resolution 256 --out scene.ply   # train on the procedural scene, extract
    python examples/extract_mesh.py --ckpt model.pth --resolution 256 --out scene.obj     # a saved NGP state_dict

--sdf fits f(x) = MLP(HashEncoder(x)) to the signed distance of a sphere (centre 0.5, radius 0.3) in [0, 1]^3 with an eikonal term, as
examples/fit_sdf_eikonal.py does, and extracts the zero level with sign=-1 (solid where f < 0).  The other two modes extract the surface
density = threshold of an Instant-NGP model; the default threshold is the occupancy threshold of the training loop,
0.01 * MAX_SAMPLES / sqrt(3).  The file type follows the suffix of --out (.ply binary little-endian, .obj text).  One JSON line reports
V, T, the Euler characteristic V - E + T, the number of boundary edges (0 = closed surface) and the times.
--keep_largest K and --min_component_faces N (both off by default) remove floaters before the file is written (ngp_hip.clean_mesh:
connected components on the device) and print its report and the topology before and after.
--simplify_cell H, --simplify_resolution R or --target_faces N (all off by default, at most one) then make the mesh smaller
(ngp_hip.simplify_mesh: vertex clustering with quadric representatives, after the cleaning) and print V and T before and after.
--smooth N (off by default) runs N iterations of Taubin smoothing after the cleaning and before the simplification
(ngp_hip.smooth_mesh with boundary="fixed": the staircase of the grid goes, the faces stay as they are); no coordinate moves farther than
--smooth_max_move CELLS (default 0.5) spacings of the extraction grid.  It prints one JSON line: the seconds, the boundary vertices, the
mean and the largest displacement in cells; with --sdf, where the true surface is known, also the mean distance of the vertices from
the sphere (in cells) and the mean angle between the face normals and the sphere's (in degrees), before and after.  The normals of a
smoothed mesh are ngp_hip.vertex_normals of the new positions.
--colors field | images (off by default; --train_steps or --ckpt) colours the final mesh, after every other step: `field` asks the model
for its colour looking down the normal, --field_offset CELLS grid spacings along it from the vertex (default -2, inside: the level set of
the occupancy threshold lies in the fuzzy rim of the density, where the colour is barely trained; DESIGN.md has the PSNR per offset),
`images` renders --views N posed views of the procedural scene and bakes them
onto the vertices with an occlusion test against the mesh itself.  The file then carries the colours (uchar red green blue in a .ply,
`v x y z r g b` in an .obj), and one JSON line reports the seconds, how many vertices were baked, filled from their neighbours or left at
the default, and the PSNR of the coloured mesh rendered from held-out poses (ngp_hip.render_mesh(colors=)) against the synthetic views
there, over the pixels where both are hit."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def fit_sphere_sdf(args, dev):
    """The fit of examples/fit_sdf_eikonal.py -> (callable points [n,3] -> f [n], last SDF loss)."""
    from modules.hash_encoder import HashEncoder
    torch.manual_seed(args.seed)
    enc = HashEncoder(max_params=2**args.log2_T, levels=args.levels, max_res=args.max_res, twice_differentiable=True).to(dev)
    with torch.no_grad():
        enc.hash_table.uniform_(-1e-4, 1e-4)
    mlp = torch.nn.Sequential(torch.nn.Linear(enc.out_dim, args.width), torch.nn.Softplus(beta=100.0), torch.nn.Linear(args.width, 1)).to(dev)
    opt = torch.optim.Adam(list(enc.parameters()) + list(mlp.parameters()), lr=args.lr, eps=1e-15)
    gen = torch.Generator(dev).manual_seed(args.seed)
    sdf_loss = torch.zeros((), device=dev)
    for _ in range(args.steps):
        x = torch.rand(args.n, 3, device=dev, generator=gen).requires_grad_()
        f = mlp(enc(x)).squeeze(1)
        (grad,) = torch.autograd.grad(f.sum(), x, create_graph=True)
        sdf_loss = (f - (torch.linalg.norm(x.detach() - 0.5, dim=1) - 0.3)).abs().mean()
        loss = sdf_loss + args.eikonal_weight * ((torch.linalg.norm(grad, dim=1) - 1.0) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return (lambda pts: mlp(enc(pts.contiguous())).squeeze(1)), float(sdf_loss.detach())


def _cameras(n, radius, seed, device):
    g = torch.Generator().manual_seed(seed)
    z = 0.1 + 0.8 * torch.rand(n, generator=g)
    phi = 2 * math.pi * torch.rand(n, generator=g)
    r = (1 - z * z).sqrt()
    pos = radius * torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], -1)
    fwd = F.normalize(-pos, dim=-1)
    right = F.normalize(torch.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd), dim=-1), dim=-1)
    down = torch.cross(fwd, right, dim=-1)
    return torch.cat([torch.stack([right, down, fwd], -1), pos[..., None]], -1).to(device)


def train_procedural_model(steps, dev, wh=100, n_views=40, batch=8192):
    """An NGP trained on the procedural scene of ngp_hip.synthetic with the schedule of examples/train_procedural.py (FusedTrainer,
    occupancy update every 16 steps, 256 warm-up steps) -> (model, occupancy threshold)."""
    from modules.networks import NGP
    from modules.rendering import MAX_SAMPLES
    from ngp_hip.rays import RayBatcher
    from ngp_hip.synthetic import procedural_render_gt
    from ngp_hip.trainer import FusedTrainer
    torch.manual_seed(23)
    focal = 1111.1 * wh / 800
    ys, xs = torch.meshgrid(torch.arange(wh, device=dev), torch.arange(wh, device=dev), indexing="ij")
    dirs = torch.stack([(xs - wh / 2 + 0.5) / focal, (ys - wh / 2 + 0.5) / focal, torch.ones_like(xs, dtype=torch.float32)], -1).reshape(-1, 3)
    poses = _cameras(n_views, 1.39, 23, dev)
    imgs = torch.stack([procedural_render_gt(p[:, 3].expand_as(dirs), dirs @ p[:, :3].T) for p in poses])
    model = NGP(scale=0.5, max_res=1024).to(dev)
    K = torch.tensor([[focal, 0, wh / 2], [0, focal, wh / 2], [0, 0, 1]], device=dev)
    model.mark_invisible_cells(K, poses, (wh, wh))
    trainer = FusedTrainer(model, lr=1e-2, max_steps=max(steps, 1))
    batcher = RayBatcher(imgs, poses, dirs, batch_size=batch)
    thr = 0.01 * MAX_SAMPLES / 3**0.5
    for step in range(steps):
        cur = batcher.sample()
        if step % 16 == 0:
            trainer.update_density_grid(thr, warmup=step < 256)
        trainer.step(cur["rays_o"], cur["rays_d"], cur["rgb"])
    torch.cuda.synchronize()
    return model, thr


def color_mesh(how, msh, model, dev, n_views=40, wh=200, n_held_out=4, field_offset=0.0):
    """Vertex colours for a mesh of the procedural scene -> (colors [V,3], report).  how = "images": n_views posed views of the scene
    (ngp_hip.synthetic, the cameras of the training set's kind) baked with ngp_hip.bake_image_colors; "field": the model's colour at the
    vertices moved by field_offset (world units) along the normal, looking down the normal (ngp_hip.bake_field_colors, the evaluation
    loops' autocast).  The coloured mesh is then rendered
    from n_held_out other poses with render_mesh(colors=) and compared with the synthetic views there: the PSNR over the pixels where
    both the mesh and the scene are hit."""
    from ngp_hip import MeshSDF, bake_field_colors, bake_image_colors, render_mesh
    from ngp_hip.synthetic import procedural_render_gt
    focal = 1111.1 * wh / 800
    ys, xs = torch.meshgrid(torch.arange(wh, device=dev), torch.arange(wh, device=dev), indexing="ij")
    dirs = torch.stack([(xs - wh / 2 + 0.5) / focal, (ys - wh / 2 + 0.5) / focal, torch.ones_like(xs, dtype=torch.float32)], -1).reshape(-1, 3)
    K = torch.tensor([[focal, 0, wh / 2], [0, focal, wh / 2], [0, 0, 1]], device=dev)
    views = lambda poses: torch.stack([procedural_render_gt(p[:, 3].expand_as(dirs), dirs @ p[:, :3].T) for p in poses]).view(-1, wh, wh, 3)
    report = {"colors": how, "image_wh": wh}
    target = MeshSDF.from_mesh(msh, signed=False)
    torch.cuda.synchronize()
    t0 = time.time()
    if how == "images":
        poses = _cameras(n_views, 1.39, 41, dev)
        images = views(poses).contiguous()
        torch.cuda.synchronize()
        t1 = time.time()
        vc = bake_image_colors(msh, images, K, poses, target=target)
        colors = vc.colors
        torch.cuda.synchronize()
        report.update(views=n_views, render_seconds=t1 - t0, bake_seconds=time.time() - t1, baked=int((vc.filled == 0).sum()),
                      filled=int(((vc.filled > 0) & (vc.filled < 255)).sum()), default=int((vc.filled == 255).sum()),
                      mean_views=float(vc.views.float().mean()))
    else:
        with torch.autocast("cuda", dtype=torch.float16):
            colors = bake_field_colors(model, msh, offset=field_offset)
        torch.cuda.synchronize()
        report.update(bake_seconds=time.time() - t0, field_offset=field_offset)
    held_out = _cameras(n_held_out, 1.39, 977, dev)
    truth = views(held_out)
    se, count = 0.0, 0
    for pose, gt in zip(held_out, truth):
        out = render_mesh(target, K, pose, (wh, wh), colors=colors)
        both = out["mask"] & (gt < 0.999).any(-1)                            # the scene's background is white, its boxes never are
        se += float(((out["rgb"] - gt)[both] ** 2).sum())
        count += 3 * int(both.sum())
    report.update(held_out_views=n_held_out, pixels_compared=count // 3, psnr=-10.0 * math.log10(se / count) if count and se > 0 else None)
    return colors, report


def sphere_errors(msh, cell):
    """(mean | |v - 0.5| - 0.3 | over the vertices in cells, mean angle in degrees between the face normals and the sphere's normal at the
    face centroids) of a mesh of the --sdf sphere."""
    v, f = msh.vertices.double(), msh.faces.long()
    if not f.shape[0]:
        return None, None
    dist = ((v - 0.5).norm(dim=1) - 0.3).abs().mean() / cell
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = F.normalize(torch.cross(b - a, c - a, dim=1), dim=1)
    cos = (n * F.normalize((a + b + c) / 3 - 0.5, dim=1)).sum(1).clamp(-1.0, 1.0)
    return float(dist), float(torch.rad2deg(torch.acos(cos)).mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--sdf", action="store_true", help="fit the sphere SDF and extract its zero level")
    mode.add_argument("--train_steps", type=int, help="train an NGP on the procedural scene for this many steps, then extract")
    mode.add_argument("--ckpt", help="state_dict of an NGP(scale, max_res) model")
    ap.add_argument("--resolution", type=int, default=128, help="cells per axis")
    ap.add_argument("--threshold", type=float, default=None, help="density level (default: the occupancy threshold 0.01 * 1024 / sqrt(3))")
    ap.add_argument("--normals", default="grid", choices=["grid", "analytic", "none"])
    ap.add_argument("--out", default="mesh.ply", help=".ply or .obj")
    ap.add_argument("--compare", default=None, metavar="PATH.ply",
                    help="also report surface_distance (mean / max, both ways) between the extracted mesh and this one (.ply or .obj)")
    ap.add_argument("--keep_largest", type=int, default=None, metavar="K",
                    help="clean the mesh before writing it: keep the K connected components of the largest area (ngp_hip.clean_mesh)")
    ap.add_argument("--min_component_faces", type=int, default=0, metavar="N", help="clean the mesh: drop components of fewer than N faces")
    small = ap.add_mutually_exclusive_group()
    small.add_argument("--simplify_cell", type=float, default=None, metavar="H",
                       help="simplify the mesh before writing it: cluster the vertices on a grid of this edge length (ngp_hip.simplify_mesh)")
    small.add_argument("--simplify_resolution", type=int, default=None, metavar="R", help="simplify: R cells along the longest side of the mesh")
    small.add_argument("--target_faces", type=int, default=None, metavar="N", help="simplify: the finest grid found that leaves at most N faces")
    ap.add_argument("--smooth", type=int, default=0, metavar="N",
                    help="smooth the mesh before writing it: N Taubin iterations with the boundary fixed (ngp_hip.smooth_mesh); 0: off")
    ap.add_argument("--smooth_max_move", type=float, default=0.5, metavar="CELLS",
                    help="smoothing moves no coordinate farther than this many spacings of the extraction grid")
    ap.add_argument("--colors", default="none", choices=["none", "field", "images"],
                    help="vertex colours for the final mesh of the procedural scene: the model's colour at the vertices "
                         "(ngp_hip.bake_field_colors) or baked from --views posed views of the scene (ngp_hip.bake_image_colors)")
    ap.add_argument("--views", type=int, default=40, metavar="N", help="--colors images: the number of views to bake from")
    ap.add_argument("--field_offset", type=float, default=-2.0, metavar="CELLS",
                    help="--colors field: ask the model this many spacings of the extraction grid along the normal (negative: inside)")
    ap.add_argument("--scale", type=float, default=0.5)
    # the --sdf fit (fit_sdf_eikonal.py's options); --max_res also sizes the NGP of --ckpt
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--log2_T", type=int, default=19)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--max_res", type=float, default=None)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--eikonal_weight", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this example needs the GPU: libngp_hip has no CPU path")
    if not args.out.endswith((".ply", ".obj")):
        raise SystemExit("--out must end in .ply or .obj")
    dev = torch.device("cuda")
    from ngp_hip import mesh
    normals = None if args.normals == "none" else args.normals
    info = {}
    t0 = time.time()
    if args.sdf:
        if normals == "analytic":
            raise SystemExit("--normals analytic needs a model (--train_steps or --ckpt)")
        if args.max_res is None:
            args.max_res = 2048.0
        fn, last = fit_sphere_sdf(args, dev)
        info.update(mode="sdf", fit_steps=args.steps, sdf_loss_last=last)
        torch.cuda.synchronize()
        t1 = time.time()
        msh, grid = mesh.extract_mesh(fn, args.resolution, 0.0 if args.threshold is None else args.threshold,
                                      bounds=((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), normals=normals, sign=-1, return_grid=True)
        cell = [1.0 / args.resolution] * 3
    else:
        from modules.networks import NGP
        from modules.rendering import MAX_SAMPLES
        thr = 0.01 * MAX_SAMPLES / 3**0.5 if args.threshold is None else args.threshold
        if args.ckpt:
            model = NGP(scale=args.scale, max_res=1024 if args.max_res is None else int(args.max_res)).to(dev)
            sd = torch.load(args.ckpt, map_location=dev)
            sd = sd.get("state_dict", sd)
            model.load_state_dict({k[6:] if k.startswith("model.") else k: v for k, v in sd.items()})
            info.update(mode="ckpt")
        else:
            model, _ = train_procedural_model(args.train_steps, dev)
            info.update(mode="procedural scene", train_steps=args.train_steps)
        model.eval()
        torch.cuda.synchronize()
        t1 = time.time()
        with torch.autocast("cuda", dtype=torch.float16):                  # the evaluation loops' numerics: density runs the fused kernels
            msh, grid = mesh.extract_mesh(model, args.resolution, thr, normals=normals, return_grid=True)
        info.update(threshold=thr)
        cell = mesh.grid_spacing(model.xyz_min.reshape(3).tolist(), model.xyz_max.reshape(3).tolist(), args.resolution)[1]
    torch.cuda.synchronize()
    t2 = time.time()
    if args.keep_largest is not None or args.min_component_faces > 0:        # off by default: the output is then what it always was
        before = mesh.topology(msh)
        msh, report = mesh.clean_mesh(msh, keep_largest=args.keep_largest, min_faces=args.min_component_faces)
        torch.cuda.synchronize()
        report.pop("kept")
        info.update(clean=dict(report, before=before, seconds=time.time() - t2))
        print("clean_mesh:", json.dumps(info["clean"]))
        print("topology before:", json.dumps(before), "after:", json.dumps(mesh.topology(msh)))
    if args.smooth > 0:                                                      # off by default
        if not args.smooth_max_move >= 0.0:
            raise SystemExit("--smooth_max_move must be >= 0")
        torch.cuda.synchronize()
        t_smooth = time.time()
        res = mesh.smooth_mesh(msh, iterations=args.smooth, boundary="fixed", max_move=[args.smooth_max_move * c for c in cell],
                               normals=normals is not None)
        torch.cuda.synchronize()
        seconds = time.time() - t_smooth
        moved = (res.mesh.vertices - msh.vertices).abs() / torch.tensor(cell, device=dev, dtype=torch.float32)
        found = moved.numel() > 0
        report = dict(iterations=args.smooth, seconds=seconds, boundary_vertices=res.adjacency.boundary_vertices,
                      bad_faces=res.bad_faces, bad_vertices=res.bad_vertices, max_move_cells=args.smooth_max_move,
                      mean_displacement_cells=float(moved.norm(dim=1).mean()) if found else None,
                      max_displacement_cells=float(moved.max()) if found else None)
        if args.sdf:
            d0, a0 = sphere_errors(msh, cell[0])
            d1, a1 = sphere_errors(res.mesh, cell[0])
            report.update(sphere_distance_cells={"before": d0, "after": d1}, face_normal_error_degrees={"before": a0, "after": a1})
        msh = res.mesh
        info.update(smooth=report)
        print("smooth_mesh:", json.dumps(report))
    if args.simplify_cell is not None or args.simplify_resolution is not None or args.target_faces is not None:      # off by default
        t_simplify = time.time()
        before = {"vertices": int(msh.vertices.shape[0]), "faces": int(msh.faces.shape[0])}
        res = mesh.simplify_mesh(msh, cell=args.simplify_cell, resolution=args.simplify_resolution, target_faces=args.target_faces,
                                 normals=normals is not None)
        msh = res.mesh
        torch.cuda.synchronize()
        info.update(simplify=dict(vertices=int(msh.vertices.shape[0]), faces=int(msh.faces.shape[0]), before=before, cell=list(res.h),
                                  grid=list(res.grid), clusters=res.n_clusters, seconds=time.time() - t_simplify))
        print("simplify_mesh:", json.dumps(info["simplify"]))
    colors = None
    if args.colors != "none":                                                # off by default; last: colours belong to the final vertices
        if args.sdf:
            raise SystemExit("--colors needs a model of the procedural scene (--train_steps or --ckpt)")
        if args.views < 1:
            raise SystemExit("--views must be positive")
        if msh.faces.shape[0]:
            colors, report = color_mesh(args.colors, msh, model, dev, n_views=args.views, field_offset=args.field_offset * min(cell))
            info.update(colors=report)
            print("colors:", json.dumps(report))
    t_write = time.time()
    write = mesh.write_ply if args.out.endswith(".ply") else mesh.write_obj
    write(args.out, msh) if colors is None else write(args.out, msh, colors=colors)
    t3 = time.time()
    info.update(mesh.topology(msh))
    info.update(resolution=args.resolution, normals=args.normals, out=args.out, prepare_seconds=t1 - t0, extract_seconds=t2 - t1,
                write_seconds=t3 - t_write)
    if args.compare:
        from ngp_hip import surface_distance
        other = (mesh.read_ply if args.compare.endswith(".ply") else mesh.read_obj)(args.compare)
        found = msh.faces.shape[0] > 0 and other.faces.shape[0] > 0           # an empty surface has no distance: null
        info.update(compare=args.compare,
                    surface_distance=surface_distance(msh, other, 65536, torch.Generator().manual_seed(args.seed)) if found else None)
    print(json.dumps(info))
    info.update(mesh=msh, grid=grid)
    return info


if __name__ == "__main__":
    main()
