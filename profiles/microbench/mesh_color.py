"""Time of the vertex-colour bake (csrc/mesh_color.hip + the any-hit ray cast of csrc/mesh_raycast.hip) on the MI355X, recorded in
profiles/mesh_color.json.

    python profiles/microbench/mesh_color.py --out profiles/mesh_color.json

Two meshes: the marching-tetrahedra sphere of profiles/microbench/mesh_extract.py (257^3 points, about 333 k vertices) and the mesh of an
NGP trained on the procedural scene with examples/extract_mesh.py's schedule.  100 views of 400 x 400 from cameras of the example's kind.
The images of the timed runs hold a smooth function of the pixel: what a texel holds does not change the time.  The cameras are cut
into the chunks bake_image_colors itself would cut them into (256 MiB of per-pair buffers); per stage -- project, the any-hit ray cast,
accumulate -- the time is that of ALL chunks, each stage run over the stored outputs of the one before, warmed, then timed with HIP
events: minimum and median.  The fill is eight rounds over the adjacency, the finish launch and the whole bake_image_colors call (with a
MeshSDF at hand, so without host work) are timed too.
The same contract as a torch composition, per camera: the projection in torch, MeshSDF.visible for the segment, grid_sample for the
bilinear lookup, a masked add into float64 sums.
Last, examples/extract_mesh.py's color_mesh on the procedural-scene mesh: the PSNR of --colors field (at the example's default offset of
-2 cells along the normal, and at four other offsets) and --colors images on held-out views."""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUNDS = 20
WH = 400
VIEWS = 100


def timed(fn, rounds=ROUNDS, warm=3):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return {"min_us": min(us), "median_us": float(np.median(us)), "max_us": max(us)}


def smooth_images(n, wh, dev):
    j, y, x, c = torch.meshgrid(torch.arange(n, device=dev), torch.arange(wh, device=dev), torch.arange(wh, device=dev),
                                torch.arange(3, device=dev), indexing="ij")
    return (0.5 + 0.45 * torch.sin(0.037 * x * (c + 1) + 0.023 * y + 1.3 * j + c)).float().contiguous()


def torch_bake(mesh, target, normals, images, K, c2w, eps, cos_min=0.1, near=1e-6):
    """The contract as a torch composition, a camera at a time -> (colors, weight, views)."""
    v = mesh.vertices
    n_v, (h, w) = v.shape[0], images.shape[1:3]
    acc = torch.zeros(n_v, 4, device=v.device, dtype=torch.float64)
    views = torch.zeros(n_v, device=v.device, dtype=torch.int32)
    o = v + eps * normals
    for j in range(c2w.shape[0]):
        c, rot = c2w[j, :, 3], c2w[j, :, :3]
        d = c - v
        cos = (normals * d).sum(1) / torch.linalg.norm(d, dim=1)
        p = (v - c) @ rot
        a = K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2] - 0.5
        b = K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2] - 0.5
        ok = (cos > cos_min) & (p[:, 2] > near) & (a >= 0) & (a <= w - 1) & (b >= 0) & (b <= h - 1)
        ok &= target.visible(o, c.expand_as(o).contiguous(), eps=0.0)
        grid = torch.stack([(a + 0.5) / w * 2 - 1, (b + 0.5) / h * 2 - 1], -1).view(1, 1, n_v, 2)
        rgb = torch.nn.functional.grid_sample(images[j].permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="border", align_corners=False)
        wgt = torch.where(ok, cos * cos, torch.zeros_like(cos)).double()
        acc[:, :3] += wgt[:, None] * rgb[0, :, 0].T.double()
        acc[:, 3] += wgt
        views += ok
    return (acc[:, :3] / acc[:, 3:].clamp_min(1e-300)).float(), acc[:, 3].float(), views


def measure(name, mesh, dev, example):
    from ngp_hip import MeshSDF, bake_image_colors, ops, vertex_normals
    n_v, n_f = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    focal = 1111.1 * WH / 800
    K = torch.tensor([[focal, 0, WH / 2], [0, focal, WH / 2], [0, 0, 1]], device=dev)
    c2w = example._cameras(VIEWS, 1.39, 41, dev).contiguous()
    images = smooth_images(VIEWS, WH, dev)
    normals = mesh.normals if mesh.normals is not None else vertex_normals(mesh)
    target = MeshSDF.from_mesh(mesh, signed=False)
    eps = (1e-3 * torch.linalg.norm(target.hi - target.lo)).reshape(1).float()
    per_chunk = max(1, min(VIEWS, (256 << 20) // (ops.MESH_COLOR_PAIR_BYTES * n_v)))
    chunks = [(n0, min(n0 + per_chunk, VIEWS)) for n0 in range(0, VIEWS, per_chunk)]
    project = lambda: [ops.mesh_color_project(mesh.vertices, normals, K, c2w[a:b], (WH, WH), eps) for a, b in chunks]
    pairs = project()
    cast = lambda: [target.raycast(p[0], p[1], t_min=0.0, t_max=1.0, any_hit=True, details=False).t for p in pairs]
    ts = cast()
    accum = torch.zeros(n_v, 4, device=dev, dtype=torch.float64)
    views = torch.zeros(n_v, device=dev, dtype=torch.int32)

    def accumulate():
        accum.zero_(); views.zero_()
        for (a, b), p, t in zip(chunks, pairs, ts):
            ops.mesh_color_accumulate(images[a:b], p[2], p[3], p[4], t, accum, views)
    accumulate()
    colors, weight, filled = ops.mesh_color_finish(accum, views)
    row_start, neighbours = ops.mesh_adjacency(mesh.vertices, mesh.faces)[:2]
    accepted = sum(int((p[3] > 0).sum()) for p in pairs)
    counted = sum(int(((p[3] > 0) & torch.isinf(t)).sum()) for p, t in zip(pairs, ts))
    out = {"vertices": n_v, "faces": n_f, "views": VIEWS, "image_wh": WH, "pairs": n_v * VIEWS, "accepted_pairs": accepted, "counted_pairs": counted,
           "cameras_per_chunk": per_chunk, "chunks": len(chunks), "vertices_without_a_view": int((filled == 255).sum()),
           "project": timed(project), "raycast_any_hit": timed(cast), "accumulate": timed(accumulate),
           "finish": timed(lambda: ops.mesh_color_finish(accum, views)),
           "fill_8_rounds": timed(lambda: ops.mesh_color_fill(colors.clone(), filled.clone(), row_start, neighbours, 8)),
           "bake_image_colors": timed(lambda: bake_image_colors(mesh, images, K, c2w, normals=normals, target=target), rounds=5, warm=1),
           "torch_composition": timed(lambda: torch_bake(mesh, target, normals, images, K, c2w, eps), rounds=3, warm=1)}
    out["rays_per_second_all_pairs"] = n_v * VIEWS / (out["raycast_any_hit"]["min_us"] * 1e-6)
    out["rays_per_second_accepted_pairs"] = accepted / (out["raycast_any_hit"]["min_us"] * 1e-6)
    ours = bake_image_colors(mesh, images, K, c2w, normals=normals, target=target, fill_rounds=0)
    theirs = torch_bake(mesh, target, normals, images, K, c2w, eps)
    both = (ours.views > 0) & (theirs[2] == ours.views)
    out["torch_composition_agreement"] = {"vertices_with_the_same_views": int((theirs[2] == ours.views).sum()),
                                          "max_colour_difference_there": float((ours.colors - theirs[0])[both].abs().max()) if bool(both.any()) else None}
    stages = out["project"]["min_us"] + out["raycast_any_hit"]["min_us"] + out["accumulate"]["min_us"]
    print("%s: V=%d T=%d, %d views: project %.0f us, any-hit ray cast %.0f us (%.0f M segments/s over all pairs, %.0f M/s over the %d accepted), "
          "accumulate %.0f us, fill %.0f us; bake_image_colors %.0f us; torch composition %.0f us (%.1f x)"
          % (name, n_v, n_f, VIEWS, out["project"]["min_us"], out["raycast_any_hit"]["min_us"], out["rays_per_second_all_pairs"] / 1e6,
             out["rays_per_second_accepted_pairs"] / 1e6, accepted, out["accumulate"]["min_us"], out["fill_8_rounds"]["min_us"],
             out["bake_image_colors"]["min_us"], out["torch_composition"]["min_us"], out["torch_composition"]["min_us"] / out["bake_image_colors"]["min_us"]))
    out["three_stages_min_us"] = stages
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_color.json"))
    ap.add_argument("--resolution", type=int, default=256, help="cells per axis of both extractions")
    ap.add_argument("--train_steps", type=int, default=500)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernels' time")
    dev = torch.device("cuda")
    from ngp_hip import mesh
    spec = importlib.util.spec_from_file_location("extract_mesh_example", os.path.join(ROOT, "examples", "extract_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res = args.resolution
    out = {"what": "vertex colours from %d views of %d x %d: ngp_mesh_color_project / ngp_mesh_raycast (any hit, t in [0, 1]) / "
                   "ngp_mesh_color_accumulate over all chunks, HIP events, %d rounds after 3 warm ones" % (VIEWS, WH, WH, ROUNDS),
           "pair_bytes": 44, "workspace_bytes": 256 << 20}
    # the sphere of mesh_extract.py, moved to the origin so that the example's cameras look at it
    sdf = lambda x: torch.linalg.norm(x - torch.tensor([0.0, -0.03, 0.02], device=x.device), dim=1) - 0.3
    sphere = mesh.extract_mesh(sdf, res, 0.0, bounds=((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), sign=-1, device=dev)
    out["sphere"] = measure("sphere", sphere, dev, ex)
    del sphere
    model, thr = ex.train_procedural_model(args.train_steps, dev)
    model.eval()
    with torch.autocast("cuda", dtype=torch.float16):
        scene = mesh.extract_mesh(model, res, thr)
    scene, _ = mesh.clean_mesh(scene)                                       # nothing dropped but bad faces and unused vertices
    out["procedural_scene"] = measure("procedural scene", scene, dev, ex)
    out["procedural_scene"].update(train_steps=args.train_steps, threshold=thr)
    out["example_psnr"] = {"field_by_offset_cells": {}}
    for cells in (0.0, -0.5, -1.0, -2.0, -4.0):                                # the example's default is -2
        _, report = ex.color_mesh("field", scene, model, dev, field_offset=cells / res)
        out["example_psnr"]["field_by_offset_cells"]["%g" % cells] = report["psnr"]
        if cells == -2.0:
            out["example_psnr"]["field"] = report
    _, out["example_psnr"]["images"] = ex.color_mesh("images", scene, model, dev, n_views=40)
    for how in ("field", "images"):
        print("example --colors %s: %s" % (how, json.dumps(out["example_psnr"][how])))
    print("field PSNR by offset in cells:", json.dumps(out["example_psnr"]["field_by_offset_cells"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
