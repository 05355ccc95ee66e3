"""Time of the marching-tetrahedra kernels (csrc/mesh.hip) on the MI355X, recorded in profiles/mesh_extract.json.

    python profiles/microbench/mesh_extract.py --out profiles/mesh_extract.json
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o mesh -- python profiles/microbench/mesh_extract.py --loop 20     # a run of its own

Two 257^3 grids: the analytic signed distance of a sphere (iso 0, sign -1) and the density of an NGP trained on the procedural scene with
examples/extract_mesh.py's schedule, sampled by sample_grid under fp16 autocast (iso = the occupancy threshold, sign +1).  ngp_mesh_count
(count + scan) and ngp_mesh_emit with and without normals are warmed, then timed with HIP events, 20 rounds: minimum and median.  In the
same process the time sample_grid(model.density) takes for those 257^3 points is recorded -- existing kernels, the price a user already
pays for the grid -- and the relation to check is count + emit < that evaluation.

Algorithmic bytes: count reads 4 B per point and writes the 4 B per point of workspace; emit reads that workspace again (mask, triangle
count and, where a vertex is looked up, the rank) and writes 12 B per vertex (24 B with normals) and 12 B per face.  The value re-reads
of emit are sparse (points with a vertex, cells with a face) and are not counted.  The share of 8 TB/s is those bytes over the time."""
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
HBM_BYTES_PER_S = 8e12
WORKSPACE_BYTES_PER_POINT = 4


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


def sphere_grid(res, dev):
    from ngp_hip import mesh
    sdf = lambda x: torch.linalg.norm(x - torch.tensor([0.5, 0.47, 0.52], device=x.device), dim=1) - 0.3
    return mesh.sample_grid(sdf, (0, 0, 0), (1, 1, 1), res, device=dev), (0.0, 0.0, 0.0), (1.0 / res,) * 3


def measure(values, iso, sign, lo, h):
    from ngp_hip import ops
    n = values.numel()
    workspace, counts = ops.mesh_count(values, iso, sign)
    V, T = counts.tolist()
    out = {"points": n, "vertices": V, "faces": T,
           "count": timed(lambda: ops.mesh_count(values, iso, sign, workspace=workspace)),
           "emit_with_normals": timed(lambda: ops.mesh_emit(values, iso, sign, lo, h, workspace, V, T, normals=True)),
           "emit_without_normals": timed(lambda: ops.mesh_emit(values, iso, sign, lo, h, workspace, V, T, normals=False))}
    byts = {"count": n * (4 + WORKSPACE_BYTES_PER_POINT),
            "emit_with_normals": n * WORKSPACE_BYTES_PER_POINT + 24 * V + 12 * T,
            "emit_without_normals": n * WORKSPACE_BYTES_PER_POINT + 12 * V + 12 * T}
    for k, b in byts.items():
        out[k]["algorithmic_bytes"] = b
        out[k]["share_of_8TB_per_s"] = b / (out[k]["min_us"] * 1e-6) / HBM_BYTES_PER_S
    out["count_plus_emit_with_normals_min_us"] = out["count"]["min_us"] + out["emit_with_normals"]["min_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_extract.json"))
    ap.add_argument("--resolution", type=int, default=256, help="cells per axis: 257^3 points")
    ap.add_argument("--train_steps", type=int, default=500)
    ap.add_argument("--loop", type=int, default=0, help="only run count + emit on the sphere grid this many times (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernels' time")
    dev = torch.device("cuda")
    from ngp_hip import mesh, ops
    res = args.resolution
    values, lo, h = sphere_grid(res, dev)
    if args.loop:
        for _ in range(args.loop):
            workspace, counts = ops.mesh_count(values, 0.0, -1)
            V, T = counts.tolist()
            ops.mesh_emit(values, 0.0, -1, lo, h, workspace, V, T, normals=True)
        torch.cuda.synchronize()
        print(json.dumps({"loop": args.loop, "points": values.numel(), "vertices": V, "faces": T}))
        return
    out = {"what": "ngp_mesh_count / ngp_mesh_emit on %d^3 points, HIP events, %d rounds after 3 warm ones; the density evaluation of the same "
                   "grid (sample_grid(model.density), fp16 autocast, existing kernels) in the same process" % (res + 1, ROUNDS),
           "workspace_bytes_per_point": WORKSPACE_BYTES_PER_POINT,
           "workspace_bytes": int(ops._lib().ngp_mesh_workspace_bytes(res + 1, res + 1, res + 1)),
           "sphere_sdf": measure(values, 0.0, -1, lo, h)}
    del values
    spec = importlib.util.spec_from_file_location("extract_mesh_example", os.path.join(ROOT, "examples", "extract_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    model, thr = ex.train_procedural_model(args.train_steps, dev)
    model.eval()
    b = (model.xyz_min.reshape(3).tolist(), model.xyz_max.reshape(3).tolist())
    lo, h = mesh.grid_spacing(b[0], b[1], res)
    with torch.autocast("cuda", dtype=torch.float16):
        grid = mesh.sample_grid(model.density, b[0], b[1], res, device=dev)
        evaluation = timed(lambda: mesh.sample_grid(model.density, b[0], b[1], res, device=dev), rounds=5, warm=1)
    out["procedural_scene_density"] = measure(grid, thr, +1, lo, h)
    out["procedural_scene_density"].update(train_steps=args.train_steps, threshold=thr, density_evaluation=evaluation)
    for k in ("sphere_sdf", "procedural_scene_density"):
        out[k]["count_plus_emit_over_density_evaluation"] = out[k]["count_plus_emit_with_normals_min_us"] / evaluation["min_us"]
        print("%s: V=%d T=%d count %.1f us, emit %.1f us (%.1f us without normals); density evaluation %.1f us"
              % (k, out[k]["vertices"], out[k]["faces"], out[k]["count"]["min_us"], out[k]["emit_with_normals"]["min_us"],
                 out[k]["emit_without_normals"]["min_us"], evaluation["min_us"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
