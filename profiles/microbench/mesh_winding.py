"""Generalized winding numbers (csrc/mesh_winding.hip): launch times, the walk's work per point, the kernels' resources, the reference's
approximation figures, and three comparisons.

    python profiles/microbench/mesh_winding.py [--out profiles/mesh_winding.json]

Meshes: the sphere (radius 0.3 in the unit box) extracted by marching tetrahedra on 65^3 and 257^3 grid points, the two meshes of
profiles/microbench/mesh_sdf.py and mesh_raycast.py.  Points: MeshSDF.sample(n, sigma 0.01, no uniform share), 16 384 and 2^20 of them.
Every time is the median (and the minimum) of --reps launches after two warm-up launches, by device events, all in this one process.
  moments_build        ngp_mesh_winding_build over the finished tree (one launch per level)
  queries              beta = 2 with 1 and 2 far-field terms; nodes / accepted nodes / faces per point from a second build of
                       mesh_winding.hip alone with -DNGP_MESH_TREE_COUNT (three atomic counters, compiled here into a temporary directory
                       or given with --counting_lib; the product library has no counters)
Comparisons at 16 384 points, each labelled with what it is:
  exact_sum_through_the_tree      the kernel's own beta = inf mode: every face, the built-in brute force
  brute_force_torch               every point against every face, the same formula in float32 torch, chunked (the 65^3 mesh only)
  closest_point_query_same_points MeshSDF.__call__ (csrc/mesh_sdf.hip) on the same points: the other point query of the same tree
kernel_resources: VGPRs, scratch and occupancy of the four kernels as hipcc -Rpass-analysis=kernel-resource-usage reports them (a
cross-compile; needs no GPU: --resources_only prints just these and the reference's figures).
reference_beta2: per named set of tests/mesh_winding_reference.py and number of far-field terms, A_set = max |tree64 - exact|, its mean,
E32, the undecided fraction and the terms per point, in float64 on the host."""
import argparse
import ctypes
import json
import math
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(times), "min_ms": min(times)}


def brute_force(x, tri, chunk_pairs=2**24):
    """w [n]: the kernel's formula in float32 torch over every (point, face) pair, `chunk_pairs` pairs a time."""
    out = torch.empty(x.shape[0], device=x.device)
    step = max(chunk_pairs // tri.shape[0], 1)
    dot = lambda u, v: (u * v).sum(-1)
    for s in range(0, x.shape[0], step):
        q = x[s:s + step, None, :]
        a, b, c = tri[None, :, 0] - q, tri[None, :, 1] - q, tri[None, :, 2] - q
        la, lb, lc = torch.linalg.norm(a, dim=-1), torch.linalg.norm(b, dim=-1), torch.linalg.norm(c, dim=-1)
        num = dot(a, torch.cross(b, c, dim=-1))
        den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
        out[s:s + step] = (2.0 * torch.atan2(num, den)).sum(1) / (4.0 * math.pi)
    return out


def counting_library(tmp, prebuilt=None):
    """mesh_winding.hip alone with the three counters, bound by hand (the product header does not declare the counter entry).
    -Bsymbolic: its launches must reach its own kernels, not the equally named ones of the product library loaded before it."""
    from ngp_hip import lib
    path = prebuilt
    if path is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        path = os.path.join(tmp, "libmesh_winding_count.so")
        subprocess.run([hipcc] + lib.HIPCC_FLAGS + ["-DNGP_MESH_TREE_COUNT", "-Wl,-Bsymbolic", "-o", path, os.path.join(lib.CSRC, "mesh_winding.hip")],
                       check=True)
    so = ctypes.CDLL(path)
    so.ngp_mesh_winding_query.argtypes = lib.SIGNATURES["ngp_mesh_winding_query"]
    so.ngp_mesh_winding_counters.argtypes = [ctypes.c_void_p]
    return so


def kernel_resources(tmp):
    """{kernel: {vgprs, sgprs, scratch_bytes_per_lane, occupancy_waves_per_simd, lds_bytes}} from the compiler's remarks."""
    from ngp_hip import lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    res = subprocess.run([hipcc] + lib.HIPCC_FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "libres.so"),
                                                      os.path.join(lib.CSRC, "mesh_winding.hip")], capture_output=True, text=True, check=True)
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd",
            "LDS Size [bytes/block]": "lds_bytes"}
    for line in res.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            mangled = m.group(1)
            order = re.search(r"query_kernelILi(\d)E", mangled)
            name = re.search(r"mesh_winding_[a-z]+_kernel", mangled).group(0) + ("<%s>" % order.group(1) if order else "")
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and name and m.group(1) in keys:
            out[name][keys[m.group(1)]] = int(m.group(2))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_winding.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--grids", type=int, nargs="+", default=[65, 257])
    ap.add_argument("--no_counters", action="store_true")
    ap.add_argument("--no_reference", action="store_true", help="leave out the host-side figures of tests/mesh_winding_reference.py")
    ap.add_argument("--resources_only", action="store_true", help="no GPU: only kernel_resources and reference_beta2")
    ap.add_argument("--counting_lib", default=None, help="a prebuilt -DNGP_MESH_TREE_COUNT build of mesh_winding.hip")
    args = ap.parse_args(argv)
    tmp = tempfile.mkdtemp()
    result = {"kernel_resources": kernel_resources(tmp)}
    if not args.no_reference:
        import mesh_winding_reference as W
        result["reference_beta2"] = W.figures(2.0)
    if args.resources_only:
        print(json.dumps(result))
        return result
    from ngp_hip import MeshSDF, ops
    from ngp_hip.mesh import extract_mesh
    dev = torch.device("cuda")
    sphere = lambda x: torch.linalg.norm(x - 0.5, dim=1) - 0.3
    counting = None if args.no_counters else counting_library(tmp, args.counting_lib)
    result.update({"device": torch.cuda.get_device_name(0), "reps": args.reps, "leaf_size": 4, "meshes": []})
    for grid in args.grids:
        m = extract_mesh(sphere, grid - 1, 0.0, bounds=((0, 0, 0), (1, 1, 1)), sign=-1, normals=None, device=dev)
        target = MeshSDF(m.vertices.cpu(), m.faces.cpu(), signed=False)
        mesh = (target.vertices, target.faces, target.order)
        entry = {"grid_points": grid, "faces": int(m.faces.shape[0]), "tree_nodes": int(target.boxes.shape[0]),
                 "moments_bytes": int(target.moments.numel() * 4),
                 "moments_build": timed(lambda: ops.mesh_winding_build(*mesh, target.boxes, 4), args.reps),
                 "boxes_build": timed(lambda: ops.mesh_bvh_build(*mesh, 4), args.reps), "queries": []}
        for n in (16384, 2**20):
            x = target.sample(n, 0.01, 0.0, torch.Generator().manual_seed(n)).contiguous()
            exact = target.winding(x, beta=float("inf")) if n == 16384 else None
            for terms in (1, 2):
                t = timed(lambda: target.winding(x, beta=2.0, order=terms), args.reps)
                q = {"points": n, "beta": 2.0, "order": terms, **t, "points_per_s": n / (t["median_ms"] * 1e-3)}
                w = target.winding(x, beta=2.0, order=terms)
                if exact is not None:
                    q.update(max_abs_difference_from_exact_sum=float((w - exact).abs().max()), mean_abs_difference_from_exact_sum=float((w - exact).abs().mean()))
                if counting is not None:
                    cnt = (ctypes.c_ulonglong * 3)()
                    counting.ngp_mesh_winding_counters(cnt)
                    P = ops._ptr
                    rc = counting.ngp_mesh_winding_query(P(x), n, P(target.vertices), P(target.faces), P(target.order), P(target.moments), target.n_faces,
                                                         4, 2.0, terms, P(w), ops._stream())
                    torch.cuda.synchronize()
                    counting.ngp_mesh_winding_counters(cnt)
                    assert rc == 0
                    q.update(nodes_per_point=cnt[0] / n, accepted_per_point=cnt[1] / n, faces_per_point=cnt[2] / n)
                entry["queries"].append(q)
            if n == 16384:
                fast = timed(lambda: target.winding(x), args.reps)
                reps = max(args.reps // 2, 3)
                entry["exact_sum_through_the_tree"] = {**timed(lambda: target.winding(x, beta=float("inf")), reps), "points": n,
                                                       "beta2_order2_median_ms": fast["median_ms"]}
                entry["exact_sum_through_the_tree"]["speedup_median"] = entry["exact_sum_through_the_tree"]["median_ms"] / fast["median_ms"]
                entry["closest_point_query_same_points"] = {**timed(lambda: target(x, details=False), args.reps), "points": n,
                                                            "beta2_order2_median_ms": fast["median_ms"]}
                if grid == args.grids[0]:
                    tri = target.vertices[target.faces.long()]
                    bt = timed(lambda: brute_force(x, tri), reps)
                    entry["brute_force_torch"] = {**bt, "points": n, "speedup_median": bt["median_ms"] / fast["median_ms"],
                                                  "max_abs_difference_from_exact_sum": float((brute_force(x, tri) - exact).abs().max())}
        result["meshes"].append(entry)
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
