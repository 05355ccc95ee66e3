"""Distance to a triangle mesh (csrc/mesh_sdf.hip): build and query times, the walk's work per point, and a chunked torch brute force.

    python profiles/microbench/mesh_sdf.py [--out profiles/mesh_sdf.json]

Meshes: the sphere (radius 0.3 in the unit box) extracted by marching tetrahedra on 65^3 and 257^3 grid points.  Queries: 16 384 and
1 048 576 points, uniform in the box and near the surface (sigma 0.01), each in random order and sorted by Morton code.  Every time is
the median (and the minimum) of --reps launches after two warm-up launches, by device events, all in this one process.
The brute force (every point against every face, the kernel's formula in torch, float32, chunked) runs on the 65^3 mesh only; for
the 257^3 mesh its cost is stated by arithmetic from the measured pair rate.
nodes / faces per point come from a second build of mesh_sdf.hip alone with -DNGP_MESH_TREE_COUNT (two atomic counters, compiled here
into a temporary directory; the product library has no counters).  "bytes" is arithmetic on those counters -- 24 per box tested,
4 + 12 + 36 per face evaluated, 12 + 36 per point in and out -- i.e. the bytes REQUESTED, most of which the caches serve; the share of
the 8 TB/s HBM roofline it would be if none were cached is given for orientation."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM = 8.0e12


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


def brute_force(x, tri, chunk_pairs=2**26):
    """min over faces of the point-triangle distance, the kernel's Voronoi-region formula in float32 torch, `chunk_pairs` pairs a time."""
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    ab, ac = b - a, c - a
    out = torch.empty(x.shape[0], device=x.device)
    step = max(chunk_pairs // tri.shape[0], 1)
    dot = lambda u, v: (u * v).sum(-1)
    for s in range(0, x.shape[0], step):
        p = x[s:s + step, None, :]
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = 1.0 / (va + vb + vc)
        v, w = vb * den, vc * den
        zero, one = torch.zeros_like(v), torch.ones_like(v)
        for cond, vn, wn in (((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 1 - (d4 - d3) / ((d4 - d3) + (d5 - d6)), (d4 - d3) / ((d4 - d3) + (d5 - d6))),
                             ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)), ((d6 >= 0) & (d5 <= d6), zero, one),
                             ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero), ((d3 >= 0) & (d4 <= d3), one, zero),
                             ((d1 <= 0) & (d2 <= 0), zero, zero)):
            v, w = torch.where(cond, vn, v), torch.where(cond, wn, w)
        r = ap - (ab * v[..., None] + ac * w[..., None])
        out[s:s + step] = dot(r, r).nan_to_num(nan=float("inf")).min(1).values.sqrt()
    return out


def counting_library(tmp):
    """mesh_sdf.hip alone with the two counters, bound by hand (the product header does not declare the counter entry).  -Bsymbolic: its
    launches must reach its own kernels, not the equally named ones of the product library loaded before it."""
    from ngp_hip import lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    path = os.path.join(tmp, "libmesh_sdf_count.so")
    subprocess.run([hipcc] + lib.HIPCC_FLAGS + ["-DNGP_MESH_TREE_COUNT", "-Wl,-Bsymbolic", "-o", path, os.path.join(lib.CSRC, "mesh_sdf.hip")], check=True)
    so = ctypes.CDLL(path)
    so.ngp_mesh_sdf_query.argtypes = lib.SIGNATURES["ngp_mesh_sdf_query"]
    so.ngp_mesh_sdf_counters.argtypes = [ctypes.c_void_p]
    return so


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sdf.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--grids", type=int, nargs="+", default=[65, 257])
    ap.add_argument("--no_counters", action="store_true")
    args = ap.parse_args(argv)
    from ngp_hip import MeshSDF, mesh_sdf, ops
    from ngp_hip.mesh import extract_mesh
    dev = torch.device("cuda")
    sphere = lambda x: torch.linalg.norm(x - 0.5, dim=1) - 0.3
    tmp = tempfile.mkdtemp()
    counting = None if args.no_counters else counting_library(tmp)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "leaf_size": 4, "meshes": []}
    pair_rate = None
    for grid in args.grids:
        m = extract_mesh(sphere, grid - 1, 0.0, bounds=((0, 0, 0), (1, 1, 1)), sign=-1, normals=None, device=dev)
        host = (m.vertices.cpu(), m.faces.cpu())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        target = MeshSDF(*host)
        torch.cuda.synchronize()
        construct_s = time.perf_counter() - t0
        order_s = timed(lambda: mesh_sdf.morton_order(target.vertices[target.faces.long()].mean(1), target.lo, target.hi), args.reps)
        build = timed(lambda: ops.mesh_bvh_build(target.vertices, target.faces, target.order, 4), args.reps)
        entry = {"grid_points": grid, "vertices": int(m.vertices.shape[0]), "faces": int(m.faces.shape[0]), "tree_nodes": int(target.boxes.shape[0]),
                 "construct_s_incl_host_pseudonormals": construct_s, "morton_sort_ms": order_s, "bvh_build_ms": build, "queries": []}
        gen = torch.Generator().manual_seed(grid)
        for n in (16384, 1 << 20):
            sets = {"uniform": torch.rand(n, 3, generator=gen).to(dev),
                    "near": target.sample(n, 0.01, 0.0, gen).contiguous()}
            for kind, x in sets.items():
                lo, hi = x.min(0).values, x.max(0).values
                for layout, pts in (("random", x), ("morton", x[mesh_sdf.morton_order(x, lo, hi)].contiguous())):
                    t = timed(lambda: target(pts), args.reps)
                    q = {"points": n, "kind": kind, "order": layout, **t, "queries_per_s": n / (t["median_ms"] * 1e-3)}
                    if counting is not None:
                        out = ops.mesh_sdf_query(pts, target.vertices, target.faces, target.order, target.boxes, 4, target.edge_normals,
                                                 target.vertex_normals)                       # shapes checked; now the counting build
                        cnt = (ctypes.c_ulonglong * 2)()
                        counting.ngp_mesh_sdf_counters(cnt)
                        P = ops._ptr
                        rc = counting.ngp_mesh_sdf_query(P(pts), n, P(target.vertices), P(target.faces), P(target.order), P(target.boxes),
                                                         target.n_faces, 4, P(target.edge_normals), P(target.vertex_normals), P(out[0]), P(out[1]),
                                                         P(out[2]), P(out[3]), ops._stream())
                        torch.cuda.synchronize()
                        counting.ngp_mesh_sdf_counters(cnt)
                        assert rc == 0
                        nodes, faces = cnt[0] / n, cnt[1] / n
                        req = n * (24 * nodes + 52 * faces + 48)
                        q.update(nodes_per_point=nodes, faces_per_point=faces, bytes_requested=req,
                                 requested_GBps=req / (t["median_ms"] * 1e-3) / 1e9,
                                 share_of_8TBps_if_uncached=req / (t["median_ms"] * 1e-3) / HBM)
                    entry["queries"].append(q)
                    if grid == args.grids[0] and n == 16384:
                        tri = target.vertices[target.faces.long()]
                        bt = timed(lambda: brute_force(pts, tri), max(args.reps // 2, 3))
                        got = target(pts).sdf.abs()
                        q["brute_force"] = {**bt, "max_abs_difference": float((brute_force(pts, tri) - got).abs().max()),
                                            "speedup_median": bt["median_ms"] / t["median_ms"]}
                        pair_rate = n * tri.shape[0] / (bt["median_ms"] * 1e-3)
        result["meshes"].append(entry)
    if pair_rate is not None and len(result["meshes"]) > 1:
        big = result["meshes"][-1]
        result["brute_force_on_the_large_mesh_BY_ARITHMETIC"] = {
            "pairs_per_s_measured_on_the_small_mesh": pair_rate,
            "seconds_for_16384_points": 16384 * big["faces"] / pair_rate, "seconds_for_1048576_points": (1 << 20) * big["faces"] / pair_rate}
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
