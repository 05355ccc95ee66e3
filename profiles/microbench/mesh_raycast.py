"""Ray casting against a triangle mesh (csrc/mesh_raycast.hip): launch times, the walk's work per ray, and two comparisons.

    python profiles/microbench/mesh_raycast.py [--out profiles/mesh_raycast.json]

Meshes: the sphere (radius 0.3 in the unit box) extracted by marching tetrahedra on 65^3 and 257^3 grid points, the two meshes of
profiles/microbench/mesh_sdf.py.  Rays: the 800 x 800 primary rays of a camera 1.5 from the centre that sees the whole mesh (about a
fifth of them hit), unit directions, and 16 384 of them drawn at random; first hit and any hit, with and without the details.  Every
time is the median (and the minimum) of --reps launches after two warm-up launches, by device events, all in this one process.
boxes / faces per ray come from a second build of mesh_raycast.hip alone with -DNGP_MESH_TREE_COUNT (two atomic counters, compiled
here into a temporary directory or given with --counting_lib; the product library has no counters).
Comparisons on the 65^3 mesh at 16 384 rays, each labelled with what it is:
  brute_force_torch_moller_trumbore   every ray against every face, plain Moller-Trumbore in float32 torch, chunked: not watertight, not
                                      the kernel's formula -- the obvious way to do without a hierarchy
  closest_point_query_same_count      MeshSDF.__call__ (csrc/mesh_sdf.hip) on as many points (the rays' hit points, or points near the
                                      surface for the misses): the other walk of the same tree"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
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


def brute_force(o, d, tri, chunk_pairs=2**25):
    """min over faces of the Moller-Trumbore t (float32 torch), `chunk_pairs` pairs a time -> t [n], +inf on a miss."""
    a, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    out = torch.empty(o.shape[0], device=o.device)
    step = max(chunk_pairs // tri.shape[0], 1)
    dot = lambda u, v: (u * v).sum(-1)
    for s in range(0, o.shape[0], step):
        oo, dd = o[s:s + step, None, :], d[s:s + step, None, :]
        p = torch.cross(dd.expand(-1, tri.shape[0], -1), e2.expand(dd.shape[0], -1, -1), dim=-1)
        det = dot(e1, p)
        inv = 1.0 / det
        tv = oo - a
        u = dot(tv, p) * inv
        q = torch.cross(tv, e1.expand_as(tv), dim=-1)
        v = dot(dd, q) * inv
        t = dot(e2, q) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
        out[s:s + step] = torch.where(ok, t, torch.full_like(t, float("inf"))).min(1).values
    return out


def counting_library(tmp, prebuilt=None):
    """mesh_raycast.hip alone with the two counters, bound by hand (the product header does not declare the counter entry).  -Bsymbolic:
    its launches must reach its own kernels, not the equally named ones of the product library loaded before it."""
    from ngp_hip import lib
    path = prebuilt
    if path is None:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        path = os.path.join(tmp, "libmesh_raycast_count.so")
        subprocess.run([hipcc] + lib.HIPCC_FLAGS + ["-DNGP_MESH_TREE_COUNT", "-Wl,-Bsymbolic", "-o", path, os.path.join(lib.CSRC, "mesh_raycast.hip")],
                       check=True)
    so = ctypes.CDLL(path)
    so.ngp_mesh_raycast.argtypes = lib.SIGNATURES["ngp_mesh_raycast"]
    so.ngp_mesh_raycast_counters.argtypes = [ctypes.c_void_p]
    return so


def camera_rays(wh, dev):
    from ngp_hip.rays import get_ray_directions, get_rays
    pos = torch.tensor([0.5 + 1.5 * 0.48, 0.5 - 1.5 * 0.64, 0.5 + 1.5 * 0.6])
    fwd = torch.nn.functional.normalize(torch.tensor([0.5, 0.5, 0.5]) - pos, dim=0)
    right = torch.nn.functional.normalize(torch.cross(fwd, torch.tensor([0.0, 0.0, 1.0]), dim=0), dim=0)
    c2w = torch.cat([torch.stack([right, torch.cross(fwd, right, dim=0), fwd], -1), pos[:, None]], -1).to(dev)
    K = torch.tensor([[1.1 * wh, 0.0, wh / 2], [0.0, 1.1 * wh, wh / 2], [0.0, 0.0, 1.0]])
    o, d = get_rays(get_ray_directions(wh, wh, K, device=dev), c2w)
    return o.contiguous(), (d / torch.linalg.norm(d, dim=1, keepdim=True)).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_raycast.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--grids", type=int, nargs="+", default=[65, 257])
    ap.add_argument("--wh", type=int, default=800)
    ap.add_argument("--no_counters", action="store_true")
    ap.add_argument("--counting_lib", default=None, help="a prebuilt -DNGP_MESH_TREE_COUNT build of mesh_raycast.hip")
    args = ap.parse_args(argv)
    from ngp_hip import MeshSDF, ops
    from ngp_hip.mesh import extract_mesh
    dev = torch.device("cuda")
    sphere = lambda x: torch.linalg.norm(x - 0.5, dim=1) - 0.3
    tmp = tempfile.mkdtemp()
    counting = None if args.no_counters else counting_library(tmp, args.counting_lib)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "leaf_size": 4, "meshes": []}
    o_all, d_all = camera_rays(args.wh, dev)
    pick = torch.randperm(o_all.shape[0], generator=torch.Generator().manual_seed(1))[:16384].to(dev)
    ray_sets = {"%dx%d primary" % (args.wh, args.wh): (o_all, d_all), "16384 of them": (o_all[pick].contiguous(), d_all[pick].contiguous())}
    for grid in args.grids:
        m = extract_mesh(sphere, grid - 1, 0.0, bounds=((0, 0, 0), (1, 1, 1)), sign=-1, normals=None, device=dev)
        target = MeshSDF(m.vertices.cpu(), m.faces.cpu(), signed=False)
        entry = {"grid_points": grid, "faces": int(m.faces.shape[0]), "tree_nodes": int(target.boxes.shape[0]), "casts": []}
        for name, (o, d) in ray_sets.items():
            n = o.shape[0]
            hit_share = float(target.raycast(o, d, details=False).hit.float().mean())
            for any_hit in (False, True):
                for details in (True, False):
                    t = timed(lambda: target.raycast(o, d, any_hit=any_hit, details=details), args.reps)
                    q = {"rays": name, "n": n, "mode": "any hit" if any_hit else "first hit", "details": details, "hit_share": hit_share, **t,
                         "rays_per_s": n / (t["median_ms"] * 1e-3)}
                    if counting is not None and details:
                        out = ops.mesh_raycast(o, d, target.vertices, target.faces, target.order, target.boxes, 4, any_hit=any_hit)   # shapes checked
                        cnt = (ctypes.c_ulonglong * 2)()
                        counting.ngp_mesh_raycast_counters(cnt)
                        P = ops._ptr
                        rc = counting.ngp_mesh_raycast(P(o), P(d), n, P(target.vertices), P(target.faces), P(target.order), P(target.boxes),
                                                       target.n_faces, 4, 0.0, float("inf"), int(any_hit), P(out[0]), P(out[1]), P(out[2]), P(out[3]),
                                                       ops._stream())
                        torch.cuda.synchronize()
                        counting.ngp_mesh_raycast_counters(cnt)
                        assert rc == 0
                        q.update(boxes_per_ray=cnt[0] / n, faces_per_ray=cnt[1] / n)
                    entry["casts"].append(q)
            if grid == args.grids[0] and n == 16384:
                first = target.raycast(o, d)
                cast = timed(lambda: target.raycast(o, d), args.reps)
                tri = target.vertices[target.faces.long()]
                bt = timed(lambda: brute_force(o, d, tri), max(args.reps // 2, 3))
                ref = brute_force(o, d, tri)
                both = first.hit & torch.isfinite(ref)
                entry["brute_force_torch_moller_trumbore"] = {
                    **bt, "rays": n, "speedup_median": bt["median_ms"] / cast["median_ms"], "rays_it_misses_that_the_kernel_hits": int((first.hit & ~torch.isfinite(ref)).sum()),
                    "rays_it_hits_that_the_kernel_misses": int((~first.hit & torch.isfinite(ref)).sum()),
                    "max_abs_t_difference": float((first.t - ref)[both].abs().max()) if bool(both.any()) else 0.0}
                x = torch.where(first.hit[:, None], first.points(o, d), target.sample(n, 0.01, 0.0, torch.Generator().manual_seed(2))).contiguous()
                entry["closest_point_query_same_count"] = {**timed(lambda: target(x), args.reps), "points": n,
                                                           "ray_cast_first_hit_median_ms": cast["median_ms"]}
        result["meshes"].append(entry)
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
