"""Time of the mesh smoothing (csrc/mesh_smooth.hip) on the MI355X, recorded in profiles/mesh_smooth.json.

    python profiles/microbench/mesh_smooth.py --out profiles/mesh_smooth.json

The two meshes of profiles/microbench/mesh_components.py, extracted at 257^3 points: the analytic sphere and the density of an NGP
trained on the procedural scene for 500 steps, the latter after clean_mesh(keep_largest=1).  HIP events around the call, 20 rounds
after 3 warm ones, minimum and median:
  adjacency_keys / adjacency_sort / adjacency_build   the three parts of ops.mesh_adjacency (the sort is torch.sort of 6 T int64 keys)
  one_pass           one smoothing pass with the bound on (x0 read), and one with the bound off
  ten_iterations     smooth_mesh's twenty passes over a precomputed adjacency, normals off
  vertex_normals     ops.mesh_vertex_normals with its stable sort of 3 T keys, and that sort alone
beside a torch composition of the same contract on the same device (directed edge list -> unique -> index_add_ in float64 per pass;
index_add_ of the area vectors for the normals): what a user would write today.  The algorithmic bytes of a pass (24 B of positions in
and out, 12 B of x0 under the bound, 4 (d + 1) B of CSR, 12 d B gathered, d B of neighbour flags; d the mean degree) are set against
8 TB/s at the measured time.  That the gathered positions come mostly from L2 is an ASSUMPTION (marching tetrahedra numbers the vertices
in the grid's linear order); no counter run backs it.  The hub fan of 10^4 faces (one lane walks a row of 10^4) is timed for the record.
--only sphere runs the first mesh alone (a kernel-trace run).  --quality also runs examples/extract_mesh.py --sdf --steps 500
--resolution 128 --smooth N for N in 0, 5, 10, 20 on one shared fit and records its report and the enclosed volume."""
import argparse
import importlib.util
import json
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cc_bench = _load(os.path.join(ROOT, "profiles", "microbench", "mesh_components.py"), "mesh_components_bench")
ROUNDS, WARM = 20, 3
HBM_BYTES_PER_US = 8e6            # 8 TB/s


def timed(fn, rounds=ROUNDS, warm=WARM):
    return cc_bench.timed(fn, rounds=rounds, warm=warm)


def torch_adjacency(f, V):
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).long()
    e = torch.cat([e, e.flip(1)])
    keys = torch.unique(e[:, 0] * V + e[:, 1])
    return keys // V, keys % V


def torch_pass(x, u, w, factor):
    xd = x.double()
    s = torch.zeros_like(xd).index_add_(0, u, xd[w])
    deg = torch.bincount(u, minlength=x.shape[0]).double()[:, None]
    return torch.where(deg > 0, xd + factor * (s / deg.clamp_min(1.0) - xd), xd).float()


def torch_smooth(x, f, iterations, lam=0.5, mu=-0.53):
    u, w = torch_adjacency(f, x.shape[0])
    for _ in range(iterations):
        x = torch_pass(torch_pass(x, u, w, lam), u, w, mu)
    return x


def torch_normals(v, f):
    fl = f.long()
    a, b, c = (v[fl[:, k]].double() for k in range(3))
    area = 0.5 * torch.linalg.cross(b - a, c - a)
    s = torch.zeros(v.shape[0], 3, device=v.device, dtype=torch.float64)
    for k in range(3):
        s.index_add_(0, fl[:, k], area)
    return torch.nn.functional.normalize(s, dim=1).float()


def measure(msh, cell):
    import ngp_hip
    from ngp_hip import lib, ops
    v, f = msh.vertices, msh.faces
    V, T = v.shape[0], f.shape[0]
    L = lib.load()
    adj = ngp_hip.adjacency(msh)
    E2 = int(adj.neighbours.shape[0])
    d = E2 / max(V, 1)
    out = {"vertices": V, "faces": T, "directed_edges": E2, "mean_degree": d, "boundary_vertices": adj.boundary_vertices,
           "bad_faces": adj.bad_faces, "bad_vertices": adj.bad_vertices}
    keys = torch.empty(6 * T, device=v.device, dtype=torch.int64)
    counts = torch.empty(4, device=v.device, dtype=torch.int32)

    def make_keys():
        lib.check(L.ngp_mesh_adjacency_keys(ops._ptr(f), T, V, ops._ptr(keys), ops._ptr(counts), ops._stream()), "ngp_mesh_adjacency_keys")
    make_keys()
    out["adjacency_keys"] = timed(make_keys)
    out["adjacency_sort"] = timed(lambda: torch.sort(keys))
    out["adjacency"] = timed(lambda: ops.mesh_adjacency(v, f))
    out["adjacency_build_min_us"] = out["adjacency"]["min_us"] - out["adjacency_keys"]["min_us"] - out["adjacency_sort"]["min_us"]
    raw = (adj.row_start, adj.neighbours, adj.multiplicity, adj.vertex_flags)
    move = [0.5 * cell] * 3
    out["one_pass_bounded"] = timed(lambda: ops.mesh_smooth(v, *raw, 1, 0.5, 0.0, "fixed", None, move))
    out["one_pass_unbounded"] = timed(lambda: ops.mesh_smooth(v, *raw, 1, 0.5, 0.0, "fixed", None, None))
    out["clone_of_the_positions"] = timed(lambda: v.clone())            # ops.mesh_smooth starts with it: part of both numbers above
    for key, clamp in (("one_pass_bounded", 12), ("one_pass_unbounded", 0)):
        nbytes = V * (24 + clamp + 4 * (d + 1) + 12 * d + d)
        us = out[key]["min_us"] - out["clone_of_the_positions"]["min_us"]
        out[key].update(algorithmic_bytes=nbytes, kernel_min_us=us, fraction_of_8TBps=nbytes / us / HBM_BYTES_PER_US if us > 0 else None)
    out["ten_iterations"] = timed(lambda: ngp_hip.smooth_mesh(msh, iterations=10, max_move=move, normals=False, adjacency=adj))
    out["smooth_mesh_ten_iterations_whole_call"] = timed(lambda: ngp_hip.smooth_mesh(msh, iterations=10, max_move=move))
    out["vertex_normals"] = timed(lambda: ops.mesh_vertex_normals(v, f))
    nkeys = torch.empty(3 * T, device=v.device, dtype=torch.int64)
    lib.check(L.ngp_mesh_vertex_normals_keys(ops._ptr(f), T, V, ops._ptr(nkeys), ops._stream()), "ngp_mesh_vertex_normals_keys")
    out["vertex_normals_sort"] = timed(lambda: torch.sort(nkeys, stable=True))
    res = ngp_hip.smooth_mesh(msh, iterations=10, max_move=move, adjacency=adj)
    moved = (res.mesh.vertices - v).abs() / cell
    out["ten_iterations_displacement_cells"] = {"mean": float(moved.norm(dim=1).mean()), "max": float(moved.max())}
    try:
        u, w = torch_adjacency(f, V)
        same = u.numel() == E2 and torch.equal(w.int(), adj.neighbours)
        tc = {"adjacency": timed(lambda: torch_adjacency(f, V), rounds=5, warm=1), "neighbours_equal_ours": bool(same),
              "one_pass": timed(lambda: torch_pass(v, u, w, 0.5), rounds=5, warm=1),
              "ten_iterations": timed(lambda: torch_smooth(v, f, 10), rounds=3, warm=1),
              "vertex_normals": timed(lambda: torch_normals(v, f), rounds=5, warm=1)}
        free = ops.mesh_smooth(v, *raw, 1, 0.5, 0.0, "free", None, None)
        tc["one_pass_max_difference_to_ours"] = float((torch_pass(v, u, w, 0.5) - free).abs().max())
        tc["normals_max_difference_to_ours"] = float((torch_normals(v, f) - ops.mesh_vertex_normals(v, f)).abs().max())
        tc["ratio_adjacency"] = tc["adjacency"]["min_us"] / out["adjacency"]["min_us"]
        tc["ratio_one_pass"] = tc["one_pass"]["min_us"] / out["one_pass_unbounded"]["min_us"]
        tc["ratio_ten_iterations"] = tc["ten_iterations"]["min_us"] / (out["ten_iterations"]["min_us"] + out["adjacency"]["min_us"])
        tc["ratio_vertex_normals"] = tc["vertex_normals"]["min_us"] / out["vertex_normals"]["min_us"]
        out["torch_composition"] = tc
    except RuntimeError as e:                           # an operator the installed torch lacks on this device: recorded, not hidden
        out["torch_composition"] = {"error": str(e)[:200]}
    print(json.dumps(out))
    return out


def hub_fan(n, dev):
    import ngp_hip
    from ngp_hip import mesh, ops
    t = 2 * math.pi * torch.arange(n, dtype=torch.float64) / n
    v = torch.cat([torch.tensor([[0.0, 0.0, 0.3]], dtype=torch.float64), torch.stack([t.cos(), t.sin(), torch.zeros(n, dtype=torch.float64)], 1)]).float().to(dev)
    k = torch.arange(n)
    f = torch.stack([torch.zeros(n, dtype=torch.long), 1 + k, 1 + (k + 1) % n], 1).int().to(dev)
    adj = ngp_hip.adjacency(mesh.Mesh(v, f, None))
    raw = (adj.row_start, adj.neighbours, adj.multiplicity, adj.vertex_flags)
    return {"faces": n, "hub_degree": int(adj.degree[0]), "one_pass_free": timed(lambda: ops.mesh_smooth(v, *raw, 1, 0.5, 0.0, "free", None, None)),
            "vertex_normals": timed(lambda: ops.mesh_vertex_normals(v, f))}


def quality(dev):
    """examples/extract_mesh.py --sdf --steps 500 --resolution 128 --smooth N on one shared fit."""
    import ngp_hip
    ex = _load(os.path.join(ROOT, "examples", "extract_mesh.py"), "extract_mesh_example")
    fits, fit = [], ex.fit_sphere_sdf

    def fit_once(args, d):
        if not fits:
            fits.append(fit(args, d))
        return fits[0]
    ex.fit_sphere_sdf = fit_once
    rows, path = {}, os.path.join(tempfile.mkdtemp(), "sphere.ply")
    for n in (0, 5, 10, 20):
        info = ex.main(["--sdf", "--steps", "500", "--resolution", "128", "--out", path] + (["--smooth", str(n)] if n else []))
        msh = info["mesh"]
        dist, angle = ex.sphere_errors(msh, 1.0 / 128)
        stats = ngp_hip.components(msh).stats
        rows["smooth_%d" % n] = {"vertices": info["vertices"], "faces": info["faces"], "euler": info["euler"], "boundary_edges": info["boundary_edges"],
                                 "sphere_distance_cells": dist, "face_normal_error_degrees": angle, "volume": float(stats.volume.sum()),
                                 "true_volume": 4.0 / 3.0 * math.pi * 0.3**3, "report": info.get("smooth")}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth.json"))
    ap.add_argument("--resolution", type=int, default=256, help="cells per axis: 257^3 points")
    ap.add_argument("--train_steps", type=int, default=500)
    ap.add_argument("--only", default=None, choices=["sphere"])
    ap.add_argument("--quality", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernels' time")
    dev = torch.device("cuda")
    import ngp_hip
    from ngp_hip import mesh
    res = args.resolution
    out = {"what": "smoothing of two meshes extracted at %d^3 points: HIP events around the call, %d rounds after %d warm ones"
                   % (res + 1, ROUNDS, WARM)}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    sdf = lambda x: torch.linalg.norm(x - torch.tensor([0.5, 0.47, 0.52], device=x.device), dim=1) - 0.3
    values = mesh.sample_grid(sdf, (0, 0, 0), (1, 1, 1), res, device=dev)
    msh, _ = cc_bench.extract(values, 0.0, -1, (0.0, 0.0, 0.0), (1.0 / res,) * 3)
    out["sphere_sdf"] = measure(msh, 1.0 / res)
    save()
    del values, msh
    if args.only is None:
        out["hub_fan"] = hub_fan(10**4, dev)
        save()
        ex = _load(os.path.join(ROOT, "examples", "extract_mesh.py"), "extract_mesh_example_train")
        model, thr = ex.train_procedural_model(args.train_steps, dev)
        model.eval()
        b = (model.xyz_min.reshape(3).tolist(), model.xyz_max.reshape(3).tolist())
        lo, h = mesh.grid_spacing(b[0], b[1], res)
        with torch.autocast("cuda", dtype=torch.float16):
            grid = mesh.sample_grid(model.density, b[0], b[1], res, device=dev)
        msh, _ = cc_bench.extract(grid, thr, +1, lo, h)
        cleaned, _ = ngp_hip.clean_mesh(msh, keep_largest=1)
        row = measure(cleaned, h[0])
        before = mesh.topology(cleaned)
        after = mesh.topology(ngp_hip.smooth_mesh(cleaned, iterations=10, max_move=[0.5 * x for x in h]).mesh)
        row.update(train_steps=args.train_steps, threshold=thr, faces_before_cleaning=int(msh.faces.shape[0]), topology_before=before,
                   topology_after_ten_iterations=after)
        out["procedural_scene_keep_largest_1"] = row
        save()
        del grid, msh, cleaned, model
    if args.quality:
        out["quality_sphere_fit_resolution_128"] = quality(dev)
        save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
