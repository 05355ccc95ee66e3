"""Time of the mesh simplification (csrc/mesh_simplify.hip) on the MI355X, recorded in profiles/mesh_simplify.json.

    python profiles/microbench/mesh_simplify.py --out profiles/mesh_simplify.json

The two meshes of profiles/microbench/mesh_components.py, extracted at 257^3 points: the analytic sphere and the density of an NGP
trained on the procedural scene for 500 steps, the latter after clean_mesh(keep_largest=1).  Cells of 2 and of 4 grid cells.  HIP events
around the call, 10 rounds after 2 warm ones, the minimum reported first:
  count_phase        ops.mesh_simplify_count: keys, the stable torch.sort of the V keys, numbering, surviving faces, the scans (no read)
  incidence          the 3 T incidence keys and their stable torch.sort
  emit               ops.mesh_simplify_emit: incidence + run bounds + the per-cluster sums and solves + the surviving faces
  sums_solve_faces   emit - incidence
  simplify_mesh      the whole call with its two host reads (the box of the vertices, the counts)
  torch_sort_*       the two sorts alone: the share that is plumbing
beside the extraction's own count + emit on the same grid, clean_mesh on the same mesh and a torch composition of the same contract
(torch.unique of the keys, index_add_ of the quadrics in float64, torch.linalg.solve), whose V', T', faces and positions are set
beside ours.  V', T' and
surface_distance(simplified, original) are recorded for each.  --only sphere runs the first mesh alone (a kernel-trace run)."""
import argparse
import importlib.util
import json
import os
import sys

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
timed = cc_bench.timed


def torch_simplify(v, f, lo, h, n, eps=1e-3):
    """The same contract from torch operators -> (vertices [V',3] f32, faces [T',3] int64)."""
    dev = v.device
    lo_t, h_t = torch.tensor(lo, device=dev), torch.tensor(h, device=dev)
    n_t = torch.tensor(n, device=dev)
    q = torch.minimum(torch.floor((v - lo_t) * (1.0 / h_t)).clamp_min(0.0), (n_t - 1).float()).long()
    key = q[:, 0] + n[0] * (q[:, 1] + n[1] * q[:, 2])
    uniq, cl = torch.unique(key, return_inverse=True)
    C = uniq.numel()
    qc = torch.stack([uniq % n[0], uniq // n[0] % n[1], uniq // (n[0] * n[1])], 1).double()
    centre = lo_t.double() + (qc + 0.5) * h_t.double()
    fl = f.long()
    fc = cl[fl]
    survives = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 2] != fc[:, 0])
    a, b, c = (v[fl[:, k]].double() for k in range(3))
    nn = torch.linalg.cross(b - a, c - a)
    length = torch.linalg.norm(nn, dim=1)
    has = length > 0
    w, nrm = 0.5 * length, nn / length.clamp_min(1e-300)[:, None]
    sums = torch.zeros(C, 9, device=dev, dtype=torch.float64)
    for k, first in enumerate((has, has & (fc[:, 1] != fc[:, 0]), has & (fc[:, 2] != fc[:, 0]) & (fc[:, 2] != fc[:, 1]))):
        ck = fc[first, k]
        wk, nk = w[first], nrm[first]
        d = -(nk * (a[first] - centre[ck])).sum(1)
        rows = torch.cat([wk[:, None] * nk[:, [0, 0, 0, 1, 1, 2]] * nk[:, [0, 1, 2, 1, 2, 2]], (wk * d)[:, None] * nk], 1)
        sums.index_add_(0, ck, rows)
    mean = torch.zeros(C, 3, device=dev, dtype=torch.float64).index_add_(0, cl, v.double() - centre[cl])
    mean /= torch.bincount(cl, minlength=C)[:, None]
    A = sums[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].view(C, 3, 3)
    trace = A.diagonal(dim1=1, dim2=2).sum(1)
    mu = eps * trace.clamp_min(1e-300)
    y = torch.linalg.solve(A + mu[:, None, None] * torch.eye(3, device=dev, dtype=torch.float64), (mu[:, None] * mean - sums[:, 6:9])[:, :, None])[:, :, 0]
    y = torch.where(trace[:, None] > 0, y, mean)
    half = 0.5 * h_t.double()
    x = (centre + torch.maximum(torch.minimum(y, half), -half)).float()
    used = torch.zeros(C, dtype=torch.bool, device=dev)
    used[fc[survives].reshape(-1)] = True
    number = torch.cumsum(used, 0) - 1
    return x[used], number[fc[survives]]


def measure(msh, grid_h, cells, extraction_us):
    import ngp_hip
    from ngp_hip import lib, mesh, ops
    v, f = msh.vertices, msh.faces
    V, T = v.shape[0], f.shape[0]
    out = {"vertices": V, "faces": T, "extraction_count_plus_emit_min_us": extraction_us}
    out["clean_mesh"] = timed(lambda: ngp_hip.clean_mesh(msh))
    box = (v.amin(0).tolist(), v.amax(0).tolist())
    for k in cells:
        cell = k * grid_h
        lo, h, n = mesh.simplify_grid(box, cell=cell)
        st = ops.mesh_simplify_count(v, f, lo, h, n)
        C, Vo, To, bad_v, bad_f = st.counts.tolist()
        row = {"cell": cell, "grid": list(n), "clusters": C, "out_vertices": Vo, "out_faces": To}
        row["count_phase"] = timed(lambda: ops.mesh_simplify_count(v, f, lo, h, n))
        keys = torch.empty(3 * T, device=v.device, dtype=torch.int64)

        def incidence():
            lib.check(lib.load().ngp_mesh_simplify_incidence_keys(ops._ptr(v), ops._ptr(f), T, V, ops._ptr(st.vertex_cluster), ops._ptr(keys),
                                                                   ops._stream()), "ngp_mesh_simplify_incidence_keys")
            return torch.sort(keys, stable=True)
        row["incidence"] = timed(incidence)
        row["emit"] = timed(lambda: ops.mesh_simplify_emit(v, f, st, C, Vo, To))
        row["sums_solve_faces_min_us"] = row["emit"]["min_us"] - row["incidence"]["min_us"]
        row["simplify_mesh"] = timed(lambda: ngp_hip.simplify_mesh(msh, cell=cell))
        vertex_keys = torch.empty(V, device=v.device, dtype=torch.int64).copy_(st.vertex_keys[torch.randperm(V, device=v.device)])
        row["torch_sort_of_V_int64_keys"] = timed(lambda: torch.sort(vertex_keys, stable=True))
        row["torch_sort_of_3T_int64_keys"] = timed(lambda: torch.sort(keys, stable=True))
        row["sorts_share_of_count_plus_emit"] = (row["torch_sort_of_V_int64_keys"]["min_us"] + row["torch_sort_of_3T_int64_keys"]["min_us"]) \
            / (row["count_phase"]["min_us"] + row["emit"]["min_us"])
        small = ngp_hip.simplify_mesh(msh, cell=cell)
        assert small.mesh.faces.shape[0] == To and small.mesh.vertices.shape[0] == Vo
        try:
            tv, tf = torch_simplify(v, f, lo.tolist(), h.tolist(), n)
            same = tuple(tv.shape) == (Vo, 3) and tuple(tf.shape) == (To, 3)
            row["torch_composition"] = dict(timed(lambda: torch_simplify(v, f, lo.tolist(), h.tolist(), n), rounds=3, warm=1),
                                            out_vertices=int(tv.shape[0]), out_faces=int(tf.shape[0]),
                                            faces_equal_ours=bool(same and torch.equal(tf.int(), small.mesh.faces)),
                                            max_position_difference=float((tv - small.mesh.vertices).abs().max()) if same else None)
        except RuntimeError as e:                       # an operator the installed torch lacks on this device: recorded, not hidden
            row["torch_composition"] = {"error": str(e)[:200]}
        row["over_extraction"] = (row["count_phase"]["min_us"] + row["emit"]["min_us"]) / extraction_us
        row["surface_distance_to_original"] = ngp_hip.surface_distance(small.mesh, msh, 65536, torch.Generator().manual_seed(7))
        row["mean_surface_distance_in_cells"] = row["surface_distance_to_original"]["mean"] / cell
        out["cell_%d_grid_cells" % k] = row
        print(json.dumps(row))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify.json"))
    ap.add_argument("--resolution", type=int, default=256, help="cells per axis: 257^3 points")
    ap.add_argument("--train_steps", type=int, default=500)
    ap.add_argument("--only", default=None, choices=["sphere"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernels' time")
    dev = torch.device("cuda")
    import ngp_hip
    from ngp_hip import mesh
    res = args.resolution
    out = {"what": "simplification of two meshes extracted at %d^3 points, cells of 2 and 4 grid cells: HIP events around the call, "
                   "%d rounds after 2 warm ones" % (res + 1, cc_bench.ROUNDS)}
    sdf = lambda x: torch.linalg.norm(x - torch.tensor([0.5, 0.47, 0.52], device=x.device), dim=1) - 0.3
    values = mesh.sample_grid(sdf, (0, 0, 0), (1, 1, 1), res, device=dev)
    msh, us = cc_bench.extract(values, 0.0, -1, (0.0, 0.0, 0.0), (1.0 / res,) * 3)
    out["sphere_sdf"] = measure(msh, 1.0 / res, (2, 4), us)
    del values, msh
    if args.only is None:
        ex = _load(os.path.join(ROOT, "examples", "extract_mesh.py"), "extract_mesh_example")
        model, thr = ex.train_procedural_model(args.train_steps, dev)
        model.eval()
        b = (model.xyz_min.reshape(3).tolist(), model.xyz_max.reshape(3).tolist())
        lo, h = mesh.grid_spacing(b[0], b[1], res)
        with torch.autocast("cuda", dtype=torch.float16):
            grid = mesh.sample_grid(model.density, b[0], b[1], res, device=dev)
        msh, us = cc_bench.extract(grid, thr, +1, lo, h)
        cleaned, _ = ngp_hip.clean_mesh(msh, keep_largest=1)
        out["procedural_scene_keep_largest_1"] = measure(cleaned, h[0], (2, 4), us)
        out["procedural_scene_keep_largest_1"].update(train_steps=args.train_steps, threshold=thr, faces_before_cleaning=int(msh.faces.shape[0]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
