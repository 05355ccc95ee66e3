"""Time of the connected-components kernels (csrc/mesh_components.hip) on the MI355X, recorded in profiles/mesh_components.json.

    python profiles/microbench/mesh_components.py --out profiles/mesh_components.json

Two meshes, both extracted at 257^3 points as profiles/microbench/mesh_extract.py does: the analytic sphere (one component) and the
density of an NGP trained on the procedural scene for 500 steps with examples/extract_mesh.py's schedule (thousands of components).
Timed with HIP events, 10 rounds after 2 warm ones, minimum and median; a timed call includes its host reads (the round flags, the
counts), because that is what a caller waits for:
  label       ops.mesh_components_label: the union-find rounds and the numbering; the rounds it took
  table       ops.mesh_components_table, and torch.sort of its 3 T int64 keys alone (the share of the table that is plumbing)
  measure     ops.mesh_components_measure, and the stable torch.sort of face_component alone
  select      ops.mesh_select keeping the largest component (count, scan, one read, emit)
Compared against, on the same mesh: mesh.topology() on the host (wall clock, one run); a torch composition of the same labelling
(scatter_reduce(amin) over the edges, then pointer jumping until nothing moves, repeated until fixed; its number of components must
equal ours); and the extraction's own count + emit.  The procedural mesh is also cleaned with keep_largest=1 and V, T, euler,
boundary edges and the component count before and after are recorded: the mesh is the one
`examples/extract_mesh.py --train_steps 500 --resolution 256 --keep_largest 1` extracts and cleans, built in this process."""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUNDS = 10


def timed(fn, rounds=ROUNDS, warm=2):
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


def torch_label(faces, n_vertices):
    """The same labelling from torch operators alone -> (root per vertex, outer rounds)."""
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    parent = torch.arange(n_vertices, device=faces.device)
    rounds = 0
    while True:
        pa, pb = parent[e[:, 0]], parent[e[:, 1]]
        new = parent.scatter_reduce(0, torch.maximum(pa, pb), torch.minimum(pa, pb), "amin")
        while True:
            jumped = new[new]
            if torch.equal(jumped, new):
                break
            new = jumped
        rounds += 1
        if torch.equal(new, parent):
            return parent, rounds
        parent = new


def measure(msh, extraction_us):
    from ngp_hip import mesh, ops
    import ngp_hip
    V, T = msh.vertices.shape[0], msh.faces.shape[0]
    cc = ngp_hip.components(msh)
    s = cc.stats
    out = {"vertices": V, "faces": T, "components": cc.n, "rounds": cc.rounds, "unused_vertices": cc.unused_vertices,
           "largest_component_faces": int(s.faces.max()), "components_with_boundary": int((s.boundary_edges > 0).sum()),
           "components_below_100_faces": int((s.faces < 100).sum())}
    out["label"] = timed(lambda: ops.mesh_components_label(msh.faces, V))
    out["table"] = timed(lambda: ops.mesh_components_table(msh.faces, V, cc.vertex_component, cc.face_component, cc.n))
    e = torch.cat([msh.faces[:, [0, 1]], msh.faces[:, [1, 2]], msh.faces[:, [2, 0]]]).long()
    keys = torch.minimum(e[:, 0], e[:, 1]) * V + torch.maximum(e[:, 0], e[:, 1])               # the keys the table sorts, up to their order
    out["table"]["torch_sort_of_3T_int64_keys"] = timed(lambda: torch.sort(keys))
    out["measure"] = timed(lambda: ops.mesh_components_measure(msh.vertices, msh.faces, cc.face_component, s.faces, cc.bad_faces))
    out["measure"]["torch_stable_sort_of_face_component"] = timed(lambda: torch.sort(cc.face_component, stable=True))
    keep = torch.zeros(cc.n, dtype=torch.bool, device=msh.faces.device)
    keep[int(s.area.argmax())] = True
    out["select"] = timed(lambda: ops.mesh_select(msh.vertices, msh.normals, msh.faces, cc.vertex_component, cc.face_component, keep))
    out["label_table_measure_select_min_us"] = sum(out[k]["min_us"] for k in ("label", "table", "measure", "select"))
    t0 = time.time()
    top = mesh.topology(msh)
    out["host_topology"] = dict(top, seconds=time.time() - t0)
    parent, rounds = torch_label(msh.faces, V)
    used = cc.vertex_component >= 0
    out["torch_composition"] = dict(timed(lambda: torch_label(msh.faces, V), rounds=3, warm=1), outer_rounds=rounds,
                                    components=int(torch.unique(parent[used]).numel()))
    assert out["torch_composition"]["components"] == cc.n
    assert int(s.euler.sum()) + cc.unused_vertices == top["euler"] and int(s.boundary_edges.sum()) == top["boundary_edges"]
    out["extraction_count_plus_emit_min_us"] = extraction_us
    out["cleaning_over_extraction"] = out["label_table_measure_select_min_us"] / extraction_us
    return out, cc


def extract(values, iso, sign, lo, h):
    from ngp_hip import mesh, ops
    workspace, counts = ops.mesh_count(values, iso, sign)
    V, T = counts.tolist()
    us = timed(lambda: ops.mesh_count(values, iso, sign, workspace=workspace))["min_us"] \
        + timed(lambda: ops.mesh_emit(values, iso, sign, lo, h, workspace, V, T, normals=True))["min_us"]
    return mesh.marching_tetrahedra(values, iso, sign=sign, lo=lo, h=h), us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_components.json"))
    ap.add_argument("--resolution", type=int, default=256, help="cells per axis: 257^3 points")
    ap.add_argument("--train_steps", type=int, default=500)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernels' time")
    dev = torch.device("cuda")
    import ngp_hip
    from ngp_hip import mesh
    res = args.resolution
    out = {"what": "connected components of two meshes extracted at %d^3 points: HIP events around the ops.* call (host reads included), "
                   "%d rounds after 2 warm ones" % (res + 1, ROUNDS)}
    sdf = lambda x: torch.linalg.norm(x - torch.tensor([0.5, 0.47, 0.52], device=x.device), dim=1) - 0.3
    values = mesh.sample_grid(sdf, (0, 0, 0), (1, 1, 1), res, device=dev)
    msh, us = extract(values, 0.0, -1, (0.0, 0.0, 0.0), (1.0 / res,) * 3)
    out["sphere_sdf"], _ = measure(msh, us)
    print("sphere:", json.dumps(out["sphere_sdf"]))
    del values, msh
    spec = importlib.util.spec_from_file_location("extract_mesh_example", os.path.join(ROOT, "examples", "extract_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    model, thr = ex.train_procedural_model(args.train_steps, dev)
    model.eval()
    b = (model.xyz_min.reshape(3).tolist(), model.xyz_max.reshape(3).tolist())
    lo, h = mesh.grid_spacing(b[0], b[1], res)
    with torch.autocast("cuda", dtype=torch.float16):
        grid = mesh.sample_grid(model.density, b[0], b[1], res, device=dev)
    msh, us = extract(grid, thr, +1, lo, h)
    out["procedural_scene_density"], cc = measure(msh, us)
    out["procedural_scene_density"].update(train_steps=args.train_steps, threshold=thr)
    print("procedural:", json.dumps(out["procedural_scene_density"]))
    cleaned, report = ngp_hip.clean_mesh(msh, keep_largest=1)
    report.pop("kept")
    out["procedural_scene_keep_largest_1"] = {"before": dict(mesh.topology(msh), components=cc.n),
                                              "after": dict(mesh.topology(cleaned), components=ngp_hip.components(cleaned).n), "report": report}
    print("keep_largest=1:", json.dumps(out["procedural_scene_keep_largest_1"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
