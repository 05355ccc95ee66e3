"""Time of the importance-resampling kernels (csrc/resample.hip) on the MI355X against the same refinement composed from torch ops,
recorded in profiles/resample.json.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o resample -- python profiles/microbench/resample.py --out profiles/resample.json
    python profiles/microbench/resample.py --out profiles/resample.json --trace DIR        # folds the trace's medians into the file

Workload: 8192 lego rays marched (jittered) through the procedural scene's occupancy (128^3 cells, occupied where the analytic density
is positive at the cell centre) -- the ~217 k samples of profiles/surface_composite.json --, weights from the surface compositor with
f = -0.005 inside the boxes, +0.05 outside, c = -1, s = 400, r = 1, and K = 32 draws per ray with the march's jitter.
In one process, alternating, HIP events around each: ops.resample_rays (three launches, two allocations' worth of workspaces and one
read of the total) and `torch_refine`, the same refinement from cumsum / searchsorted / sort / repeat_interleave / bincount (the
comparison, not the code under test: it rounds differently and is only checked to give the same number of samples within 1 %)."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUNDS, WARM = 30, 3
N_RAYS, K = 8192, 32
HBM_BYTES_PER_US = 8e6                      # 8 TB/s


def workload(dev):
    from modules.utils import packbits
    from ngp_hip import ops, synthetic
    from ngp_hip.surface import MAX_SAMPLES, SDFField
    torch.manual_seed(23)
    model = SDFField(scale=0.5, levels=8, log2_T=14, max_res=256).to(dev)          # the holder of the occupancy grid only
    with torch.no_grad():
        for c, (indices, coords) in enumerate(model.get_all_cells()):
            s = min(2 ** (c - 1), model.scale)
            half = s / model.grid_size
            x = (coords / (model.grid_size - 1) * 2 - 1) * (s - half)
            model.density_grid[c, indices] = synthetic.procedural_field(x)[0].float()
        packbits(model.density_grid.reshape(-1).contiguous(), 1e-6, model.density_bitfield)
    o, d = synthetic.lego_rays(N_RAYS, seed=23)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    noise = torch.rand(N_RAYS, device=dev)
    hits = ops.ray_aabb(o, d, 0.5)
    rays_a, xyzs, dirs, deltas, ts, total = ops.march_train(o, d, hits, model.density_bitfield, noise, model.cascades, 0.5, 0.0,
                                                            model.grid_size, MAX_SAMPLES)
    inside = synthetic.procedural_field(xyzs)[0] > 0
    f = torch.where(inside, torch.full_like(ts, -0.005), torch.full_like(ts, 0.05))
    ws = ops.surface_composite_fwd(f, torch.full_like(ts, -1.0), torch.zeros_like(xyzs), deltas, ts, rays_a,
                                   torch.full((1,), 400.0, device=dev), 1.0, 1e-4)[6]
    return dict(ws=ws, deltas=deltas, ts=ts, rays_a=rays_a, rays_o=o, rays_d=d, noise=noise)


def torch_refine(w):
    """The same refinement from torch ops (float32; the CDF is one global cumsum, re-based per ray)."""
    ws, deltas, ts, rays_a, o, d, noise = (w[k] for k in ("ws", "deltas", "ts", "rays_a", "rays_o", "rays_d", "noise"))
    n, S = rays_a.shape[0], ws.shape[0]
    cnt, start = rays_a[:, 2].long(), rays_a[:, 1].long()
    ray_of = torch.repeat_interleave(torch.arange(n, device=ws.device), cnt)
    wt = ws.clamp_min(0.0)
    c = torch.cumsum(wt, 0)
    base = torch.where(start > 0, c[(start - 1).clamp_min(0)], torch.zeros_like(c[:1]))
    last = c[(start + cnt - 1).clamp(0, S - 1)] - base
    ok = (cnt > 0) & (last > 0)
    u = (torch.arange(K, device=ws.device)[None, :] + noise[rays_a[:, 0].long()][:, None]) / K
    target = u * last[:, None]
    j = torch.searchsorted(c, (target + base[:, None]).reshape(-1), right=True).view(n, K)
    j = torch.minimum(j.clamp_min(0), (start + cnt - 1).clamp_min(0)[:, None])
    c_prev = torch.where(j > start[:, None], c[(j - 1).clamp_min(0)] - base[:, None], torch.zeros_like(target))
    lo, hi = ts - 0.5 * deltas, ts + 0.5 * deltas
    tstar = lo[j] + (target - c_prev) / wt[j] * deltas[j]
    keep = ok[:, None] & (lo[j] < tstar) & (tstar < hi[j])
    keep[:, 1:] &= tstar[:, 1:] != tstar[:, :-1]
    starts = torch.cat([lo, tstar[keep]])
    parent = torch.cat([torch.arange(S, device=ws.device), j[keep]])
    key = parent.double() + ((starts - lo[parent]) / deltas[parent]).double().clamp(0.0, 0.999999)
    order = torch.sort(key).indices
    a, par = starts[order], parent[order]
    nxt_same = torch.cat([par[1:] == par[:-1], torch.zeros(1, dtype=torch.bool, device=ws.device)])
    b = torch.where(nxt_same, torch.cat([a[1:], a[:1]]), hi[par])
    cut = torch.cat([nxt_same[:1] & False, nxt_same[:-1]]) | nxt_same
    t_new = torch.where(cut, 0.5 * (a + b), ts[par])
    d_new = torch.where(cut, b - a, deltas[par])
    ray_new = ray_of[par]
    cnt_new = torch.bincount(ray_new, minlength=n)
    rays_a_new = torch.stack([rays_a[:, 0].long(), torch.cumsum(cnt_new, 0) - cnt_new, cnt_new], 1).int()
    ridx = rays_a[:, 0].long()[ray_new]
    dirs = d[ridx]
    xyzs = o[ridx] + t_new[:, None] * dirs
    return rays_a_new, xyzs, dirs, d_new, t_new, par.int(), int(a.shape[0])


def alternate(fns, rounds=ROUNDS, warm=WARM):
    for _ in range(warm):
        for fn in fns.values():
            fn()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3)
    return {k: {"min_us": min(v), "median_us": float(np.median(v)), "max_us": max(v)} for k, v in us.items()}


def fold_trace(out, trace_dir):
    """Medians of the three kernels from rocprofv3's kernel trace (csv)."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    dur = {}
    for path in files:
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                for k in ("resample_count_kernel", "resample_scan_kernel", "resample_write_kernel"):
                    if k in name:
                        dur.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out["kernels_rocprofv3"] = {k: {"launches": len(v), "min_us": min(v), "median_us": float(np.median(v)), "max_us": max(v)}
                                for k, v in dur.items()}
    S, S_out, kept = out["marched_samples"], out["refined_samples"], out["refined_samples"] - out["marched_samples"]
    by = {"resample_count_kernel": S * (4 + 4) + N_RAYS * (12 + 4 + 4) + N_RAYS * K * 16 + kept * 8,
          "resample_write_kernel": S * 8 + kept * 8 + N_RAYS * (24 + 24) + S_out * (12 + 12 + 4 + 4 + 4)}
    out["algorithmic_bytes"] = dict(by, note="count: ws read + CDF written per section, per draw the ws / ts / deltas / two CDF entries of its "
                                    "section (16 B; the bisection's ~log2 N further CDF reads hit lines the wave just wrote) and 8 B staged "
                                    "per kept cut; write: ts, deltas read per section, 8 B per kept cut, 36 B written per child")
    for k, nb in by.items():
        if k in out["kernels_rocprofv3"]:
            out["kernels_rocprofv3"][k]["fraction_of_8TBps_at_median"] = nb / out["kernels_rocprofv3"][k]["median_us"] / HBM_BYTES_PER_US


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.json"))
    ap.add_argument("--trace", default=None, help="fold the kernel trace under this directory into --out; runs nothing on the GPU")
    ap.add_argument("--traced", default=None, help="with --trace: the --out file the traced process wrote")
    args = ap.parse_args()
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    if args.trace is None:
        if not torch.cuda.is_available():
            raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernels' time")
        from ngp_hip import ops
        w = workload(torch.device("cuda"))
        call = lambda: ops.resample_rays(w["ws"], w["deltas"], w["ts"], w["rays_a"], w["rays_o"], w["rays_d"], w["noise"], K)
        got, ref = call(), torch_refine(w)
        S, S_out = int(w["ws"].shape[0]), int(got[6])
        assert abs(ref[6] - S_out) <= 0.01 * S_out, (ref[6], S_out)
        out.update(what="ops.resample_rays (ngp_resample_count / _scan / _write) against the same refinement composed from torch ops; HIP "
                        "events around each whole call, alternating, %d rounds after %d warm ones; kernel times from one rocprofv3 "
                        "--kernel-trace --stats run of this script" % (ROUNDS, WARM),
                   rays=N_RAYS, K=K, marched_samples=S, refined_samples=S_out, torch_refined_samples=ref[6],
                   rays_cut=int((got[0][:, 2] > w["rays_a"][:, 2]).sum()), whole_call_events=alternate({"ops_resample_rays": call,
                                                                                                     "torch_refine": lambda: torch_refine(w)}))
        print(json.dumps(out, indent=1))
    else:
        fold_trace(out, args.trace)
        if args.traced and os.path.exists(args.traced):      # the traced process's own event times: tracing slows the host
            with open(args.traced) as f:
                out["whole_call_events_under_rocprofv3"] = json.load(f)["whole_call_events"]
        print(json.dumps(out.get("kernels_rocprofv3"), indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
