"""One 800 x 800 frame of the trained example model (examples/train_surface.py at its defaults) through the sphere tracer
(csrc/sdf_trace.hip) on the MI355X, against the training renderer at test time and against the same tracing rule composed from torch
ops, recorded in profiles/sdf_trace.json.

    python profiles/microbench/sdf_trace.py --out profiles/sdf_trace.json --save MODEL.pt          # trains, measures, keeps the model
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o sdf -- python profiles/microbench/sdf_trace.py --load MODEL.pt --kernel-only --out T.json
    python profiles/microbench/sdf_trace.py --out profiles/sdf_trace.json --trace DIR              # folds the kernel's times into the file

In one process, alternating, HIP events around each whole call: trace_surface (one launch; the coarse occupancy bits and the weight
pack are made once outside), render_surface(test_time=True, chunk = the whole frame: a chunk in which no ray marches a sample is
refused by the compositor's entry point, and the first 16 384 rays of this frame are sky) and torch_trace, a masked batched loop over model.sdf under no_grad that
follows the rule of include/ngp_hip.h ("sphere tracing") step for step.  torch_trace is the yardstick, not the code under test: it
rounds differently (torch's Linear sums in another order), so it is compared in status and depth and the shares that agree are
recorded.  evaluations / s = the sum of n_eval over the kernel's time; 12.9 kFLOP per evaluation is arithmetic (2 x 6464 multiply-adds
of the 35 -> 64 -> 64 -> 1 network), not a measurement."""
import argparse
import csv
import glob
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

WH, ROUNDS, WARM = 800, 5, 1
FLOP_PER_EVAL = 2 * (64 * 35 + 64 * 64 + 64)
PARAMS = dict(eps=1e-4, step_scale=1.0, min_step=1.7320508075688772 / 1024, n_refine=8, max_evals=256)
KERNEL = "sdf_trace_kernel"


def trained_model(args, dev):
    from ngp_hip.surface import SDFField
    if args.load:
        model = SDFField(scale=0.5, levels=16, log2_T=19, max_res=1024).to(dev)
        model.load_state_dict(torch.load(args.load, map_location=dev))
        return model, None
    import train_surface
    info, model = train_surface.main([], return_model=True)
    if args.save:
        torch.save(model.state_dict(), args.save)
    return model, info


def frame_rays(dev):
    from ngp_hip import synthetic
    o, d = synthetic.orbit_camera_rays(1, (WH, WH), seed=4007)
    o, d = torch.from_numpy(o).to(dev).float().contiguous(), torch.from_numpy(d).to(dev).float()
    return o, (d / torch.linalg.norm(d, dim=1, keepdim=True)).contiguous()


def torch_trace(model, o, d, eps, step_scale, min_step, n_refine, max_evals):
    """The tracing rule from torch ops: every round the live rays walk through empty cells, then one model.sdf call on the rays that
    need a value.  One cascade (scale 0.5).  -> status, t, n_eval."""
    from ngp_hip import ops
    assert model.cascades == 1
    dev, n, G = o.device, o.shape[0], model.grid_size
    dt_min, mb = 1.7320508075688772 / 1024, min(0.5, model.scale)
    bits = model.density_bitfield
    hits = ops.ray_aabb(o, d, model.scale)
    t, t2 = hits[:, 0].clone(), hits[:, 1].clone()
    d_inv = 1.0 / d
    status = torch.full((n,), -1, device=dev, dtype=torch.int32)
    t_fin, n_eval = torch.zeros(n, device=dev), torch.zeros(n, device=dev, dtype=torch.int32)
    have_prev, refine = torch.zeros(n, device=dev, dtype=torch.bool), torch.zeros(n, device=dev, dtype=torch.bool)
    prev_t, prev_f, ta, fa, tb, fb = (torch.zeros(n, device=dev) for _ in range(6))
    k_ref = torch.zeros(n, device=dev, dtype=torch.int32)

    def finish(idx, st, tf):
        status[idx] = st
        t_fin[idx] = tf

    bad = ~((t2 >= 0) & torch.isfinite(t2))
    finish(bad.nonzero().squeeze(1), 0, -1.0)
    while bool((status < 0).any()):
        te = t.clone()
        pending = (status < 0) & refine
        te[pending] = 0.5 * (ta[pending] + tb[pending])
        walk = ((status < 0) & ~refine).nonzero().squeeze(1)
        while walk.numel():
            out = ~(t[walk] < t2[walk])
            finish(walk[out], 0, t2[walk[out]])
            walk = walk[~out]
            if not walk.numel():
                break
            xyz = o[walk] + t[walk, None] * d[walk]
            nxyz = (0.5 * (xyz / mb + 1.0) * G).clamp(0.0, G - 1.0)
            idx = ops.morton3d(nxyz.int().contiguous()).long()
            occ = ((bits[idx >> 3] >> (idx & 7).to(torch.uint8)) & 1).bool()
            full = occ & (n_eval[walk] >= max_evals)
            finish(walk[full], 3, t[walk[full]])
            go = walk[occ & ~full]
            pending[go] = True
            w = walk[~occ]
            v = (((nxyz[~occ] + 0.5 + 0.5 * torch.sign(d[w])) / G * 2.0 - 1.0) * mb - xyz[~occ]) * d_inv[w]
            tn = t[w] + torch.nan_to_num(v, nan=float("inf")).amin(1).clamp_min(0.0) + dt_min
            have_prev[w] = False
            stuck = ~(tn > t[w])
            finish(w[stuck], 3, t[w[stuck]])
            t[w[~stuck]] = tn[~stuck]
            walk = w[~stuck]
        te = torch.where(pending & ~refine, t, te)
        p = pending.nonzero().squeeze(1)
        if not p.numel():
            continue
        f = model.sdf((o[p] + te[p, None] * d[p]).contiguous())
        n_eval[p] += 1
        fin = torch.isfinite(f)
        finish(p[~fin], 3, te[p[~fin]])
        p, f = p[fin], f[fin]
        rf = refine[p]
        q, fq = p[~rf], f[~rf]
        far = fq > eps
        a = q[far]
        prev_t[a], prev_f[a], have_prev[a] = t[a], fq[far], True
        t[a] = t[a] + torch.clamp_min(fq[far] * step_scale, min_step)
        q, fq = q[~far], fq[~far]
        pos = fq >= 0
        finish(q[pos], 1, t[q[pos]])
        q, fq = q[~pos], fq[~pos]
        first = ~have_prev[q]
        finish(q[first], 2, t[q[first]])
        q, fq = q[~first], fq[~first]
        ta[q], fa[q], tb[q], fb[q], k_ref[q], refine[q] = prev_t[q], prev_f[q], t[q], fq, 0, True
        b, fm = p[rf], f[rf]
        up = fm >= 0
        ta[b[up]], fa[b[up]] = te[b[up]], fm[up]
        tb[b[~up]], fb[b[~up]] = te[b[~up]], fm[~up]
        k_ref[b] += 1
        z = ((status < 0) & refine & (k_ref >= n_refine)).nonzero().squeeze(1)
        th = ta[z] + ((tb[z] - ta[z]) * fa[z]) / (fa[z] - fb[z])
        ok = torch.isfinite(th)
        finish(z[ok], 1, th[ok])
        finish(z[~ok], 3, tb[z[~ok]])
        refine[z] = False
    return status, t_fin, n_eval


def alternate(fns, rounds=ROUNDS, warm=WARM):
    for _ in range(warm):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"min_ms": min(v), "median_ms": float(np.median(v)), "max_ms": max(v)} for k, v in ms.items()}


def fold_trace(out, trace_dir, stats_path):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    dur = []
    for path in files:
        with open(path) as f:
            for row in csv.DictReader(f):
                if KERNEL in row.get("Kernel_Name", ""):
                    dur.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if not dur:
        raise SystemExit("the trace holds no %s" % KERNEL)
    med = float(np.median(dur))
    evals = out["evaluations"]
    out["kernel_rocprofv3"] = {"launches": len(dur), "min_us": min(dur), "median_us": med, "max_us": max(dur),
                               "evaluations_per_s_at_median": evals / (med * 1e-6),
                               "fp32_tflops_at_median_arithmetic": evals * FLOP_PER_EVAL / (med * 1e-6) / 1e12}
    with open(stats_path, "w") as f:
        f.write("rocprofv3 --kernel-trace --stats -f csv -- python profiles/microbench/sdf_trace.py --load MODEL.pt --kernel-only   (a run of its own, one MI355X)\n")
        f.write("%d x %d rays on the trained example model (examples/train_surface.py at its defaults), default trace parameters; %d launches\n"
                % (WH, WH, len(dur)))
        f.write("the other kernels of the run (torch kernels that build the rays and the pack once) are left out\n\n")
        f.write("%-28s %6s %12s %10s %10s %10s\n" % ("kernel", "calls", "average_us", "min_us", "max_us", "stddev_us"))
        f.write("%-28s %6d %12.1f %10.1f %10.1f %10.1f\n" % (KERNEL, len(dur), float(np.mean(dur)), min(dur), max(dur), float(np.std(dur))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_trace.json"))
    ap.add_argument("--save", default=None, help="keep the trained model's state here")
    ap.add_argument("--load", default=None, help="a state kept by --save instead of training")
    ap.add_argument("--kernel-only", action="store_true", help="ten launches of the kernel and nothing else (the traced run)")
    ap.add_argument("--trace", default=None, help="fold the kernel trace under this directory into --out; runs nothing on the GPU")
    ap.add_argument("--stats", default=None, help="with --trace: where the stats text goes (default: next to --out)")
    args = ap.parse_args()
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    if args.trace is not None:
        fold_trace(out, args.trace, args.stats or os.path.join(os.path.dirname(os.path.abspath(args.out)), "sdf_trace_rocprofv3_stats.txt"))
        print(json.dumps(out["kernel_rocprofv3"], indent=1))
    else:
        if not torch.cuda.is_available():
            raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernel's time")
        from ngp_hip import ops
        from ngp_hip.surface import render_surface, render_surface_traced, trace_surface
        dev = torch.device("cuda")
        model, info = trained_model(args, dev)
        o, d = frame_rays(dev)
        wpack = model.packed_geometry()
        coarse = ops.coarse_bitfield(model.density_bitfield, model.cascades, model.grid_size)
        stats = torch.zeros(2, device=dev, dtype=torch.int64)
        kernel = lambda st=None: trace_surface(model, o, d, wpack=wpack, coarse=coarse, stats=st, **PARAMS)
        tr = kernel(stats)
        torch.cuda.synchronize()
        if args.kernel_only:
            for _ in range(10):
                kernel()
            torch.cuda.synchronize()
            out = {"launches": 11}
        else:
            with torch.no_grad():
                ts, tt, tn = torch_trace(model, o, d, **PARAMS)
                same = ts == tr["status"]
                both_hit = same & (tr["status"] == 1)
                dd = (tt - tr["t"])[both_hit].abs()
                events = alternate({"trace_surface": kernel,
                                    "render_surface_traced": lambda: render_surface_traced(model, o, d, **PARAMS),
                                    "render_surface_test_time": lambda: render_surface(model, o, d, test_time=True, chunk=WH * WH)})
                events.update(alternate({"torch_trace": lambda: torch_trace(model, o, d, **PARAMS)}, rounds=2, warm=0))   # seconds per call
            slots, used = (int(v) for v in stats.tolist())
            evals = int(tr["n_eval"].sum())
            out.update(what="one %d x %d frame of the trained example model: trace_surface (ngp_sdf_trace, one launch) against "
                            "render_surface(test_time=True) and against torch_trace, the same rule as a masked batched loop over model.sdf; HIP "
                            "events around each whole call, alternating, %d rounds after %d warm (torch_trace: 2 rounds on its own, after the call that is cross-checked); the kernel's own time from one rocprofv3 "
                            "--kernel-trace --stats run" % (WH, WH, ROUNDS, WARM),
                       rays=WH * WH, params=PARAMS, training=info, status_counts=[int((tr["status"] == k).sum()) for k in range(4)],
                       evaluations=evals, n_eval_mean=evals / (WH * WH), n_eval_max=int(tr["n_eval"].max()),
                       flop_per_evaluation_arithmetic=FLOP_PER_EVAL,
                       lane_slots_of_evaluation_rounds=slots, lane_slots_used=used, idle_share_of_evaluation_slots=1.0 - used / max(1, slots),
                       whole_call_events=events,
                       torch_trace_cross_check={"status_agrees": float(same.float().mean()), "rays_hit_by_both": int(both_hit.sum()),
                                                "depth_abs_diff_median": float(dd.median()) if dd.numel() else None,
                                                "depth_abs_diff_max": float(dd.max()) if dd.numel() else None,
                                                "n_eval_mean_torch": float(tn.float().mean())})
            e = events["trace_surface"]["median_ms"]
            out["evaluations_per_s_whole_call"] = evals / (e * 1e-3)
            out["speedup_over_torch_trace"] = events["torch_trace"]["median_ms"] / e
            out["speedup_over_render_surface_test_time"] = events["render_surface_test_time"]["median_ms"] / events["render_surface_traced"]["median_ms"]
            print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
