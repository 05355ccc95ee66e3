"""Frame time of the deployment renderer (ngp_hip/deploy.py) against the only path that could render a deployment model before it:
the same weights in NGP(**deployment config) through modules.rendering.render(test_time=True) (encoder kernel + torch layers).

    python profiles/microbench/deploy_render.py --out profiles/deploy_render.json
    rocprofv3 --kernel-trace --stats -d DIR -o shade -- python profiles/microbench/deploy_render.py --shade-loop 20      # a run of its own
    python profiles/microbench/deploy_render.py --out profiles/deploy_render.json --rocprof-stats DIR/.../shade_kernel_stats.csv
    python profiles/microbench/deploy_render.py --fused --out profiles/deploy_render_fused.json       # mode="fused" against one-shot
    rocprofv3 --kernel-trace --stats -d DIR -o fused -- python profiles/microbench/deploy_render.py --fused-loop 20     # a run of its own

The model is the trained one of examples/render_deployment.py (procedural scene), so rays terminate as in a real scene.  Per size
(300x600, 800x800): warm, five frames, HIP events around the whole frame (rays, slab test, march, shade, composite), minimum and
spread; samples per frame; the shade kernel alone on the frame's samples (events, and rocprofv3's own figure when given); and that time
against the floor of 512 B per sample at 8.6 TB/s, the rate uniformly random rows of a 38 MB table are gathered at from the Infinity
Cache (1152-byte rows; 16-byte rows of 64-byte lines cannot reach it, so the floor is a floor).

--fused: mode="fused" (one launch per frame: ngp_deploy_render) and one-shot ALTERNATING in one process on the same model, per size warm
frames and then seven timed frames each, HIP events around the whole frame; minimum and spread of both, the fused kernel alone (events),
its floor (composited samples x 512 B at 8.6 TB/s) and the lane utilisation of its mapping, replayed on the host from the frame's per-ray
counts (lane_utilisation below): composited samples / (64 x shade iterations)."""
import argparse
import csv
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

GATHER_BYTES_PER_SAMPLE = 512
INFINITY_CACHE_GATHER_BPS = 8.6e12
SIZES = ((300, 600), (800, 800))


def example():
    spec = importlib.util.spec_from_file_location("render_deployment_example", os.path.join(ROOT, "examples", "render_deployment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, warm=2, runs=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "runs_ms": ms}


def frame_samples(m, pose, res):
    """The samples of one frame as the one-shot renderer marches them."""
    from ngp_hip import ops
    from ngp_hip.deploy import get_directions
    from ngp_hip.rays import get_rays
    dev = m.device
    d = torch.from_numpy(get_directions(*res)).to(dev)
    o, r = get_rays(d, torch.as_tensor(pose).float().to(dev))
    hits = ops.ray_aabb(o, r, 0.5)
    xs, ds = [], []
    for a in range(0, o.shape[0], 65536):
        b = min(a + 65536, o.shape[0])
        _, xyzs, dirs, _, _, _ = ops.march_train(o[a:b], r[a:b], hits[a:b].contiguous(), m._tensors()[3], torch.zeros(b - a, device=dev), 1, 0.5,
                                                 0.0, 128, 1024)
        xs.append(xyzs); ds.append(dirs)
    return torch.cat(xs), torch.cat(ds)


def lane_utilisation(n_samples, group=64, queue=32):
    """Replay of the fused kernel's mapping on one frame's per-ray counts.  A wave owns `group` consecutive rays; per iteration each of
    its L rays that still has samples gets group // L slots (at most the `queue` positions a ray queues ahead), and an iteration with any sample in it costs one shade pass of 64 lanes.
    (The replay takes a ray for alive until its last composited sample: what the kernel shades behind a ray's termination point and the
    slots of rays that are still searching for a sample they will not find are not in the per-ray counts.)  Also the figure of the
    plain mapping without slot sharing -- one sample per alive ray and iteration, i.e. the longest ray's count per wave."""
    c = n_samples.to(torch.int64)
    pad = (-c.shape[0]) % group
    if pad:
        c = torch.cat([c, c.new_zeros(pad)])
    rem = c.reshape(-1, group).clone()
    plain = int(rem.max(1).values.sum())
    iters = torch.zeros(rem.shape[0], dtype=torch.int64, device=rem.device)
    longest = 0
    while True:
        alive = rem > 0
        n_alive = alive.sum(1)
        if not bool(n_alive.any()):
            break
        quota = group // n_alive.clamp(min=1)
        rem = rem - torch.minimum(rem, quota.clamp(max=queue)[:, None])
        iters += (n_alive > 0).to(torch.int64)
        longest += 1
    total = int(c.sum())
    return {"composited_samples": total, "shade_iterations": int(iters.sum()), "longest_wave_iterations": longest,
            "longest_ray_samples": int(c.max()), "waves": int(rem.shape[0]), "waves_without_samples": int((iters == 0).sum()),
            "lane_utilisation": total / max(1, group * int(iters.sum())),
            "without_slot_sharing": {"shade_iterations": plain, "lane_utilisation": total / max(1, group * plain)}}


def fused(args, m, pose, dev):
    from ngp_hip import ops
    from ngp_hip.deploy import get_directions
    from ngp_hip.rays import get_rays
    pose = torch.as_tensor(pose).float().to(dev)
    if args.fused_loop:
        d = torch.from_numpy(get_directions(*SIZES[-1])).to(dev)
        for _ in range(args.fused_loop):
            frame = m.render(pose, directions=d, T_threshold=1e-2, max_samples=1024, mode="fused")
        torch.cuda.synchronize()
        print(json.dumps({"fused_loop": args.fused_loop, "composited_samples": int(frame["total_samples"])}))
        return
    out = {"what": "DeployedModel.render(mode='fused') (get_rays + ONE launch, ngp_deploy_render) against mode='oneshot', alternating in one process",
           "T_threshold": 1e-2, "max_samples": 1024, "frames_each": args.frames, "mapping": "64 consecutive rays per wave; the L rays still alive share the wave's 64 slots, 64 // L samples each per round (at most what it has queued); every ray queues up to 32 sample positions ahead",
           "floor": "512 B per composited sample at 8.6 TB/s (Infinity-Cache gather rate of 1152-byte rows)", "sizes": {}}
    for res in SIZES:
        d = torch.from_numpy(get_directions(*res)).to(dev)
        modes = {"oneshot": lambda: m.render(pose, directions=d, T_threshold=1e-2, max_samples=1024),
                 "fused": lambda: m.render(pose, directions=d, T_threshold=1e-2, max_samples=1024, mode="fused")}
        for _ in range(3):
            for fn in modes.values():
                fn()
        ms = {k: [] for k in modes}
        for _ in range(args.frames):
            for k, fn in modes.items():                                     # alternating: both see the same clocks and caches
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms[k].append(a.elapsed_time(b))
        st = {k: {"min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v), "runs_ms": v} for k, v in ms.items()}
        one, fu = modes["oneshot"](), modes["fused"]()
        o, r = get_rays(d, pose)
        table, sw, rw, bits = m._tensors()
        kern = timed(lambda: ops.deploy_render(o, r, bits, m._coarse_table(), table, m.levels, sw, rw, 1e-2, 1024), runs=args.frames)
        util = lane_utilisation(fu["n_samples"])
        floor_us = util["composited_samples"] * GATHER_BYTES_PER_SAMPLE / INFINITY_CACHE_GATHER_BPS * 1e6
        spread = max(st["oneshot"]["spread_ms"], st["fused"]["spread_ms"])
        entry = {"rays": res[0] * res[1], "oneshot": st["oneshot"], "fused": st["fused"], "speedup": st["oneshot"]["min_ms"] / st["fused"]["min_ms"],
                 "faster_by_more_than_the_spread": bool(st["oneshot"]["min_ms"] - st["fused"]["min_ms"] > spread),
                 "composited_samples_oneshot": int(one["total_samples"]), "max_abs_rgb_difference": float((one["rgb"] - fu["rgb"]).abs().max()),
                 "max_abs_opacity_difference": float((one["opacity"] - fu["opacity"]).abs().max()),
                 "fused_kernel_events": kern, "fused_floor_us": floor_us, "fused_kernel_over_floor": kern["min_ms"] * 1e3 / floor_us}
        entry.update(util)
        out["sizes"]["%dx%d" % res] = entry
        print("%dx%d: fused %.3f ms (spread %.3f) vs one-shot %.3f ms (spread %.3f): x%.2f; kernel %.1f us = %.1f x floor; lane utilisation %.3f" % (
            res[0], res[1], st["fused"]["min_ms"], st["fused"]["spread_ms"], st["oneshot"]["min_ms"], st["oneshot"]["spread_ms"], entry["speedup"],
            kern["min_ms"] * 1e3, entry["fused_kernel_over_floor"], util["lane_utilisation"]))
    if args.rocprof_stats:
        with open(args.rocprof_stats) as f:
            rows = [r for r in csv.DictReader(f) if "deploy_render_kernel" in r.get("Name", "")]
        if rows:
            r = rows[0]
            avg_us = float(r["AverageNs"]) / 1e3
            out["fused_kernel_rocprofv3"] = {"size": "%dx%d" % SIZES[-1], "calls": int(r["Calls"]), "average_us": avg_us, "min_us": float(r["MinNs"]) / 1e3,
                                             "over_floor": avg_us / out["sizes"]["%dx%d" % SIZES[-1]]["fused_floor_us"]}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train_steps", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deploy_render.json"))
    ap.add_argument("--shade-loop", type=int, default=0, help="only launch the shade kernel this many times on an 800x800 frame's samples")
    ap.add_argument("--rocprof-stats", default=None, help="kernel stats CSV of a --shade-loop run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--fused", action="store_true", help="measure mode='fused' against one-shot, alternating (write it to --out)")
    ap.add_argument("--fused-loop", type=int, default=0, help="only render this many 800x800 frames in fused mode (for rocprofv3)")
    ap.add_argument("--frames", type=int, default=7, help="timed frames per mode and size of --fused")
    args = ap.parse_args()
    from modules.rendering import render
    from ngp_hip.deploy import DeployedModel, get_directions
    from ngp_hip.rays import get_rays
    dev = torch.device("cuda")
    ex = example()
    model, poses, _, losses = ex.train_deployment_model(args.train_steps, dev)
    model.eval()
    m = DeployedModel.from_module(model)
    pose = poses[min(20, len(poses) - 1)]

    if args.fused or args.fused_loop:
        return fused(args, m, pose, dev)

    if args.shade_loop:
        xyzs, dirs = frame_samples(m, pose, SIZES[-1])
        for _ in range(args.shade_loop):
            m.shade(xyzs, dirs)
        torch.cuda.synchronize()
        print(json.dumps({"shade_loop": args.shade_loop, "samples": int(xyzs.shape[0])}))
        return

    out = {"what": "deployment model rendered by ngp_hip.deploy (one-shot) vs the same weights through modules.rendering.render(test_time=True)",
           "model": "NGP(**DEPLOYMENT_CONFIG) trained %d steps on the procedural scene; loss %.5f -> %.5f" % (
               args.train_steps, float(losses[:10].mean()), float(losses[-10:].mean())),
           "T_threshold": 1e-2, "max_samples": 1024, "floor": "512 B per sample at 8.6 TB/s (Infinity-Cache gather rate of 1152-byte rows)",
           "sizes": {}}
    for res in SIZES:
        d = torch.from_numpy(get_directions(*res)).to(dev)

        def parent(autocast):
            o, r = get_rays(d, pose)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                return render(model, o, r, test_time=True, exp_step_factor=0, T_threshold=1e-2, max_samples=1024)

        new = timed(lambda: m.render(pose, directions=d, T_threshold=1e-2, max_samples=1024))
        old32 = timed(lambda: parent(False))
        old16 = timed(lambda: parent(True))
        frame = m.render(pose, directions=d, T_threshold=1e-2, max_samples=1024)
        ref = parent(False)
        xyzs, dirs = frame_samples(m, pose, res)
        shade = timed(lambda: m.shade(xyzs, dirs))
        n = int(xyzs.shape[0])
        floor_us = n * GATHER_BYTES_PER_SAMPLE / INFINITY_CACHE_GATHER_BPS * 1e6
        best_old = min(old32["min_ms"], old16["min_ms"])
        entry = {"rays": res[0] * res[1], "marched_samples": n, "composited_samples": int(frame["total_samples"]),
                 "deploy_render": new, "modules_render_fp32": old32, "modules_render_autocast_fp16": old16,
                 "speedup_vs_faster_parent_path": best_old / new["min_ms"],
                 "faster_by_more_than_the_spread": bool(best_old - new["min_ms"] > max(new["spread_ms"], old32["spread_ms"], old16["spread_ms"])),
                 "max_abs_rgb_difference_vs_fp32_parent": float((frame["rgb"] + (1 - frame["opacity"])[:, None] - ref["rgb"]).abs().max()),
                 "shade_kernel_events": shade, "shade_floor_us": floor_us, "shade_events_over_floor": shade["min_ms"] * 1e3 / floor_us,
                 "shade_Gsamples_per_s_events": n / shade["min_ms"] / 1e6}
        out["sizes"]["%dx%d" % res] = entry
        print("%dx%d: %.3f ms vs %.3f / %.3f ms (x%.2f), %d samples, shade %.1f us = %.2f x floor" % (
            res[0], res[1], new["min_ms"], old32["min_ms"], old16["min_ms"], entry["speedup_vs_faster_parent_path"], n, shade["min_ms"] * 1e3,
            entry["shade_events_over_floor"]))
    if args.rocprof_stats:
        with open(args.rocprof_stats) as f:
            rows = [r for r in csv.DictReader(f) if "deploy_shade_kernel" in r.get("Name", "")]
        if rows:
            r = rows[0]
            avg_us = float(r["AverageNs"]) / 1e3
            e = out["sizes"]["%dx%d" % SIZES[-1]]
            out["shade_kernel_rocprofv3"] = {"size": "%dx%d" % SIZES[-1], "calls": int(r["Calls"]), "average_us": avg_us, "min_us": float(r["MinNs"]) / 1e3,
                                             "over_floor": avg_us / e["shade_floor_us"], "Gsamples_per_s": e["marched_samples"] / avg_us / 1e3}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
