"""Time and accuracy of the hash encoder's position-gradient kernel (csrc/hash_grad_input.hip) on the MI355X, recorded in
profiles/hash_input_grad.json.

    python profiles/microbench/hash_input_grad.py --out profiles/hash_input_grad.json
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o hgi -- python profiles/microbench/hash_input_grad.py --loop 20   # a run of its own
    python profiles/microbench/hash_input_grad.py --out profiles/hash_input_grad.json --merge-rocprof DIR/.../hgi_kernel_trace.csv

Timing: ngp_hash_bwd_input_f32 against ngp_hash_fwd_f32 on the same samples and the same table -- the forward gathers the same bytes
(8 corners x 8 B x 16 levels per sample), so it is what the new kernel should cost.  The samples are ray-ordered samples of the
procedural scene: an NGP is trained briefly on it (examples/render_normals.py's schedule) for its occupancy grid and its table, 16384
rays of synthetic.lego_rays are marched with zero noise and the first 360 000 samples are kept (the bench's live-sample count per
step).  Both kernels are warmed, then timed ALTERNATING with HIP events, 20 rounds; minimum, median and spread of each and their ratio.
The bf16 and f16 entries are timed the same way against their forwards.
Accuracy: the figures tests/test_gpu_hash_input_grad.py asserts on, on its inputs: per (level table, entry) the serial-float32 error
E32 of the reference and the kernel's worst |gpu - dx64| / (E32 S) over n in {1, 63, 64, 65, 1000} (the test's bound is 4)."""
import argparse
import csv
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_SAMPLES = 360_000
ROUNDS = 20
BYTES_PER_SAMPLE = {"f32": 16 * (8 * 8 + 8) + 12 + 12, "bf16": 16 * (8 * 4 + 8) + 12 + 12, "f16": 16 * (8 * 4 + 4) + 12 + 12}


def scene_samples(train_steps, dev):
    """(model, x01 [N_SAMPLES or fewer, 3]): ray-ordered sample positions of the procedural scene in the encoder's [0, 1] frame."""
    from modules.networks import NGP
    from modules.rendering import MAX_SAMPLES
    from ngp_hip import ops, synthetic
    spec = importlib.util.spec_from_file_location("render_normals_example", os.path.join(ROOT, "examples", "render_normals.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    torch.manual_seed(23)
    model = NGP(scale=0.5).to(dev)
    wh, focal = 100, 1111.1 * 100 / 800
    poses = ex.cameras(40, 1.39, 23, dev)
    K = torch.tensor([[focal, 0, wh / 2], [0, focal, wh / 2], [0, 0, 1]], device=dev)
    model.mark_invisible_cells(K, poses, (wh, wh))
    ex.train(model, train_steps, poses, ex.pixel_dirs(wh, focal, dev))
    o, d = synthetic.lego_rays(16384, seed=23)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    hits = ops.ray_aabb(o, d, 0.5)
    _, xyzs, _, _, _, _ = ops.march_train(o, d, hits, model.density_bitfield, torch.zeros(o.shape[0], device=dev), model.cascades, 0.5, 0.0,
                                          model.grid_size, MAX_SAMPLES)
    x01 = ((xyzs[:N_SAMPLES] + 0.5).clamp(0, 1)).contiguous()
    return model, x01, int(xyzs.shape[0])


def pairs(model, x01):
    """entry -> (forward, position gradient) closures on the same samples and table."""
    from ngp_hip import ops
    lv = model.pos_encoder.levels_struct
    n = x01.shape[0]
    table = model.pos_encoder.hash_table.detach().contiguous()
    g = torch.Generator(x01.device).manual_seed(1)
    denc = torch.randn(n, 32, device=x01.device, generator=g)
    t_bf, t_h, denc_h = table.bfloat16(), table.half().reshape(-1, 2), denc.half().reshape(n, 16, 2)
    return {"f32": (lambda: ops.hash_fwd_f32(x01, table, lv), lambda: ops.hash_bwd_input_f32(x01, table, denc, lv)),
            "bf16": (lambda: ops.hash_fwd_bf16(x01, t_bf, lv), lambda: ops.hash_bwd_input_bf16(x01, t_bf, denc, lv)),
            "f16": (lambda: ops.hash_fwd_f16(x01, t_h, lv), lambda: ops.hash_bwd_input_f16(x01, t_h, denc_h, lv))}


def alternate(fwd, bwd, rounds=ROUNDS, warm=5):
    for _ in range(warm):
        fwd(); bwd()
    ms = {"forward": [], "position_gradient": []}
    for _ in range(rounds):
        for k, fn in (("forward", fwd), ("position_gradient", bwd)):          # alternating: both see the same clocks and caches
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) * 1e3)
    out = {k: {"min_us": min(v), "median_us": float(np.median(v)), "max_us": max(v), "spread_us": max(v) - min(v)} for k, v in ms.items()}
    out["ratio_of_minima"] = out["position_gradient"]["min_us"] / out["forward"]["min_us"]
    out["ratio_of_medians"] = out["position_gradient"]["median_us"] / out["forward"]["median_us"]
    return out


def accuracy():
    import test_gpu_hash_input_grad as t
    rows = {}
    for shape, kind in t.CASES:
        c = t._input(shape, kind)
        worst = 0.0
        for n in t.NS:
            got = t._run(kind, c["x"][:n], c["table"], c["denc"][:n], c["lv"]).cpu().numpy().astype(np.float64)
            r = c["rows"][:n]
            worst = max(worst, float(np.max(np.abs(got[r] - c["dx64"][:n][r]) / (c["e32"] * c["S"][:n][r]))))
        rows["%s/%s" % (shape, kind)] = {"levels": list(t.SHAPES[shape]), "E32": c["e32"], "worst_error_over_E32_S": worst, "bound": 4.0}
    return rows


KERNELS = ("hash_bwd_input_kernel", "hash_fwd_f32_xcd_kernel")


def merge_rocprof(path, out_path, last):
    """Add rocprofv3's per-kernel figures to --out.  `path` is the kernel TRACE of a --loop run (the last `last` dispatches of each of
    the two kernels: the training that prepares the table launches the forward too, so whole-run statistics would mix them) or, for
    kernels only the loop launches, the kernel stats CSV."""
    out = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            out = json.load(f)
    with open(path) as f:
        rows = list(csv.DictReader(f))
    stats = []
    if rows and "Kernel_Name" in rows[0]:
        for k in KERNELS:
            d = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if k in r["Kernel_Name"])[-last:]
            us = [(b - a) / 1e3 for a, b in d]
            if us:
                stats.append({"kernel": k, "calls": len(us), "average_us": sum(us) / len(us), "min_us": min(us), "max_us": max(us),
                              "source": "kernel trace, last %d dispatches" % last})
    else:
        for r in rows:
            if any(k in r.get("Name", "") for k in KERNELS):
                stats.append({"kernel": r["Name"][:120], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
                              "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3, "source": "kernel stats, whole run"})
    out["rocprofv3_kernel_stats"] = stats
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("merged", len(stats), "kernel rows into", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_input_grad.json"))
    ap.add_argument("--train_steps", type=int, default=256)
    ap.add_argument("--loop", type=int, default=0, help="only launch the f32 forward and position gradient this many times (for rocprofv3)")
    ap.add_argument("--merge-rocprof", default=None, help="kernel trace (or stats) CSV of a --loop run under rocprofv3: add it to --out (no GPU work)")
    ap.add_argument("--last", type=int, default=20, help="--merge-rocprof on a trace: the dispatches per kernel that belong to the loop")
    args = ap.parse_args()
    if args.merge_rocprof:
        return merge_rocprof(args.merge_rocprof, args.out, args.last)
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernel's time")
    dev = torch.device("cuda")
    model, x01, marched = scene_samples(args.train_steps, dev)
    p = pairs(model, x01)
    if args.loop:
        for _ in range(args.loop):
            p["f32"][0](); p["f32"][1]()
        torch.cuda.synchronize()
        print(json.dumps({"loop": args.loop, "samples": int(x01.shape[0])}))
        return
    n = int(x01.shape[0])
    out = {"what": "ngp_hash_bwd_input_* (position gradient of the hash encoder) against the forward on the same samples and table, HIP events, "
                   "alternating, %d rounds after 5 warm ones" % ROUNDS,
           "samples": n, "marched_samples_of_16384_rays": marched,
           "scene": "procedural scene, NGP trained %d steps for occupancy grid and table; zero-noise march, ray order" % args.train_steps,
           "levels": "L 16, F 2, log2_T 19, base 16, max 2048", "mapping": "one lane per (sample, level), level fastest; 16-lane xor-shuffle tree",
           "timing": {}, "accuracy": accuracy()}
    for kind, (fwd, bwd) in p.items():
        t = alternate(fwd, bwd)
        t["bytes_per_sample"] = BYTES_PER_SAMPLE[kind]
        t["position_gradient_GB_per_s"] = n * BYTES_PER_SAMPLE[kind] / t["position_gradient"]["min_us"] / 1e3
        out["timing"][kind] = t
        print("%s: forward %.1f us, position gradient %.1f us (x%.2f), spreads %.1f / %.1f us" % (
            kind, t["forward"]["min_us"], t["position_gradient"]["min_us"], t["ratio_of_minima"], t["forward"]["spread_us"],
            t["position_gradient"]["spread_us"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
