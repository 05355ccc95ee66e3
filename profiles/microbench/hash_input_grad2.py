"""Time and accuracy of the hash encoder's double-backward kernels (csrc/hash_grad_input2.hip) on the MI355X, recorded in
profiles/hash_input_grad2.json.

    python profiles/microbench/hash_input_grad2.py --out profiles/hash_input_grad2.json

Timing: on the 360 000 ray-ordered samples and the default level table of profiles/microbench/hash_input_grad.py (same scene, same
brief training, same march), HIP events, alternating, 20 rounds after 5 warm ones:
    ngp_hash_bwd2_gather_f32 (both outputs, and each alone)   against   ngp_hash_bwd_input_f32, the first-order gather;
    ngp_hash_bwd2_gather_bf16                                  against   ngp_hash_bwd_input_bf16;
    ngp_hash_bwd2_table_f32                                    against   ngp_hash_bwd_f32's float-atomic form (ngp_hash_bwd_f32 called
                                                                         directly: the operator would route this size to the LDS-sliced form).
Both scatters add into the same preallocated buffer; it is not cleared between launches (the sums grow, the work does not change).
There is no bar: the times and the ratio to the first-order kernels are recorded.
Accuracy: the figures tests/test_gpu_hash_input_grad2.py asserts on, on its inputs -- per (level table, kind) the serial-float32 error
E32 of the reference and the kernels' worst |gpu - ref64| / (E32 S) (bound 4), and the end-to-end eikonal-loss ratios (bound 4)."""
import argparse
import ctypes
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

ROUNDS = 20
BYTES_PER_SAMPLE = {"gather_f32": 16 * (8 * 8 + 8 + 8) + 12 + 12 + 12, "gather_bf16": 16 * (8 * 4 + 8 + 8) + 12 + 12 + 12,
                    "first_order_f32": 16 * (8 * 8 + 8) + 12 + 12, "first_order_bf16": 16 * (8 * 4 + 8) + 12 + 12}


def _first_order_bench():
    spec = importlib.util.spec_from_file_location("hash_input_grad_bench", os.path.join(ROOT, "profiles", "microbench", "hash_input_grad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def alternate(first, second, rounds=ROUNDS, warm=5):
    for _ in range(warm):
        first(); second()
    ms = {"first_order": [], "second_order": []}
    for _ in range(rounds):
        for k, fn in (("first_order", first), ("second_order", second)):          # alternating: both see the same clocks and caches
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) * 1e3)
    out = {k: {"min_us": min(v), "median_us": float(np.median(v)), "max_us": max(v), "spread_us": max(v) - min(v)} for k, v in ms.items()}
    out["ratio_of_minima"] = out["second_order"]["min_us"] / out["first_order"]["min_us"]
    out["ratio_of_medians"] = out["second_order"]["median_us"] / out["first_order"]["median_us"]
    return out


def pairs(model, x01):
    """name -> (first-order kernel, double-backward kernel) closures on the same samples and table.  The closures call the C entries
    on preallocated outputs, so a timed interval holds the kernel and nothing else."""
    from ngp_hip import lib, ops
    L = lib.load()
    lv = model.pos_encoder.levels_struct
    n = x01.shape[0]
    dev = x01.device
    table = model.pos_encoder.hash_table.detach().contiguous()
    t_bf = table.bfloat16()
    g = torch.Generator(dev).manual_seed(1)
    denc = torch.randn(n, 32, device=dev, generator=g)
    ddx = torch.randn(n, 3, device=dev, generator=g)
    dx, d_x, d_denc = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, 32, device=dev)
    dt1, dt2 = torch.zeros_like(table), torch.zeros_like(table)
    P, S, LV = ops._ptr, ops._stream, ctypes.byref(lv)

    def call(name, *a):
        lib.check(getattr(L, name)(*a, S()), name)

    first_f32 = lambda: call("ngp_hash_bwd_input_f32", P(x01), P(table), P(denc), LV, n, P(dx))
    first_bf16 = lambda: call("ngp_hash_bwd_input_bf16", P(x01), P(t_bf), P(denc), LV, n, P(dx))
    return {
        "gather_f32": (first_f32, lambda: call("ngp_hash_bwd2_gather_f32", P(x01), P(table), P(denc), P(ddx), LV, n, P(d_denc), P(d_x))),
        "gather_f32_d_denc_only": (first_f32, lambda: call("ngp_hash_bwd2_gather_f32", P(x01), P(table), P(denc), P(ddx), LV, n, P(d_denc), P(None))),
        "gather_f32_d_x_only": (first_f32, lambda: call("ngp_hash_bwd2_gather_f32", P(x01), P(table), P(denc), P(ddx), LV, n, P(None), P(d_x))),
        "gather_bf16": (first_bf16, lambda: call("ngp_hash_bwd2_gather_bf16", P(x01), P(t_bf), P(denc), P(ddx), LV, n, P(d_denc), P(d_x))),
        "scatter_f32": (lambda: call("ngp_hash_bwd_f32", P(x01), P(denc), LV, n, P(dt1)),
                        lambda: call("ngp_hash_bwd2_table_f32", P(x01), P(denc), P(ddx), LV, n, P(dt2))),
    }


def accuracy():
    import test_gpu_hash_input_grad2 as t
    out = {"gather": {}, "scatter": {}, "end_to_end_eikonal": {}}
    for shape, kind in t.CASES:
        out["gather"]["%s/%s" % (shape, kind)] = dict(t.gather_figures(shape, kind), levels=list(t.t1.SHAPES[shape]))
    for shape in t.TABLES:
        out["scatter"][shape] = dict(t.scatter_figures(shape), levels=list(t.t1.SHAPES[shape]))
    for shape in ("tiny", "default"):
        out["end_to_end_eikonal"][shape] = t.e2e_figures(shape)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_input_grad2.json"))
    ap.add_argument("--train_steps", type=int, default=256)
    ap.add_argument("--no-accuracy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernels' time")
    dev = torch.device("cuda")
    model, x01, marched = _first_order_bench().scene_samples(args.train_steps, dev)
    n = int(x01.shape[0])
    out = {"what": "ngp_hash_bwd2_* (double backward of the hash encoder through its position gradient) against the first-order kernels on "
                   "the same samples and table, HIP events, alternating, %d rounds after 5 warm ones" % ROUNDS,
           "samples": n, "marched_samples_of_16384_rays": marched,
           "scene": "procedural scene, NGP trained %d steps for occupancy grid and table; zero-noise march, ray order" % args.train_steps,
           "levels": "L 16, F 2, log2_T 19, base 16, max 2048",
           "mapping": "gather: one lane per (sample, level), level fastest, 16-lane xor-shuffle tree for d_x; scatter: lane quads on one "
                      "64-byte line, 16 samples x one level per wave, segmented scan over equal-cell runs, float atomics",
           "timing": {}}
    for name, (first, second) in pairs(model, x01).items():
        t = alternate(first, second)
        kind = "bf16" if name.endswith("bf16") else "f32"
        if name in ("gather_f32", "gather_bf16"):
            t["bytes_per_sample"] = BYTES_PER_SAMPLE[name]
            t["second_order_GB_per_s"] = n * BYTES_PER_SAMPLE[name] / t["second_order"]["min_us"] / 1e3
            t["first_order_bytes_per_sample"] = BYTES_PER_SAMPLE["first_order_" + kind]
        out["timing"][name] = t
        print("%s: first order %.1f us, double backward %.1f us (x%.2f), spreads %.1f / %.1f us" % (
            name, t["first_order"]["min_us"], t["second_order"]["min_us"], t["ratio_of_minima"], t["first_order"]["spread_us"],
            t["second_order"]["spread_us"]), flush=True)
    del model
    if not args.no_accuracy:
        out["accuracy"] = accuracy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
