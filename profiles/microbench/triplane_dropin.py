"""Tri-plane drop-in training throughput: NGP(scale=0.5, pos_encoder_type='triplane', max_res=1024) on the trained-Lego occupancy grid
(tests/golden/lego_density_bitfield.npz) with procedural Lego rays, trained the way train.py does (render + compat FusedAdam +
GradScaler under autocast fp16).  Prints ONE JSON line: rays/s at 8192 rays per step, plus the float-atomic bytes per live sample of
the backward, counted by replaying the kernel's merge rule (LDS levels: one add per touched float per workgroup; other levels: one add
per run of equal destinations within a wave of 64) on one step's samples.
    python profiles/microbench/triplane_dropin.py [--steps 60] [--warmup 10] [--rays 8192]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd"), os.path.join(ROOT, "taichi-nerfs_amd", "compat")):
    sys.path.insert(0, p)


def atomic_bytes_per_sample(x01, lv, threads=512, max_blocks=512):
    """Replay of triplane_bwd_kernel's atomic count (all rows live)."""
    n = x01.shape[0]
    M = lv.max_res
    res = list(lv.resolution[:lv.n_levels])
    budget, used, lds_levels = 20480, 0, 0
    for r in res:
        need = 3 * (r + 1) ** 2 * 4
        if used + need > budget:
            break
        used += need
        lds_levels += 1
    blocks = min((n + threads - 1) // threads, max_blocks)
    stride = blocks * threads
    block_of = (np.arange(n) % stride) // threads
    wave_of = np.arange(n) // 64
    adds = 0
    for l, r in enumerate(res):
        pos = x01 * np.float32(r - 1) + np.float32(0.5)
        g = np.floor(pos).astype(np.int64)
        for p in range(3):
            a, b = p, (p + 1) % 3
            for c in range(4):
                ga, gb = g[:, a] + (c & 1), g[:, b] + (c >> 1)
                if l < lds_levels:
                    key = (block_of * 3 + p) * (r + 1) ** 2 + gb * (r + 1) + ga
                    adds += 4 * len(np.unique(key))
                else:
                    oa = ((ga.astype(np.float32) / np.float32(r)) * np.float32(M - 1)).astype(np.int64)
                    ob = ((gb.astype(np.float32) / np.float32(r)) * np.float32(M - 1)).astype(np.int64)
                    key = oa + ob * M
                    head = np.ones(n, bool)
                    head[1:] = (key[1:] != key[:-1]) | (wave_of[1:] != wave_of[:-1])
                    adds += 4 * int(head.sum())
    return 4.0 * adds / n, lds_levels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rays", type=int, default=8192)
    args = ap.parse_args()
    import apex
    from modules.networks import NGP
    from modules.rendering import render
    from ngp_hip import lib, synthetic
    lib.build()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = NGP(scale=0.5, pos_encoder_type="triplane", max_res=1024).to(dev)
    bits = np.load(os.path.join(ROOT, "tests", "golden", "lego_density_bitfield.npz"))["density_bitfield"]
    model.density_bitfield.copy_(torch.from_numpy(bits).to(dev))
    opt = apex.optimizers.FusedAdam(model.parameters(), lr=1e-2, eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**19)
    batches = []
    for s in range(8):
        o, d = synthetic.lego_rays(args.rays, seed=s)
        batches.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), torch.rand(args.rays, 3, device=dev)))

    def step(i):
        o, d, target = batches[i % len(batches)]
        with torch.autocast("cuda", dtype=torch.float16):
            res = render(model, o, d, exp_step_factor=0.0)
            loss = torch.nn.functional.mse_loss(res["rgb"], target)
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return res

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # one step's samples for the atomic-byte replay (ray order, normalised to [0, 1] as the kernel does)
    from ngp_hip import ops
    o, d, _ = batches[0]
    hits = ops.ray_aabb(o, d, 0.5)
    _, xyzs, *_ = ops.march_train(o, d, hits, model.density_bitfield, torch.rand(args.rays, device=dev), 1, 0.5, 0.0, 128, 1024)
    x01 = np.clip((xyzs.cpu().numpy() + np.float32(0.5)) / np.float32(1.0), 0, 1).astype(np.float32)
    bps, lds_levels = atomic_bytes_per_sample(x01, model.pos_encoder.levels_struct)
    print(json.dumps({"metric": "triplane_dropin_rays_per_sec", "rays_per_sec": args.rays * args.steps / dt, "rays": args.rays,
                      "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
                      "replay_samples": int(x01.shape[0]),
                      "bwd_atomic_bytes_per_sample": bps, "naive_atomic_bytes_per_sample": 8 * 12 * 4 * 4, "lds_levels": lds_levels,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
