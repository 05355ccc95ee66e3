"""Voxel-grid (model_name='svox') drop-in training throughput: MODEL_DICT['svox'] at the driver's defaults (scale 0.5, degree 2,
G = 256, radius 0.0125) trained the way train.py does (render + compat FusedAdam + GradScaler under autocast fp16), 8192 rays per
step with procedural Lego rays.  The occupancy grid is the trained-Lego 128^3 bitfield (tests/golden/lego_density_bitfield.npz)
refined to 256^3 (every cell's eight children inherit its bit).  Prints ONE JSON line: rays/s, and the per-step split between the
forward (march + voxel_fwd + composite), the backward (composite bwd + gradient zero-fill + voxel_bwd), the zero-fill alone and the
optimizer step (dense Adam over both fields), from CUDA events.
`--trilinear` runs the model with use_trilinear=True (the eight-corner lookup) instead of the nearest voxel.
    python profiles/microbench/voxel_dropin.py [--steps 30] [--warmup 5] [--rays 8192] [--trilinear]"""
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


def refined_lego_bitfield(dev, G=256):
    from ngp_hip import ops
    bits128 = np.load(os.path.join(ROOT, "tests", "golden", "lego_density_bitfield.npz"))["density_bitfield"]
    occ128 = torch.from_numpy(np.unpackbits(bits128, bitorder="little").astype(np.uint8)).to(dev)
    coords = ops.morton3d_invert(torch.arange(G**3, device=dev, dtype=torch.int32))
    parent = ops.morton3d((coords // 2).contiguous().int())
    occ = occ128[parent.long()].reshape(-1, 8).to(torch.int32)
    weights = (2 ** torch.arange(8, device=dev, dtype=torch.int32))
    return (occ * weights).sum(1).to(torch.uint8)


def atomic_bytes_per_sample(xyzs, model):
    """Replay of the backward's merge rule on one step's samples (every sample taken as contributing): a wave of 64 consecutive samples
    issues one add per channel of every run of equal rows (nearest) or, trilinear, of every valid corner of every run of equal base
    cells.  Returns (bytes per sample, samples per run)."""
    G, W = model.grid_size, 3 * model.sh_dim + 1
    u = (xyzs.float() - np.float32(model.grid_min)) / np.float32(model.grid_radius)
    if model.use_trilinear:
        ok = ((u >= -1) & (u < G)).all(1)
        b = torch.floor(u).long()
        key = ((b[:, 0] + 1) * (G + 1) + b[:, 1] + 1) * (G + 1) + b[:, 2] + 1
        corners = ((b >= 0).long() + (b + 1 < G).long()).prod(1)
    else:
        b = torch.round(u).long()
        ok = ((b >= 0) & (b < G)).all(1)
        key = (b[:, 0] * G + b[:, 1]) * G + b[:, 2]
        corners = torch.ones_like(key)
    key = torch.where(ok, key, torch.full_like(key, -1))
    lane = torch.arange(key.numel(), device=key.device) % 64
    head = ((lane == 0) | (key != torch.roll(key, 1))) & (key >= 0)
    return float(corners[head].sum()) * W * 4 / key.numel(), float(ok.sum()) / max(int(head.sum()), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--trilinear", action="store_true")
    args = ap.parse_args()
    import apex
    from modules.networks import MODEL_DICT
    from modules.rendering import render
    from ngp_hip import lib, synthetic
    lib.build()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = MODEL_DICT["svox"](scale=0.5, half_opt=False, sh_degree=2, grid_size=256, grid_radius=0.0125, origin_sh=0.,
                               origin_sigma=0.1, use_trilinear=args.trilinear).to(dev)
    with torch.no_grad():
        model.sh_fields.uniform_(-0.5, 0.5)
        model.density_fields.uniform_(0.0, 30.0)
    model.density_bitfield.copy_(refined_lego_bitfield(dev))
    opt = apex.optimizers.FusedAdam(model.parameters(), lr=1e-2, eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**19)
    batches = []
    for s in range(8):
        o, d = synthetic.lego_rays(args.rays, seed=s)
        batches.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), torch.rand(args.rays, 3, device=dev)))
    ev = lambda: torch.cuda.Event(enable_timing=True)
    split = {"forward": 0.0, "backward": 0.0, "adam": 0.0}
    samples = []

    def step(i, timed):
        o, d, target = batches[i % len(batches)]
        e = [ev() for _ in range(4)]
        e[0].record()
        with torch.autocast("cuda", dtype=torch.float16):
            res = render(model, o, d, exp_step_factor=0.0)
            loss = torch.nn.functional.mse_loss(res["rgb"], target)
        e[1].record()
        opt.zero_grad()
        scaler.scale(loss).backward()
        e[2].record()
        scaler.step(opt)
        scaler.update()
        e[3].record()
        if timed:
            samples.append(res["rm_samples"])
            torch.cuda.synchronize()
            split["forward"] += e[0].elapsed_time(e[1])
            split["backward"] += e[1].elapsed_time(e[2])
            split["adam"] += e[2].elapsed_time(e[3])

    for i in range(args.warmup):
        step(i, False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i, False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for i in range(args.steps):                                   # the split, with a sync per step (not part of the rays/s figure)
        step(i, True)
    # the backward's gradient zero-fill alone: what _VoxelShade.backward allocates and clears every step
    z0, z1 = ev(), ev()
    z0.record()
    for _ in range(args.steps):
        torch.zeros_like(model.sh_fields); torch.zeros_like(model.density_fields)
    z1.record()
    torch.cuda.synchronize()
    # one step's samples for the atomic-byte replay
    from ngp_hip import ops
    o, d, _ = batches[0]
    hits = ops.ray_aabb(o, d, 0.5)
    _, xyzs, *_ = ops.march_train(o, d, hits, model.density_bitfield, torch.rand(args.rays, device=dev), 1, 0.5, 0.0, 256, 1024)
    bps, per_run = atomic_bytes_per_sample(xyzs, model)
    n = args.steps
    sh_bytes = model.sh_fields.numel() * 4
    print(json.dumps({"metric": "voxel_dropin_rays_per_sec", "rays_per_sec": args.rays * n / dt, "rays": args.rays, "steps": n,
                      "warmup": args.warmup, "ms_per_step": 1e3 * dt / n, "grid_size": 256, "sh_degree": 2, "trilinear": args.trilinear,
                      "samples_per_step": float(np.mean([int(s) for s in samples])),
                      "split_ms_per_step": {"forward": split["forward"] / n, "backward": split["backward"] / n,
                                            "zero_fill_of_backward": z0.elapsed_time(z1) / n, "adam": split["adam"] / n},
                      "bwd_atomic_bytes_per_sample": bps, "samples_per_run": per_run, "replay_samples": int(xyzs.shape[0]),
                      "field_bytes": sh_bytes + model.density_fields.numel() * 4,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
