"""Train the voxel-grid radiance field (MODEL_DICT['svox']) on the procedural scene of ngp_hip.synthetic, the way train.py drives it:
mark_invisible_cells, the occupancy update every 16 steps (warm-up for the first 256), render + FusedAdam(lr 1e-2, eps 1e-15) +
GradScaler(2^19) under autocast fp16, 8192 procedural Lego rays a step.  Prints one JSON line with the PSNR on held-out rays before
and after.  `--trilinear` interpolates the eight grid points around each sample instead of reading the nearest one
(VoxelGrid(use_trilinear=True); DESIGN.md, voxel grid).  This is NOT Synthetic-NeRF Lego: the numbers say that the model trains.

    python examples/train_voxel_grid.py [--trilinear] [--grid_size 256] [--sh_degree 2] [--steps 400]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd"), os.path.join(ROOT, "taichi-nerfs_amd", "compat")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def cameras(dev, n=20, seed=5, radius=1.39):
    """K, [n, 3, 4] poses and image size of Blender-like cameras on the upper hemisphere (ngp_hip.synthetic.lego_rays' rig)."""
    from ngp_hip import synthetic
    rng = np.random.default_rng(seed)
    z = 0.05 + 0.9 * rng.random(n)
    phi = rng.random(n) * 2 * np.pi
    rxy = np.sqrt(1 - z * z)
    cams = radius * np.stack([rxy * np.cos(phi), rxy * np.sin(phi), z], -1)
    rot = synthetic._look_at(cams.copy(), np.zeros_like(cams), np.zeros(n))
    poses = np.concatenate([rot, cams[:, :, None]], 2)
    K = torch.tensor([[1111.1, 0, 400], [0, 1111.1, 400], [0, 0, 1]])
    return K.to(dev), torch.from_numpy(poses).float().to(dev), (800, 800)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trilinear", action="store_true", help="trilinear lookup instead of the nearest voxel")
    ap.add_argument("--grid_size", type=int, default=256)
    ap.add_argument("--sh_degree", type=int, default=2)
    ap.add_argument("--steps", type=int, default=400)
    args = ap.parse_args()
    from apex.optimizers import FusedAdam
    from modules.networks import MODEL_DICT
    from modules.rendering import MAX_SAMPLES, render
    from ngp_hip import synthetic
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = MODEL_DICT["svox"](scale=0.5, half_opt=False, sh_degree=args.sh_degree, grid_size=args.grid_size, grid_radius=0.0125,
                               origin_sh=0., origin_sigma=0.1, use_trilinear=args.trilinear).to(dev)
    model.mark_invisible_cells(*cameras(dev))

    def rays(seed):
        o, d = synthetic.lego_rays(8192, seed=seed)
        o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        return o, d, synthetic.procedural_render_gt(o, d)

    def psnr():
        o, d, gt = rays(777)                                            # held out: the training seeds are 0 .. steps - 1
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            rgb = render(model, o, d, test_time=True, exp_step_factor=0.0)["rgb"]
        return float(-10 * torch.log10(((rgb.float().clamp(0, 1) - gt) ** 2).mean()))

    psnr0 = psnr()
    opt = FusedAdam(model.parameters(), lr=1e-2, eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**19)
    thr = 0.01 * MAX_SAMPLES / 3**0.5
    torch.cuda.synchronize()
    t0 = time.time()
    for step in range(args.steps):
        o, d, target = rays(step)
        with torch.autocast("cuda", dtype=torch.float16):
            if step % 16 == 0:
                model.update_density_grid(thr, warmup=step < 256)
            res = render(model, o, d, exp_step_factor=0.0)
            loss = torch.nn.functional.mse_loss(res["rgb"], target)
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    torch.cuda.synchronize()
    print(json.dumps({"scene": "procedural Lego-shape (NOT Synthetic-NeRF Lego)", "model": "svox", "trilinear": args.trilinear,
                      "grid_size": args.grid_size, "sh_degree": args.sh_degree, "steps": args.steps, "psnr_before": psnr0,
                      "psnr_after": psnr(), "final_loss": float(loss), "train_seconds": time.time() - t0}))


if __name__ == "__main__":
    main()
