"""Camera-pose refinement on the procedural scene of examples/train_procedural.py.

The training images are rendered from the true cameras; the poses handed to training are those cameras perturbed by a seeded rotation
(default 1 degree) and translation (default 0.01) about random axes -- what a real capture's COLMAP poses look like.  The model is
trained with the drop-in loop (render + GradScaler + Adam); a PoseRefiner (ngp_hip/poses.py: dR, dT per image) sits in a second Adam
under the same scaler and receives its gradient through ngp_sample_rays_bwd <- ngp_march_train_bwd <- the hash encoder's position
gradient.  `--no_refine` is the control run on the perturbed poses.

Prints one JSON line: mean rotation / translation error of the training poses before and after, and the held-out PSNR (test views are
rendered from their true poses; the refined training poses are not gauge-aligned to them).

    python examples/refine_poses.py --steps 3000 [--no_refine]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from train_procedural import cameras, pixel_dirs, render_gt  # noqa: E402


def perturb(poses, rot_deg, trans, seed):
    """[exp(w) R | t + dt] with |w| = rot_deg degrees and |dt| = trans along seeded random axes."""
    from ngp_hip.poses import axis_angle_delta
    g = torch.Generator().manual_seed(seed)
    n = poses.shape[0]
    w = F.normalize(torch.randn(n, 3, generator=g), dim=1).to(poses) * math.radians(rot_deg)
    dt = F.normalize(torch.randn(n, 3, generator=g), dim=1).to(poses) * trans
    R = (torch.eye(3, device=poses.device) + axis_angle_delta(w)) @ poses[:, :, :3]
    return torch.cat([R, poses[:, :, 3:] + dt[:, :, None]], 2)


def pose_errors(est, true):
    """mean rotation angle of R_est R_true^T in degrees, mean |t_est - t_true|."""
    rel = est[:, :, :3] @ true[:, :, :3].transpose(1, 2)
    cos = ((rel.diagonal(dim1=1, dim2=2).sum(1) - 1) / 2).clamp(-1, 1)
    return float(torch.rad2deg(torch.acos(cos.double())).mean()), float((est[:, :, 3] - true[:, :, 3]).norm(dim=1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--wh", type=int, default=200)
    ap.add_argument("--n_train", type=int, default=100)
    ap.add_argument("--n_test", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--rot_deg", type=float, default=1.0)
    ap.add_argument("--trans", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--pose_lr", type=float, default=1e-3)
    ap.add_argument("--no_refine", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(23)
    from modules.networks import NGP
    from modules.rendering import MAX_SAMPLES, render
    from ngp_hip.poses import PoseRefiner
    from ngp_hip.rays import RayBatcher, get_rays

    focal = 1111.1 * args.wh / 800
    dirs = pixel_dirs(args.wh, focal, dev)
    poses = cameras(args.n_train + args.n_test, 1.39, 23, dev)
    imgs = torch.stack([render_gt(p[:, 3].expand_as(dirs), dirs @ p[:, :3].T) for p in poses])   # [n, wh*wh, 3]
    true_poses, test_poses = poses[:args.n_train], poses[args.n_train:]
    train_imgs, test_imgs = imgs[:args.n_train], imgs[args.n_train:]
    noisy_poses = perturb(true_poses, args.rot_deg, args.trans, args.seed)
    rot0, tr0 = pose_errors(noisy_poses, true_poses)

    model = NGP(scale=0.5, max_res=1024).to(dev)
    K = torch.tensor([[focal, 0, args.wh / 2], [0, focal, args.wh / 2], [0, 0, 1]], device=dev)
    model.mark_invisible_cells(K, noisy_poses, (args.wh, args.wh))
    opt = torch.optim.Adam(model.parameters(), 1e-2, eps=1e-15)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, args.steps, 1e-2 / 30)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**19)
    refiner = PoseRefiner(args.n_train).to(dev)
    pose_opt = torch.optim.Adam(refiner.parameters(), args.pose_lr, eps=1e-15)

    batcher = RayBatcher(train_imgs, noisy_poses, dirs, batch_size=args.batch)
    thr = 0.01 * MAX_SAMPLES / 3**0.5
    loss = torch.zeros(())
    for step in range(args.steps):
        batch = batcher.sample() if args.no_refine else batcher.sample(poses=refiner(batcher.poses))
        with torch.autocast("cuda", dtype=torch.float16):
            if step % 16 == 0:
                model.update_density_grid(thr, warmup=step < 256)
            res = render(model, batch["rays_o"], batch["rays_d"], exp_step_factor=0.0)
            loss = F.mse_loss(res["rgb"], batch["rgb"])
        opt.zero_grad()
        pose_opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        if not args.no_refine:
            scaler.step(pose_opt)                  # same scaler: unscaled once, skipped with the model's step on an overflow
        scaler.update()
        sched.step()
    torch.cuda.synchronize()

    with torch.no_grad():
        rot1, tr1 = pose_errors(refiner(noisy_poses), true_poses)
        model.eval()
        psnrs = []
        for p, gt in zip(test_poses, test_imgs):
            rays_o, rays_d = get_rays(dirs, p)
            with torch.autocast("cuda", dtype=torch.float16):
                res = render(model, rays_o, rays_d, test_time=True, exp_step_factor=0.0)
            psnrs.append(-10.0 * math.log10(F.mse_loss(res["rgb"], gt).item()))
    out = {"scene": "procedural Lego-shape (NOT Synthetic-NeRF Lego)", "refine": not args.no_refine, "steps": args.steps,
           "batch": args.batch, "train_views": args.n_train, "test_views": args.n_test, "image_wh": args.wh,
           "perturbation": {"rot_deg": args.rot_deg, "trans": args.trans, "seed": args.seed}, "pose_lr": args.pose_lr,
           "rot_err_deg_before": rot0, "rot_err_deg_after": rot1, "trans_err_before": tr0, "trans_err_after": tr1,
           "test_psnr_mean": sum(psnrs) / len(psnrs), "final_train_loss": float(loss)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
