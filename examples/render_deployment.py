"""Render an exported deployment model: the reference's second program (deployment/InstantNGP/taichi_ngp/taichi_ngp.py) on the HIP kernels.

    python examples/render_deployment.py --model deployment.npy            # or a folder of .bin blobs
    python examples/render_deployment.py --train_steps 1000                # train -> save -> export -> reload -> render, one command

Without --model, --train_steps K first trains train.py's --deployment configuration (4-level, 4-feature dense grid, 16-wide MLPs) on
the procedural scene of examples/train_procedural.py through the drop-in modules, writes deployment.npy with save_deployment_model and
the .bin blobs with export_deployment_bins into --workdir, and renders from the blobs.  The image goes to <out>.npy ([h, w, 3] f32) and
<out>.ppm (binary PPM: no image library needed)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def cameras(n, radius, seed, device):
    """[n,3,4] camera-to-world matrices (right, down, front) on the upper hemisphere, looking at the origin (train_procedural.py)."""
    g = torch.Generator().manual_seed(seed)
    z = 0.1 + 0.8 * torch.rand(n, generator=g)
    phi = 2 * math.pi * torch.rand(n, generator=g)
    r = (1 - z * z).sqrt()
    pos = radius * torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], -1)
    fwd = F.normalize(-pos, dim=-1)
    up = torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd)
    right = F.normalize(torch.cross(fwd, up, dim=-1), dim=-1)
    down = torch.cross(fwd, right, dim=-1)
    return torch.cat([torch.stack([right, down, fwd], -1), pos[..., None]], -1).to(device)


def pixel_dirs(wh, focal, device):
    ys, xs = torch.meshgrid(torch.arange(wh, device=device), torch.arange(wh, device=device), indexing="ij")
    return torch.stack([(xs - wh / 2 + 0.5) / focal, (ys - wh / 2 + 0.5) / focal, torch.ones_like(xs, dtype=torch.float32)], -1).reshape(-1, 3)


def train_deployment_model(steps, device, wh=100, n_views=40, batch=8192, seed=23):
    """train.py --deployment on the procedural scene, drop-in path (autocast fp16, Adam 1e-2 eps 1e-15, cosine decay, GradScaler 2^19,
    occupancy update every 16 steps with a 256-step warm-up).  -> (model, poses [n,3,4], directions [wh*wh,3], losses per step)."""
    from modules.networks import NGP
    from modules.rendering import MAX_SAMPLES, render
    from ngp_hip.deploy import DEPLOYMENT_CONFIG
    from ngp_hip.rays import RayBatcher
    from ngp_hip.synthetic import procedural_render_gt as render_gt
    torch.manual_seed(seed)
    focal = 1111.1 * wh / 800
    dirs = pixel_dirs(wh, focal, device)
    poses = cameras(n_views, 1.39, seed, device)
    imgs = torch.stack([render_gt(p[:, 3].expand_as(dirs), dirs @ p[:, :3].T) for p in poses])
    model = NGP(**DEPLOYMENT_CONFIG).to(device)
    K = torch.tensor([[focal, 0, wh / 2], [0, focal, wh / 2], [0, 0, 1]], device=device)
    model.mark_invisible_cells(K, poses, (wh, wh))
    opt = torch.optim.Adam(model.parameters(), 1e-2, eps=1e-15)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, steps, 1e-2 / 30)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**19)
    batcher = RayBatcher(imgs, poses, dirs, batch_size=batch)
    thr = 0.01 * MAX_SAMPLES / 3**0.5
    losses = []
    for step in range(steps):
        cur = batcher.sample()
        with torch.autocast("cuda", dtype=torch.float16):
            if step % 16 == 0:
                model.update_density_grid(thr, warmup=step < 256)
            res = render(model, cur["rays_o"], cur["rays_d"], exp_step_factor=0.0)
            loss = F.mse_loss(res["rgb"], cur["rgb"])
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        sched.step()
        losses.append(loss.detach())
    return model, poses, dirs, torch.stack(losses).float().cpu().numpy()


def write_ppm(path, rgb):
    """rgb: [h, w, 3] floats in [0, 1] -> binary PPM."""
    img = (np.clip(rgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=None, help="deployment.npy, or a folder of .bin blobs")
    ap.add_argument("--res_w", type=int, default=300)
    ap.add_argument("--res_h", type=int, default=600)
    ap.add_argument("--pose_index", type=int, default=20)
    ap.add_argument("--out", default="deployment_render")
    ap.add_argument("--mode", default="oneshot", choices=["oneshot", "progressive", "fused"],
                    help="oneshot: march / shade / composite operators; progressive: the reference's rounds; fused: one launch per frame")
    ap.add_argument("--train_steps", type=int, default=0, help="train the deployment configuration on the procedural scene first")
    ap.add_argument("--workdir", default="results/deployment", help="where --train_steps writes deployment.npy and the blobs")
    ap.add_argument("--bin_dtype", default="float32", choices=["float32", "float16"])
    args = ap.parse_args()
    from modules.utils import save_deployment_model
    from ngp_hip.deploy import DeployedModel
    from ngp_hip.export import export_deployment_bins
    info = {}
    if args.model is None:
        if args.train_steps <= 0:
            ap.error("give --model, or --train_steps K to train one first")
        t0 = time.time()
        model, poses, _, losses = train_deployment_model(args.train_steps, torch.device("cuda"))
        torch.cuda.synchronize()
        os.makedirs(args.workdir, exist_ok=True)

        class Dataset:
            pass
        Dataset.poses = poses
        save_deployment_model(model, Dataset, args.workdir)
        bins = os.path.join(args.workdir, "bins")
        export_deployment_bins(os.path.join(args.workdir, "deployment.npy"), bins, dtype=np.dtype(args.bin_dtype).type, pose_index=args.pose_index)
        info.update(train_seconds=time.time() - t0, first_loss=float(losses[:10].mean()), last_loss=float(losses[-10:].mean()),
                    deployment_npy=os.path.join(args.workdir, "deployment.npy"), bins=bins)
        m = DeployedModel.from_bins(bins)
        pose = m.poses[0]
    else:
        m = DeployedModel.from_bins(args.model) if os.path.isdir(args.model) else DeployedModel.from_npy(args.model)
        if m.poses is None:
            ap.error("the model carries no pose")
        pose = m.poses[min(args.pose_index, len(m.poses) - 1)]
    out = m.render(pose, res=(args.res_w, args.res_h), mode=args.mode)
    torch.cuda.synchronize()
    rgb = out["rgb"].reshape(args.res_h, args.res_w, 3).cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.save(args.out + ".npy", rgb)
    write_ppm(args.out + ".ppm", rgb)
    info.update(res_w=args.res_w, res_h=args.res_h, mode=args.mode, total_samples=int(out["total_samples"]),
                mean_opacity=float(out["opacity"].mean()), out=[args.out + ".npy", args.out + ".ppm"])
    print(json.dumps(info))


if __name__ == "__main__":
    main()
