"""Time of the ray / pose gradient kernels (csrc/ray_grad.hip) and of a training step with pose refinement on the MI355X, recorded in
profiles/pose_refine.json.

    python profiles/microbench/ray_grad.py --out profiles/pose_refine.json

Workload: an NGP is trained briefly on the procedural scene (examples/render_normals.py's schedule) so that its occupancy grid is the
conditioned one; 8192 rays of 100 cameras are marched with zero noise (ray order) -- the bench's per-step sample count.
Kernels: each of ngp_march_train_bwd and ngp_sample_rays_bwd alternates with the torch composition of the same sum on the same inputs
(index_add_ over a per-sample ray index; index_add_ of the per-ray outer products), HIP events, 20 rounds after 3 warm ones, minimum and
median; algorithmic bytes per launch over the minimum against 8 TB/s.
Step: the drop-in loop of examples/train_procedural.py --path modules in three forms, alternating in one process: through the fused
whole-render node (today's default), with NGP_FUSED_RENDER=0 (the composable path the ray gradient needs), and with pose refinement
(PoseRefiner in a second Adam under the same GradScaler), plus the composable path with the batch's rays as leaves that require grad
(the ray gradient without PoseRefiner's torch algebra and its optimizer).  Composable minus fused is the price of leaving the fused
node, refinement minus composable the price of the ray gradient."""
import argparse
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
import torch.nn.functional as F  # noqa: E402

ROUNDS, WARM = 20, 3
N_RAYS, N_IMG = 8192, 100
HBM_BYTES_PER_US = 8e6                      # 8 TB/s


def _example():
    spec = importlib.util.spec_from_file_location("render_normals_example", os.path.join(ROOT, "examples", "render_normals.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def scene(train_steps, dev):
    """-> model, batcher (100 views of the procedural scene, 8192 rays a batch), the views' poses."""
    from modules.networks import NGP
    from ngp_hip.rays import RayBatcher
    from ngp_hip.synthetic import procedural_render_gt as render_gt
    ex = _example()
    torch.manual_seed(23)
    model = NGP(scale=0.5, max_res=1024).to(dev)
    wh, focal = 100, 1111.1 * 100 / 800
    poses, dirs = ex.cameras(N_IMG, 1.39, 23, dev), ex.pixel_dirs(wh, focal, dev)
    K = torch.tensor([[focal, 0, wh / 2], [0, focal, wh / 2], [0, 0, 1]], device=dev)
    model.mark_invisible_cells(K, poses, (wh, wh))
    ex.train(model, train_steps, poses, dirs)
    imgs = torch.stack([render_gt(p[:, 3].expand_as(dirs), dirs @ p[:, :3].T) for p in poses])
    return model, RayBatcher(imgs, poses, dirs, batch_size=N_RAYS), poses


def alternate(fns, rounds=ROUNDS, warm=WARM):
    """fns: name -> closure; every round runs each once between HIP events, in turn: all see the same clocks and caches."""
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


def kernel_times(model, batcher):
    from modules.rendering import MAX_SAMPLES
    from ngp_hip import ops
    dev = batcher.rays.device
    torch.manual_seed(1)
    batch = batcher.sample()
    o, d = batch["rays_o"], batch["rays_d"]
    hits = ops.ray_aabb(o, d, 0.5)
    rays_a, xyzs, _, _, ts, _ = ops.march_train(o, d, hits, model.density_bitfield, torch.zeros(N_RAYS, device=dev), model.cascades, 0.5,
                                                0.0, model.grid_size, MAX_SAMPLES)
    S = int(xyzs.shape[0])
    g = torch.Generator(dev).manual_seed(2)
    d_xyzs, d_dirs = torch.randn(S, 3, device=dev, generator=g), 0.1 * torch.randn(S, 3, device=dev, generator=g)
    ray_of = torch.repeat_interleave(rays_a[:, 0].long(), rays_a[:, 2].long())            # ray-ordered packing: sample -> ray
    assert ray_of.shape[0] == S

    def torch_march():
        d_o = torch.zeros(N_RAYS, 3, device=dev).index_add_(0, ray_of, d_xyzs)
        d_d = torch.zeros(N_RAYS, 3, device=dev).index_add_(0, ray_of, ts[:, None] * d_xyzs + d_dirs)
        return d_o, d_d

    out = {"samples": S, "rays": N_RAYS, "images": N_IMG}
    ko, kd = ops.march_train_bwd(d_xyzs, d_dirs, ts, rays_a)
    to, td = torch_march()
    out["march_train_bwd_vs_torch_max_abs_diff"] = float(max((ko - to).abs().max(), (kd - td).abs().max()))
    t = alternate({"ngp_march_train_bwd": lambda: ops.march_train_bwd(d_xyzs, d_dirs, ts, rays_a), "torch_index_add": torch_march})
    t["ngp_march_train_bwd_xyzs_only"] = alternate({"k": lambda: ops.march_train_bwd(d_xyzs, None, ts, rays_a)})["k"]
    nbytes = S * (12 + 12 + 4) + N_RAYS * (12 + 24)
    t["algorithmic_bytes"] = nbytes
    t["bytes_over_min_time_as_fraction_of_8TBps"] = nbytes / t["ngp_march_train_bwd"]["min_us"] / HBM_BYTES_PER_US
    out["march_train_bwd"] = t

    g_o, g_d = torch.randn(N_RAYS, 3, device=dev, generator=g), torch.randn(N_RAYS, 3, device=dev, generator=g)
    img, pix, dirs = batch["img_idxs"], batch["pix_idxs"], batcher.directions

    def torch_poses():
        terms = torch.cat([g_d[:, :, None] * dirs[pix][:, None, :], g_o[:, :, None]], 2)
        return torch.zeros(N_IMG, 3, 4, device=dev).index_add_(0, img, terms)

    out["sample_rays_bwd_vs_torch_max_abs_diff"] = float((ops.sample_rays_bwd(dirs, img, 0, pix, g_o, g_d, N_IMG) - torch_poses()).abs().max())
    t = alternate({"ngp_sample_rays_bwd": lambda: ops.sample_rays_bwd(dirs, img, 0, pix, g_o, g_d, N_IMG), "torch_index_add": torch_poses})
    nbytes = N_RAYS * (8 + 8 + 12 + 12 + 12) + N_IMG * 48
    t["algorithmic_bytes"] = nbytes
    t["index_bytes_read_by_all_blocks"] = N_IMG * N_RAYS * 8
    t["bytes_over_min_time_as_fraction_of_8TBps"] = nbytes / t["ngp_sample_rays_bwd"]["min_us"] / HBM_BYTES_PER_US
    out["sample_rays_bwd"] = t
    return out


def step_times(model, batcher):
    from modules.rendering import MAX_SAMPLES, render
    from ngp_hip.poses import PoseRefiner
    dev = batcher.rays.device
    opt = torch.optim.Adam(model.parameters(), 1e-3, eps=1e-15)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**10)
    refiner = PoseRefiner(N_IMG).to(dev)
    pose_opt = torch.optim.Adam(refiner.parameters(), 1e-4, eps=1e-15)

    def step(refine, fused, ray_grad=False):
        os.environ["NGP_FUSED_RENDER"] = "1" if fused else "0"
        batch = batcher.sample(poses=refiner(batcher.poses)) if refine else batcher.sample()
        if ray_grad:                                    # the rays as leaves: the ray gradient without PoseRefiner and its optimizer
            batch["rays_o"].requires_grad_(); batch["rays_d"].requires_grad_()
        with torch.autocast("cuda", dtype=torch.float16):
            res = render(model, batch["rays_o"], batch["rays_d"], exp_step_factor=0.0)
            loss = F.mse_loss(res["rgb"], batch["rgb"])
        opt.zero_grad()
        pose_opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        if refine:
            scaler.step(pose_opt)
        scaler.update()
        os.environ["NGP_FUSED_RENDER"] = "1"

    t = alternate({"fused_node": lambda: step(False, True), "composable_path": lambda: step(False, False),
                   "rays_as_leaves": lambda: step(False, True, ray_grad=True), "pose_refinement": lambda: step(True, True)})
    t["leaving_the_fused_node_us"] = t["composable_path"]["min_us"] - t["fused_node"]["min_us"]
    t["ray_gradient_us"] = t["pose_refinement"]["min_us"] - t["composable_path"]["min_us"]
    t["ray_gradient_to_the_rays_us"] = t["rays_as_leaves"]["min_us"] - t["composable_path"]["min_us"]
    t["pose_refiner_and_its_optimizer_us"] = t["pose_refinement"]["min_us"] - t["rays_as_leaves"]["min_us"]
    t["note"] = "one drop-in step (sample + render + GradScaler + Adam), HIP events around the whole step, minima compared"
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_refine.json"))
    ap.add_argument("--train_steps", type=int, default=320)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU: a CPU run says nothing about the kernels' time")
    model, batcher, _ = scene(args.train_steps, torch.device("cuda"))
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    out["what"] = ("ngp_march_train_bwd / ngp_sample_rays_bwd against the torch composition of the same sums, and one drop-in training "
                   "step in three forms; HIP events, alternating, %d rounds after %d warm ones" % (ROUNDS, WARM))
    out["scene"] = "procedural scene, NGP trained %d steps (FusedTrainer) for the occupancy grid and the table" % args.train_steps
    out["kernels"] = kernel_times(model, batcher)
    out["step"] = step_times(model, batcher)
    print(json.dumps({k: out[k] for k in ("kernels", "step")}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
