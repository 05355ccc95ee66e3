"""Render a normal map of the procedural scene from an NGP model: analytic normals -grad(sigma) / |grad(sigma)| through the hash encoder's
position gradient (NGP.density_normals), composited along every ray like a colour.

    python examples/render_normals.py --train_steps 500 --wh 200          # train briefly on the procedural scene, then render
    python examples/render_normals.py --train_steps 0 --wh 64             # a freshly initialised model (noise, but the whole path)

Every ray is marched once with the zero-noise training march, NGP.density_normals gives sigma and the unit normal at every sample (one
forward and one backward through the density branch; the backward's position gradient is ngp_hash_bwd_input_*), and the training
composite accumulates 0.5 * n + 0.5 front to back over black until T <= 1e-2.  No kernel is special to this example.  The image goes to
<out>.npy ([wh, wh, 3] f32) and, when PIL is there for the compat imageio, to <out>.png."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from train_procedural import cameras, pixel_dirs  # noqa: E402

T_THRESHOLD = 1e-2
RAY_CHUNK = 16384


def train(model, steps, poses, dirs, batch=8192):
    """The schedule of examples/train_procedural.py (device-resident trainer) for `steps` steps on views of the procedural scene."""
    from modules.rendering import MAX_SAMPLES
    from ngp_hip.rays import RayBatcher
    from ngp_hip.synthetic import procedural_render_gt as render_gt
    from ngp_hip.trainer import FusedTrainer
    imgs = torch.stack([render_gt(p[:, 3].expand_as(dirs), dirs @ p[:, :3].T) for p in poses])
    trainer = FusedTrainer(model, lr=1e-2, max_steps=max(steps, 1))
    batcher = RayBatcher(imgs, poses, dirs, batch_size=batch)
    thr = 0.01 * MAX_SAMPLES / 3**0.5
    for step in range(steps):
        cur = batcher.sample()
        if step % 16 == 0:
            trainer.update_density_grid(thr, warmup=step < 256)
        trainer.step(cur["rays_o"], cur["rays_d"], cur["rgb"])
    return trainer.last_loss() if steps else None


@torch.no_grad()
def render_normal_map(model, rays_o, rays_d, half=True):
    """rays [N,3] -> {'normal_rgb': [N,3] (0.5 n + 0.5 composited over black), 'opacity': [N], 'depth': [N], 'samples': int}."""
    from modules.rendering import MAX_SAMPLES
    from ngp_hip import ops
    n, dev = rays_o.shape[0], rays_o.device
    out = {"normal_rgb": torch.zeros(n, 3, device=dev), "opacity": torch.zeros(n, device=dev), "depth": torch.zeros(n, device=dev)}
    samples = 0
    hits_t = ops.ray_aabb(rays_o, rays_d, model.scale)
    for a in range(0, n, RAY_CHUNK):
        b = min(a + RAY_CHUNK, n)
        noise = torch.zeros(b - a, device=dev)
        rays_a, xyzs, _, deltas, ts, _ = ops.march_train(rays_o[a:b].contiguous(), rays_d[a:b].contiguous(), hits_t[a:b].contiguous(),
                                                         model.density_bitfield, noise, model.cascades, model.scale, 0.0, model.grid_size,
                                                         MAX_SAMPLES)
        if xyzs.shape[0] == 0:
            continue
        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
            sigmas, normals, _ = model.density_normals(xyzs)
        colours = (0.5 * normals.float() + 0.5).contiguous()
        _, op, dep, rgb, _ = ops.composite_train_fwd(sigmas.float().contiguous(), colours, deltas, ts, rays_a, T_THRESHOLD)
        out["normal_rgb"][a:b], out["opacity"][a:b], out["depth"][a:b] = rgb, op, dep
        samples += xyzs.shape[0]
    out["samples"] = samples
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--wh", type=int, default=200)
    ap.add_argument("--train_steps", type=int, default=500)
    ap.add_argument("--train_views", type=int, default=40)
    ap.add_argument("--train_wh", type=int, default=100)
    ap.add_argument("--encoder", default="f32", choices=["f32", "bf16", "half"])
    ap.add_argument("--fp32", action="store_true", help="shade without the fp16 autocast")
    ap.add_argument("--out", default="normals_render")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    torch.manual_seed(23)
    from modules.networks import NGP
    from modules.rendering import MAX_SAMPLES
    from ngp_hip.rays import get_rays

    model = NGP(scale=0.5, max_res=1024, half_opt=args.encoder == "half",
                table_dtype=torch.bfloat16 if args.encoder == "bf16" else None).to(dev)
    poses = cameras(args.train_views + 1, 1.39, 23, dev)
    focal_t = 1111.1 * args.train_wh / 800
    K = torch.tensor([[focal_t, 0, args.train_wh / 2], [0, focal_t, args.train_wh / 2], [0, 0, 1]], device=dev)
    model.mark_invisible_cells(K, poses[:-1], (args.train_wh, args.train_wh))
    info = {"encoder": args.encoder, "train_steps": args.train_steps, "image_wh": args.wh}
    if args.train_steps > 0:
        info["last_loss"] = train(model, args.train_steps, poses[:-1], pixel_dirs(args.train_wh, focal_t, dev))
    else:
        with torch.autocast("cuda", dtype=torch.float16):       # a fresh model still needs occupancy bits to march through
            model.update_density_grid(0.01 * MAX_SAMPLES / 3**0.5, warmup=True)
    model.eval()
    rays_o, rays_d = get_rays(pixel_dirs(args.wh, 1111.1 * args.wh / 800, dev), poses[-1])
    res = render_normal_map(model, rays_o.contiguous(), rays_d.contiguous(), half=not args.fp32)
    torch.cuda.synchronize()
    img = res["normal_rgb"].reshape(args.wh, args.wh, 3).cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.save(args.out + ".npy", img)
    written = [args.out + ".npy"]
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location("compat_imageio", os.path.join(ROOT, "taichi-nerfs_amd", "compat", "imageio.py"))
        imageio = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(imageio)
        imageio.imwrite(args.out + ".png", (np.clip(img, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8))
        written.append(args.out + ".png")
    except Exception as e:                                      # no PIL: the .npy is the result
        info["png_skipped"] = repr(e)
    info.update(samples=res["samples"], mean_opacity=float(res["opacity"].mean()), finite=bool(np.isfinite(img).all()), out=written)
    print(json.dumps(info))
    return info


if __name__ == "__main__":
    main()
