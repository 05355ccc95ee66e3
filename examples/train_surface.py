"""Train a signed-distance field FROM IMAGES through the NeuS-opacity compositor (ngp_hip.surface, csrc/surface.hip) and mesh it.

    python examples/train_surface.py
    python examples/train_surface.py --steps 60 --views 4 --wh 32 --batch 1024 --log2_T 14 --levels 8 --max_res 256 --mesh_res 32    # tiny

The scene is analytic with a KNOWN signed distance (ngp_hip.synthetic.surface_sdf: a sphere united with a box inside [-0.5, 0.5]^3),
rendered by sphere tracing with Lambert shading; no dataset is needed.  Training composites over a random grey background per step
(render and target alike), evaluation over white.  An SDFField is trained with
    loss = MSE(rgb) + eikonal_weight * mean (|grad f| - 1)^2          (the eikonal term on the marched samples)
under a cosine anneal that goes 0 -> 1 over the first --anneal_steps steps and occupancy updates every 16 steps (all cells during the
warm-up, like NGP).  Then held-out views are rendered, the level set f = 0 is extracted with marching tetrahedra, and one JSON line
reports: held-out PSNR, inv_s first / last, the mean eikonal error, the mesh's vertex / face counts, Euler characteristic and boundary
edges, and the mean |true SDF| at the mesh vertices -- for the trained model and for the untrained one (the initial sphere).
loss_first / loss_last are means over the first / last five steps.

--trace: the held-out views are also rendered by sphere tracing (ngp_hip.surface.render_surface_traced, csrc/sdf_trace.hip) and the line
gains, for both renderers, the held-out PSNR and the milliseconds per frame, and the tracer's mean / max evaluations per ray."""
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

import torch  # noqa: E402


def _mesh_report(model, res, dev):
    from ngp_hip import synthetic
    from ngp_hip.mesh import extract_mesh, topology
    mesh = extract_mesh(model.sdf, res, 0.0, bounds=([-0.5] * 3, [0.5] * 3), sign=-1, device=dev)
    topo = topology(mesh)
    err = float(synthetic.surface_sdf(mesh.vertices).abs().mean()) if topo["vertices"] else float("nan")
    return topo, err


def _frame_ms(render, frames, rounds=3):
    """milliseconds per frame of render(i) over `frames` frames, the best of `rounds` passes after a warm one"""
    best = float("inf")
    for r in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(frames):
            render(i)
        torch.cuda.synchronize()
        if r:
            best = min(best, 1e3 * (time.perf_counter() - t0) / frames)
    return best


def main(argv=None, return_model=False):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--test_views", type=int, default=4)
    ap.add_argument("--wh", type=int, default=96, help="image side in pixels")
    ap.add_argument("--batch", type=int, default=4096, help="rays per step")
    ap.add_argument("--log2_T", type=int, default=19)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--max_res", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--eikonal_weight", type=float, default=0.1)
    ap.add_argument("--anneal_steps", type=int, default=None, help="default: a quarter of --steps")
    ap.add_argument("--warmup_steps", type=int, default=256)
    ap.add_argument("--mesh_res", type=int, default=128)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--n_importance", type=int, default=0,
                    help="inverse-CDF draws per ray that refine the marched samples (hierarchical sampling); 0: the march alone")
    ap.add_argument("--trace", action="store_true",
                    help="also render the held-out views by sphere tracing; report PSNR and ms per frame of both renderers")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this example needs the GPU: libngp_hip has no CPU path")
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    from ngp_hip import synthetic
    from ngp_hip.surface import MAX_SAMPLES, SDFField, render_surface

    model = SDFField(scale=0.5, levels=args.levels, log2_T=args.log2_T, max_res=args.max_res).to(dev)
    topo0, sdf_err0 = _mesh_report(model, args.mesh_res, dev)

    t = lambda a: torch.from_numpy(a).to(dev)
    o_tr, d_tr = (t(a) for a in synthetic.orbit_camera_rays(args.views, (args.wh, args.wh), seed=args.seed))
    o_te, d_te = (t(a) for a in synthetic.orbit_camera_rays(args.test_views, (args.wh, args.wh), seed=args.seed + 1000))
    rgb_tr, hit_tr = synthetic.surface_render_gt(o_tr, d_tr)[:2]
    rgb_te = synthetic.surface_render_gt(o_te, d_te)[0]

    opt = torch.optim.Adam(model.parameters(), lr=args.lr, eps=1e-15)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, args.steps, args.lr / 30)
    anneal_steps = max(1, args.steps // 4 if args.anneal_steps is None else args.anneal_steps)
    threshold = 0.01 * MAX_SAMPLES / math.sqrt(3.0)
    gen = torch.Generator(dev).manual_seed(args.seed)
    inv_s_first = float(model.inv_s().detach())
    losses, eik_err, t0 = [], float("nan"), None
    for step in range(args.steps):
        if step == min(10, args.steps - 1):
            torch.cuda.synchronize()
            t0, step0 = time.perf_counter(), step
        if step % 16 == 0:
            model.update_density_grid(threshold, warmup=step < args.warmup_steps)
        idx = torch.randint(o_tr.shape[0], (args.batch,), device=dev, generator=gen)
        # a random grey background per step, in the render and in the target alike: over a fixed white one a white sheet in empty
        # space costs nothing, and the opacity of the field is only as right as the colours let it be
        bg = float(torch.rand((), device=dev, generator=gen))
        res = render_surface(model, o_tr[idx], d_tr[idx], cos_anneal=min(1.0, step / anneal_steps), bg=bg,
                             n_importance=args.n_importance)
        target = torch.where(hit_tr[idx][:, None], rgb_tr[idx], torch.full_like(rgb_tr[idx], bg))
        mse = torch.nn.functional.mse_loss(res["rgb"], target)
        gn = res["grad_norm"]
        eik = ((gn - 1.0) ** 2).mean() if gn.numel() else mse.new_zeros(())
        loss = mse + args.eikonal_weight * eik
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        sched.step()
        losses.append(loss.detach())
        if gn.numel():
            eik_err = (gn.detach() - 1.0).abs().mean()
    torch.cuda.synchronize()
    step_ms = 1e3 * (time.perf_counter() - t0) / max(1, args.steps - step0)
    losses = [float(x) for x in losses]
    k = min(5, len(losses))

    with torch.no_grad():
        out = render_surface(model, o_te, d_te, test_time=True, n_importance=args.n_importance)
        mse_te = float(torch.nn.functional.mse_loss(out["rgb"], rgb_te))
    topo, sdf_err = _mesh_report(model, args.mesh_res, dev)
    info = {"steps": args.steps, "views": args.views, "image": args.wh, "rays_per_step": args.batch, "levels": args.levels, "log2_T": args.log2_T,
            "max_res": args.max_res, "eikonal_weight": args.eikonal_weight, "n_importance": args.n_importance,
            "loss_first": sum(losses[:k]) / k, "loss_last": sum(losses[-k:]) / k,
            "psnr_heldout": -10.0 * math.log10(max(mse_te, 1e-12)), "inv_s_first": inv_s_first, "inv_s_last": float(model.inv_s().detach()),
            "eikonal_error": float(eik_err), "step_ms": step_ms,
            "mesh_resolution": args.mesh_res, "mesh_vertices": topo["vertices"], "mesh_faces": topo["faces"], "mesh_euler": topo["euler"],
            "mesh_boundary_edges": topo["boundary_edges"], "mesh_sdf_error": sdf_err,
            "untrained_mesh_vertices": topo0["vertices"], "untrained_mesh_sdf_error": sdf_err0}
    if args.trace:
        from ngp_hip.surface import render_surface_traced
        px = args.wh * args.wh
        view = lambda a, i: a[i * px:(i + 1) * px]
        with torch.no_grad():
            tr = render_surface_traced(model, o_te, d_te)
            mse_tr = float(torch.nn.functional.mse_loss(tr["rgb"], rgb_te))
            ms_march = _frame_ms(lambda i: render_surface(model, view(o_te, i), view(d_te, i), test_time=True, n_importance=args.n_importance),
                                 args.test_views)
            ms_trace = _frame_ms(lambda i: render_surface_traced(model, view(o_te, i), view(d_te, i)), args.test_views)
        info.update({"psnr_heldout_traced": -10.0 * math.log10(max(mse_tr, 1e-12)), "frame_ms_marched": ms_march, "frame_ms_traced": ms_trace,
                     "trace_n_eval_mean": float(tr["n_eval"].float().mean()), "trace_n_eval_max": int(tr["n_eval"].max()),
                     "trace_status_counts": [int((tr["status"] == k).sum()) for k in range(4)]})
    print(json.dumps(info))
    return (info, model) if return_model else info


if __name__ == "__main__":
    main()
