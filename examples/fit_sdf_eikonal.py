"""Fit a signed distance function with an eikonal regulariser: a loss on the GRADIENT of the network with respect to its input trains
the hash table through the encoder's double backward (HashEncoder(twice_differentiable=True), ngp_hash_bwd2_*).

    python examples/fit_sdf_eikonal.py --steps 500
    python examples/fit_sdf_eikonal.py --steps 50 --n 2048 --log2_T 14 --levels 8 --max_res 256 --sdf_weight 0      # eikonal term only

f(x) = MLP(HashEncoder(x)) is fitted to the analytic SDF of a sphere (centre 0.5, radius 0.3) in [0, 1]^3 with
    loss = sdf_weight * mean |f - sdf| + eikonal_weight * mean (|grad_x f| - 1)^2,
optimised with Adam on fresh uniform points every step.  grad_x f comes from torch.autograd.grad(..., create_graph=True): the backward of
the loss differentiates it once more, with respect to the table, the MLP weights and (unused here) the positions.  The first and last
values of the SDF loss and of mean | |grad f| - 1 | are reported as one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "taichi-nerfs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def sphere_sdf(x, radius=0.3):
    return torch.linalg.norm(x - 0.5, dim=1) - radius


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--n", type=int, default=16384, help="points per step")
    ap.add_argument("--log2_T", type=int, default=19)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--max_res", type=float, default=2048.0)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--sdf_weight", type=float, default=1.0)
    ap.add_argument("--eikonal_weight", type=float, default=0.1)
    ap.add_argument("--bf16_table", action="store_true", help="gather from the bf16 storage copy of the table")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this example needs the GPU: libngp_hip has no CPU path")
    dev = torch.device("cuda")
    torch.manual_seed(args.seed)
    from modules.hash_encoder import HashEncoder

    enc = HashEncoder(max_params=2**args.log2_T, levels=args.levels, max_res=args.max_res, twice_differentiable=True,
                      table_dtype=torch.bfloat16 if args.bf16_table else None).to(dev)
    with torch.no_grad():                                          # small features around 0: the fit starts from a smooth function
        enc.hash_table.uniform_(-1e-4, 1e-4)
    mlp = torch.nn.Sequential(torch.nn.Linear(enc.out_dim, args.width), torch.nn.Softplus(beta=100.0),
                              torch.nn.Linear(args.width, 1)).to(dev)
    opt = torch.optim.Adam(list(enc.parameters()) + list(mlp.parameters()), lr=args.lr, eps=1e-15)
    gen = torch.Generator(dev).manual_seed(args.seed)
    hist = []
    for step in range(args.steps):
        x = torch.rand(args.n, 3, device=dev, generator=gen).requires_grad_()
        f = mlp(enc(x)).squeeze(1)
        (grad,) = torch.autograd.grad(f.sum(), x, create_graph=True)
        norm = torch.linalg.norm(grad, dim=1)
        sdf_loss = (f - sphere_sdf(x.detach())).abs().mean()
        eikonal = ((norm - 1.0) ** 2).mean()
        loss = args.sdf_weight * sdf_loss + args.eikonal_weight * eikonal
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if step in (0, args.steps - 1):
            hist.append((float(sdf_loss.detach()), float((norm.detach() - 1.0).abs().mean()), float(loss.detach())))
    torch.cuda.synchronize()
    info = {"steps": args.steps, "points_per_step": args.n, "levels": args.levels, "log2_T": args.log2_T, "max_res": args.max_res,
            "table": "bf16 copy" if args.bf16_table else "f32", "sdf_weight": args.sdf_weight, "eikonal_weight": args.eikonal_weight,
            "sdf_loss_first": hist[0][0], "sdf_loss_last": hist[-1][0],
            "eikonal_error_first": hist[0][1], "eikonal_error_last": hist[-1][1],
            "loss_first": hist[0][2], "loss_last": hist[-1][2],
            "table_grad_nonzero": bool(enc.hash_table.grad is not None and enc.hash_table.grad.abs().sum() > 0)}
    print(json.dumps(info))
    return info


if __name__ == "__main__":
    main()
