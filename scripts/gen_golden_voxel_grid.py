"""Generate tests/golden/ref_voxel_grid.npz by executing the reference's own voxel-grid helpers: sh_utils.eval_sh (degrees 0-4) and
VoxelGrid.initialize_grid / normalize_samples / out_of_grid / query_grids(use_trilinear=False) (modules/networks.py:436-559), bound
to a stand-in `self` (the reference's VoxelGrid.__init__ builds an NGP hash encoder first and its forward cannot run).  Needs a
reference checkout (the path oracle/gen_golden.py names, or REF=...):
    python scripts/gen_golden_voxel_grid.py
The tests read only the .npz.

Recorded per grid size G in (16, 32): the grid minimum torch forms (grid_normalized_coords.min(0)), sample points (random ones, points
on and one ulp either side of rounding ties, points on and past the grid's faces, far outside), their normalised index
(normalize_samples), the selected row and the in-grid mask (query_grids on a field whose row r holds r + 1, and out_of_grid).  For
eval_sh: random coefficients [n, 3, 25] and unit directions, the result for every degree."""
import hashlib
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden  # noqa: E402
from oracle.gen_golden import OUT  # noqa: E402

REF = os.environ.get("REF", gen_golden.REF)
RADIUS = 0.0125


def load_reference():
    gen_golden.REF = REF
    gen_golden.load_reference()                      # registers the `refmodules` package over REF/modules (under the shim)
    sys.path.insert(0, os.path.join(ROOT, "taichi-nerfs_amd", "compat"))     # kornia's create_meshgrid3d
    for name in ("rendering", "sh_utils", "networks"):
        importlib.import_module("refmodules." + name)
    return sys.modules["refmodules.sh_utils"], sys.modules["refmodules.networks"]


def stand_in(net, G):
    """`self` for the VoxelGrid helpers: the attributes they read, grid_fields from the reference's initialize_grid."""
    me = types.SimpleNamespace(grid_size=G, grid_radius=RADIUS, device=torch.device("cpu"), sh_dim=9, origin_sh=0.0, origin_sigma=0.1)
    net.VoxelGrid.initialize_grid(me)
    for name in ("out_of_grid", "fix_out_of_grid", "normalize_samples", "query_grids"):
        setattr(me, name, types.MethodType(getattr(net.VoxelGrid, name), me))
    return me


def points(rng, G, m):
    r = np.float32(RADIUS)
    lo, hi = np.float32(m), np.float32(m) + np.float32(G - 1) * r
    x = rng.uniform(lo - 2 * r, hi + 2 * r, (160, 3)).astype(np.float32)
    # rounding ties: (p - m) / r == k + 0.5 in f32 where the arithmetic allows it, and one ulp either side
    k = rng.integers(-1, G + 1, (96, 3)).astype(np.float32)
    t = (np.float32(m) + (k + np.float32(0.5)) * r).astype(np.float32)
    t[32:64] = np.nextafter(t[32:64], np.float32(np.inf))
    t[64:96] = np.nextafter(t[64:96], np.float32(-np.inf))
    # faces: index exactly -0.5, 0, G - 1, G - 0.5 on one axis
    f = np.repeat(((hi + lo) / 2)[None], 12, 0).astype(np.float32).reshape(12, 1).repeat(3, 1)
    edges = np.array([np.float32(m) - np.float32(0.5) * r, np.float32(m), hi, hi + np.float32(0.5) * r], np.float32)
    for j in range(12):
        f[j, j % 3] = edges[j // 3]
    far = np.array([[5, 0, 0], [0, -5, 0], [0, 0, 5], [-1e6, 1e6, 0], [np.inf, 0, 0], [0, -np.inf, 0]], np.float32)
    return np.concatenate([x, t, f, far]).astype(np.float32)


def main():
    sh_utils, net = load_reference()
    rng = np.random.default_rng(382)
    data = {}
    for G in (16, 32):
        me = stand_in(net, G)
        m = me.grid_normalized_coords.min(0)[0]
        assert m.dtype == torch.float32
        x = points(rng, G, float(m[0]))
        idx = me.normalize_samples(torch.from_numpy(x))
        # a field whose row r holds (r + 1, 1): query_grids' output names the row it selected (0 where it zeroed the sample)
        rows = torch.arange(G**3, dtype=torch.float32).reshape(G, G, G, 1) + 1
        me.grid_fields = torch.cat([rows, torch.ones_like(rows)], dim=3)
        q = me.query_grids(idx.clone(), use_trilinear=False)
        mask = me.out_of_grid(torch.round(idx).to(torch.long))
        tag = "g%d" % G
        data.update({tag + "_min": m.numpy().copy(), tag + "_x": x, tag + "_idx": idx.numpy().copy(),
                     tag + "_row": (q[:, 0].to(torch.int64) - 1).numpy(), tag + "_mask": mask.numpy().copy(),
                     tag + "_sh_shape": np.array(me.sh_fields.shape), tag + "_sh_init": me.sh_fields.detach().numpy()[0, 0, 0].copy(),
                     tag + "_density_init": me.density_fields.detach().numpy()[0, 0, 0].copy()})
        print("G %d: min %r, %d points, %d outside" % (G, float(m[0]), len(x), int((~mask).sum())))
    n = 256
    sh = rng.normal(0, 1, (n, 3, 25)).astype(np.float32)
    d = rng.normal(0, 1, (n, 3)).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:6] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    data["sh_coeffs"], data["sh_dirs"] = sh, d
    for deg in range(5):
        D = (deg + 1)**2
        out = sh_utils.eval_sh(deg, torch.from_numpy(sh[..., :D]), torch.from_numpy(d))
        data["sh_deg%d" % deg] = out.numpy().copy()
    path = os.path.join(OUT, "ref_voxel_grid.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")
    for src in ("modules/networks.py", "modules/sh_utils.py"):
        print("sha256", src, hashlib.sha256(open(os.path.join(REF, src), "rb").read()).hexdigest())
    print("sha256 ref_voxel_grid.npz", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
