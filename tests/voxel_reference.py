"""Torch restatement of the voxel-grid contract (VoxelGrid, model_name='svox'; DESIGN.md, voxel grid): position -> row, eval_sh of
degree 0-4, relu density and sigmoid colour.  Runs on any device and in f32 or f64; autograd gives the reference gradient."""
import numpy as np
import torch


def _basis_table(x, y, z):
    """The 25 real spherical-harmonic basis functions of degrees 0-4 in eval_sh's normalisation and sign convention, each as
    (constant, factors): Y_k = constant * factor_1 * factor_2 ... (x, y, z: the unit direction's components)."""
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return [
        (0.28209479177387814, ()),
        (-0.4886025119029199, (y,)), (0.4886025119029199, (z,)), (-0.4886025119029199, (x,)),
        (1.0925484305920792, (xy,)), (-1.0925484305920792, (yz,)), (0.31539156525252005, (2.0 * zz - xx - yy,)),
        (-1.0925484305920792, (xz,)), (0.5462742152960396, (xx - yy,)),
        (-0.5900435899266435, (y, 3 * xx - yy)), (2.890611442640554, (xy, z)), (-0.4570457994644658, (y, 4 * zz - xx - yy)),
        (0.3731763325901154, (z, 2 * zz - 3 * xx - 3 * yy)), (-0.4570457994644658, (x, 4 * zz - xx - yy)),
        (1.445305721320277, (z, xx - yy)), (-0.5900435899266435, (x, xx - 3 * yy)),
        (2.5033429417967046, (xy, xx - yy)), (-1.7701307697799304, (yz, 3 * xx - yy)), (0.9461746957575601, (xy, 7 * zz - 1)),
        (-0.6690465435572892, (yz, 7 * zz - 3)), (0.10578554691520431, (zz * (35 * zz - 30) + 3,)),
        (-0.6690465435572892, (xz, 7 * zz - 3)), (0.47308734787878004, (xx - yy, 7 * zz - 1)),
        (-1.7701307697799304, (xz, xx - 3 * yy)), (0.6258357354491761, (xx * (xx - 3 * yy) - yy * (3 * xx - yy),)),
    ]


def eval_sh(deg, sh, dirs):
    """sum_k Y_k(dirs) * sh[..., k] over the (deg+1)^2 basis functions, accumulated in index order (sh [..., C, D], dirs [..., 3]
    unit; the result is [..., C])."""
    x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
    result = None
    for k, (const, factors) in enumerate(_basis_table(x, y, z)[:(deg + 1)**2]):
        term = const
        for f in factors:
            term = term * f
        term = term * sh[..., k]
        result = term if result is None else result + term
    return result


def grid_min(G, radius):
    """grid_normalized_coords.min(0) as the reference's initialize_grid forms it: f32 index times f32 radius."""
    return np.float32(np.float32(1 - np.ceil(G / 2)) * np.float32(radius))


def normalized_index(x, G, radius):
    """(p - m) / r in f32 (normalize_samples, networks.py:521-522); x: f32 tensor [n, 3]."""
    m = torch.tensor(grid_min(G, radius), dtype=torch.float32, device=x.device)
    return (x.float() - m) / torch.tensor(np.float32(radius), device=x.device)


def rows(x, G, radius):
    """Row (ix*G + iy)*G + iz of the nearest grid point (torch.round: half to even), -1 where any axis is outside [0, G)."""
    a = torch.round(normalized_index(x, G, radius))
    valid = ((a >= 0) & (a < G)).all(1)
    ai = torch.where(valid[:, None], a, torch.zeros_like(a)).long()
    r = (ai[:, 0] * G + ai[:, 1]) * G + ai[:, 2]
    return torch.where(valid, r, torch.full_like(r, -1))


def forward(x, d, sh_fields, density_fields, G, deg, radius):
    """(sigmas [n], rgbs [n, 3]) in the fields' dtype; differentiable w.r.t. both fields."""
    D = (deg + 1)**2
    r = rows(x, G, radius)
    valid = r >= 0
    rc = torch.where(valid, r, torch.zeros_like(r))
    sh = sh_fields.reshape(G**3, 3 * D)[rc] * valid[:, None].to(sh_fields.dtype)
    dens = density_fields.reshape(G**3)[rc] * valid.to(density_fields.dtype)
    dd = d.to(sh_fields.dtype)
    dn = dd / torch.norm(dd, dim=1, keepdim=True)
    rgb = torch.sigmoid(eval_sh(deg, sh.reshape(-1, 3, D), dn))
    return torch.relu(dens), rgb
