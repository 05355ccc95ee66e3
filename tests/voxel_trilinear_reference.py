"""Torch restatement of the trilinear voxel-grid contract (VoxelGrid(use_trilinear=True); DESIGN.md, voxel grid): base cell and
fraction of (p - m) / r in f32, the eight corners with out_of_grid's zero rows, nested lerps a + t (b - a) in z, y, x order on the raw
row, then relu / sigmoid(eval_sh).  Index and fraction are always f32; the interpolation runs in the fields' dtype, so the same
function is the f32 statement and the f64 yardstick.  Autograd gives the reference gradient."""
import torch

import voxel_reference as vr


def cell_fraction(x, G, radius):
    """(inside [n] bool, b [n, 3] int64, f [n, 3] f32): b = floor(u), f = u - b; inside is False where any u < -1, u >= G or NaN
    (b and f are then 0)."""
    u = vr.normalized_index(x, G, radius)
    inside = ((u >= -1) & (u < G)).all(1)
    u = torch.where(inside[:, None], u, torch.zeros_like(u))
    b = torch.floor(u)
    return inside, b.long(), u - b


def corner_rows(inside, b, G):
    """(rows [n, 8] int64, valid [n, 8] bool) of the eight corners b + (i, j, k) in index order 4 i + 2 j + k; row is 0 where not
    valid (out_of_grid)."""
    offs = torch.tensor([[c >> 2, (c >> 1) & 1, c & 1] for c in range(8)], device=b.device)
    q = b[:, None, :] + offs[None]
    valid = inside[:, None] & ((q >= 0) & (q < G)).all(2)
    rows = (q[..., 0] * G + q[..., 1]) * G + q[..., 2]
    return torch.where(valid, rows, torch.zeros_like(rows)), valid


def lerp(a, b, t):
    return a + t * (b - a)


def interpolate(table, inside, b, f, G):
    """table [G^3, C] -> [n, C]: nested lerps along z, then y, then x; corners outside the grid read zeros."""
    rows, valid = corner_rows(inside, b, G)
    # [n, 8, C]; index_select, whose backward is one index_add_ (advanced indexing would sort 8 n indices on every backward)
    v = table.index_select(0, rows.reshape(-1)).reshape(rows.shape[0], 8, -1) * valid[..., None].to(table.dtype)
    t = f.to(table.dtype)
    fx, fy, fz = t[:, 0:1], t[:, 1:2], t[:, 2:3]
    z = [lerp(v[:, 2 * p], v[:, 2 * p + 1], fz) for p in range(4)]
    return lerp(lerp(z[0], z[1], fy), lerp(z[2], z[3], fy), fx)


def forward(x, d, sh_fields, density_fields, G, deg, radius):
    """(sigmas [n], rgbs [n, 3]) in the fields' dtype; differentiable w.r.t. both fields."""
    D = (deg + 1)**2
    inside, b, f = cell_fraction(x, G, radius)
    table = torch.cat([sh_fields.reshape(G**3, 3 * D), density_fields.reshape(G**3, 1)], 1)
    row = interpolate(table, inside, b, f, G)
    dd = d.to(table.dtype)
    dn = dd / torch.norm(dd, dim=1, keepdim=True)
    rgb = torch.sigmoid(vr.eval_sh(deg, row[:, :3 * D].reshape(-1, 3, D), dn))
    return torch.relu(row[:, 3 * D]), rgb


def corner_weights(f):
    """[n, 8] products of the per-axis factors (1 - f or f) in the dtype of f, corner order 4 i + 2 j + k."""
    w = []
    for c in range(8):
        w.append((f[:, 0] if c & 4 else 1 - f[:, 0]) * (f[:, 1] if c & 2 else 1 - f[:, 1]) * (f[:, 2] if c & 1 else 1 - f[:, 2]))
    return torch.stack(w, 1)
