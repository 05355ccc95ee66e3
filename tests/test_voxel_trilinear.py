"""Trilinear voxel-grid lookup, CPU tier: the torch restatement (tests/voxel_trilinear_reference.py) against grid_sample, the two
exactness properties the contract names, and the module / switch / ABI surface.  No GPU."""
import numpy as np
import pytest
import torch

import voxel_reference as vr
import voxel_trilinear_reference as vt

R = 0.0125


def _points(G, radius, n, seed, lo=-2.0, hi=None):
    """f32 positions whose index u = (p - m) / r is uniform in [lo, hi) per axis (default hi: G + 1)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(lo, G + 1 if hi is None else hi, (n, 3))
    return torch.from_numpy((np.float64(vr.grid_min(G, radius)) + u * np.float64(np.float32(radius))).astype(np.float32))


def test_restatement_is_grid_sample_with_zero_padding():
    G, deg, D = 16, 1, 4
    g = torch.Generator().manual_seed(0)
    sh = torch.rand(G, G, G, 3 * D, generator=g, dtype=torch.float64) * 3 - 1.5
    dens = torch.rand(G, G, G, 1, generator=g, dtype=torch.float64) * 2 - 0.5
    x = _points(G, R, 20000, 1)
    inside, b, f = vt.cell_fraction(x, G, R)
    u = vr.normalized_index(x, G, R)
    assert 0.2 < float((~inside).float().mean()) < 0.4                      # fully outside
    border = inside & (((b < 0) | (b >= G - 1)).any(1))
    assert 0.2 < float(border.float().mean()) < 0.4                         # on a partial border cell
    table = torch.cat([sh.reshape(G**3, -1), dens.reshape(G**3, 1)], 1)
    got = vt.interpolate(table, inside, b, f, G)
    # grid_sample: input [1, C, x, y, z], grid (..., 3) addresses (z, y, x) in [-1, 1] (align_corners: -1 and 1 are grid points)
    vol = table.reshape(G, G, G, -1).permute(3, 0, 1, 2)[None]
    grid = (2 * u.double() / (G - 1) - 1).flip(1)[None, None, None]
    ref = torch.nn.functional.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0, 0].T
    assert float((got - ref).abs().max()) <= 1e-12
    # ... and the whole forward is that row through eval_sh and the activations
    d = torch.randn(x.shape[0], 3, generator=g, dtype=torch.float64) * 3
    s, c = vt.forward(x, d, sh, dens, G, deg, R)
    dn = d / d.norm(dim=1, keepdim=True)
    assert float((s - torch.relu(ref[:, -1])).abs().max()) <= 1e-12
    assert float((c - torch.sigmoid(vr.eval_sh(deg, ref[:, :-1].reshape(-1, 3, D), dn))).abs().max()) <= 1e-12
    assert bool((s[~inside] == 0).all()) and bool((c[~inside] == 0.5).all())


def test_nan_position_is_outside():
    G = 16
    x = torch.tensor([[float("nan"), 0.0, 0.0], [0.0, 0.0, 0.0]])
    s, c = vt.forward(x, torch.ones(2, 3), torch.ones(G, G, G, 3), torch.ones(G, G, G, 1), G, 0, R)
    assert float(s[0]) == 0.0 and bool((c[0] == 0.5).all()) and float(s[1]) == 1.0


def test_constant_field_is_returned_exactly():
    """The nested a + t (b - a) form gives a constant field back bit for bit (the occupancy update of a fresh model relies on it);
    the product-of-weights form does not."""
    G = 32
    x = _points(G, R, 20000, 2, lo=0.0, hi=G - 1)
    inside, b, f = vt.cell_fraction(x, G, R)
    assert bool(inside.all()) and bool(((b >= 0) & (b < G - 1)).all())
    s, c = vt.forward(x, torch.ones(x.shape[0], 3), torch.full((G, G, G, 3), 0.3), torch.full((G, G, G, 1), 0.1), G, 0, R)
    assert s.dtype == torch.float32 and bool((s == np.float32(0.1)).all())
    products = (vt.corner_weights(f) * np.float32(0.1)).sum(1)
    assert float((products != np.float32(0.1)).float().mean()) > 0.1


@pytest.mark.parametrize("G", [16, 64])
def test_grid_points_return_their_row_exactly(G):
    """grid_radius = 2^-6: m + k r and u are exact in f32, so a sample on a grid point has f = 0 and reads that row alone."""
    r, deg, D = 2.0**-6, 2, 9
    g = torch.Generator().manual_seed(G)
    sh = torch.rand(G, G, G, 3 * D, generator=g) - 0.5
    dens = torch.rand(G, G, G, 1, generator=g) * 2 - 0.5
    k = torch.randint(0, G, (4096, 3), generator=g)
    x = (float(vr.grid_min(G, r)) + k.double() * r).float()
    inside, b, f = vt.cell_fraction(x, G, r)
    assert bool(inside.all()) and torch.equal(b, k) and bool((f == 0).all())
    d = torch.randn(4096, 3, generator=g)
    s, c = vt.forward(x, d, sh, dens, G, deg, r)
    s_n, c_n = vr.forward(x, d, sh, dens, G, deg, r)                         # the nearest lookup reads the same row
    assert torch.equal(s, torch.relu(dens[k[:, 0], k[:, 1], k[:, 2], 0])) and torch.equal(s, s_n) and torch.equal(c, c_n)


def test_module_builds_in_each_mode_with_one_state_dict(monkeypatch):
    from modules.networks import MODEL_DICT, VoxelGrid
    monkeypatch.delenv("NGP_EXPERIMENT", raising=False)
    models = {u: VoxelGrid(grid_size=16, sh_degree=1, use_trilinear=u) for u in (None, False, True)}
    assert [models[u].use_trilinear for u in (None, False, True)] == [False, False, True]
    keys = [list(m.state_dict().keys()) for m in models.values()]
    assert keys[0] == keys[1] == keys[2]
    models[True].load_state_dict(models[False].state_dict())                 # a checkpoint of one mode loads in the other
    models[False].load_state_dict(models[True].state_dict())
    assert MODEL_DICT["svox"](grid_size=16, use_trilinear=True).fused_train_ok(None) is False
    with pytest.raises(ValueError, match="grid_size"):
        VoxelGrid(grid_size=24, use_trilinear=True)


def test_experiment_key_selects_the_default_and_an_explicit_argument_wins(monkeypatch):
    from modules.networks import VoxelGrid
    from ngp_hip import experiment
    assert "svox_trilinear" in experiment.KEYS
    monkeypatch.setenv("NGP_EXPERIMENT", "svox_trilinear=1")
    assert VoxelGrid(grid_size=16).use_trilinear is True
    assert VoxelGrid(grid_size=16, use_trilinear=False).use_trilinear is False
    monkeypatch.setenv("NGP_EXPERIMENT", "svox_trilinear=0")
    assert VoxelGrid(grid_size=16).use_trilinear is False
    assert VoxelGrid(grid_size=16, use_trilinear=True).use_trilinear is True


def test_entry_points_exported_and_host_tensors_refused(hip_lib):
    from ngp_hip import ops
    for name in ("ngp_voxel_trilinear_fwd", "ngp_voxel_trilinear_density", "ngp_voxel_trilinear_bwd"):
        assert hasattr(hip_lib, name), name
    G = 16
    x, sh, dens = torch.zeros(8, 3), torch.zeros(G, G, G, 3), torch.zeros(G, G, G, 1)
    m = float(vr.grid_min(G, R))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.voxel_fwd(x, x, sh, dens, G, 0, m, R, trilinear=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.voxel_density(x, dens, G, m, R, trilinear=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.voxel_bwd(x, x, torch.zeros(8), x, torch.zeros(8), x, G, 0, m, R, sh, dens, trilinear=True)
