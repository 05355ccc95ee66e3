"""Marching tetrahedra on the GPU (csrc/mesh.hip through ngp_hip.mesh) against the numpy reference of the contract
(tests/mesh_reference.py, float64).  Unless a test says otherwise it asserts: the faces are the reference's exactly, V and T are equal,
and per axis |gpu - ref64| <= 4 * 2^-24 * (|lo_k| + N_k h_k) -- one rounding each of t, i + t d, the product with h and the sum with
lo, every one on a magnitude below the far corner of the box (the reference's own f32 mode measures 0.54 * 2^-24 on the unit box)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import mesh_reference as mr
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0**-24


def _extract(values, iso, sign, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0), normals=False):
    from ngp_hip import mesh
    m = mesh.marching_tetrahedra(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(DEV), iso, sign, lo, h, normals=normals)
    assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32
    assert m.vertices.shape == (m.vertices.shape[0], 3) and m.faces.shape == (m.faces.shape[0], 3)
    assert (m.normals is not None) == bool(normals)
    return m


def _check(values, iso, sign, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0), normals=False, what=""):
    ref = mr.marching_tetrahedra(values, iso, sign, lo, h, normals=normals)
    m = _extract(values, iso, sign, lo, h, normals)
    v, f = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
    assert v.shape == ref["vertices"].shape and f.shape == ref["faces"].shape, (what, v.shape, f.shape, ref["vertices"].shape, ref["faces"].shape)
    assert np.array_equal(f, ref["faces"]), what
    assert np.isfinite(v).all(), what
    if len(v):
        lo32, h32 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(h, np.float32).astype(np.float64)
        bound = 4 * EPS * (np.abs(lo32) + np.array(values.shape) * h32)
        err = np.abs(v.astype(np.float64) - ref["vertices"]).max(0)
        print("%s: V=%d T=%d, position error / bound per axis %s" % (what, len(v), len(f), (err / bound).round(3).tolist()))
        assert (err <= bound).all(), (what, err, bound)
    return m, ref


def test_all_256_masks_of_a_single_cell_both_signs(hip_lib):
    mag = np.random.default_rng(5).uniform(0.25, 4.0, (2, 2, 2)).astype(np.float32)
    for mask in range(256):
        bits = np.array([(mask >> c) & 1 for c in range(8)], dtype=bool).reshape(2, 2, 2)
        for sign in (+1, -1):
            field = np.where(bits, sign, -sign).astype(np.float32) * mag
            ref = mr.marching_tetrahedra(field, 0.0, sign)
            m = _extract(field, 0.0, sign)
            assert np.array_equal(m.faces.cpu().numpy(), ref["faces"]), (mask, sign)
            assert m.vertices.shape[0] == len(ref["vertices"])
            if len(ref["vertices"]):
                assert np.abs(m.vertices.cpu().numpy().astype(np.float64) - ref["vertices"]).max() <= 4 * EPS * 2, (mask, sign)


def test_dense_random_field_every_tetrahedron_active(hip_lib):
    f = np.random.default_rng(11).standard_normal((5, 4, 3)).astype(np.float32)
    _, ref = _check(f, 0.0, +1, what="5x4x3 random")
    assert len(ref["faces"]) > 100


@pytest.mark.parametrize("shape", [(19, 33, 7), (130, 3, 70), (2, 2, 300)])
def test_non_cubic_grids_with_thin_axes(hip_lib, shape):
    f = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    for sign in (+1, -1):
        _check(f, 0.125, sign, lo=(-1.5, 0.25, 3.0), h=(0.5, 0.125, 0.3), what="%dx%dx%d sign %+d" % (shape + (sign,)))


@pytest.fixture(scope="module")
def noisy_sphere():
    """67 x 66 x 65 = 287 430 points = 562 chunks of 512: each of the scan block's 256 threads owns a run of 3 chunk totals (one chunk
    per thread, 131 072 points, is what a single pass of the block would cover).  lo is non-zero and h anisotropic."""
    shape, lo, h = (67, 66, 65), (-0.3, 0.2, 1.0), (1.0 / 66, 1.1 / 65, 0.9 / 64)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    pts = np.asarray(lo) + idx * np.asarray(h)
    centre = np.asarray(lo) + 0.5 * (np.array(shape) - 1) * np.asarray(h) + np.array([0.01, -0.02, 0.015])
    field = np.linalg.norm(pts - centre, axis=-1) - 0.33 + 0.004 * np.random.default_rng(2).standard_normal(shape)
    return field.astype(np.float32), lo, h


def test_sphere_with_noise_past_one_scan_pass(hip_lib, noisy_sphere):
    field, lo, h = noisy_sphere
    assert field.size > 256 * 512
    m, ref = _check(field, 0.0, -1, lo, h, what="67x66x65 noisy sphere")
    assert len(ref["vertices"]) > 20000 and mr.edge_topology(ref["faces"])["closed"]


def test_two_launches_give_identical_bytes(hip_lib, noisy_sphere):
    field, lo, h = noisy_sphere
    a, b = _extract(field, 0.0, -1, lo, h, normals=True), _extract(field, 0.0, -1, lo, h, normals=True)
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
    assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))
    assert torch.equal(a.faces, b.faces)
    c = _extract(field, 0.0, -1, lo, h, normals=False)                  # and the normals change nothing else
    assert torch.equal(a.vertices.view(torch.int32), c.vertices.view(torch.int32)) and torch.equal(a.faces, c.faces)


@pytest.mark.parametrize("kind", ["outside", "inside", "equal to iso"])
def test_no_surface_gives_empty_tensors_and_no_emit_launch(hip_lib, monkeypatch, kind):
    def boom(*a):
        raise AssertionError("ngp_mesh_emit was launched for an empty surface")
    monkeypatch.setattr(hip_lib, "ngp_mesh_emit", boom)
    value = {"outside": -1.0, "inside": 2.0, "equal to iso": 0.5}[kind]
    for sign in (+1, -1):
        m = _extract(np.full((9, 6, 70), value, np.float32), 0.5, sign, normals=True)
        assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.normals.shape == (0, 3)


def test_non_finite_values(hip_lib):
    f = mr.nonfinite_field()
    m, ref = _check(f, 0.0, +1, normals=True, what="non-finite 9x8x7")
    assert mr.edge_topology(m.faces.cpu().numpy())["closed"]
    assert torch.isfinite(m.vertices).all() and torch.isfinite(m.normals).all()


def test_surface_cut_by_the_grid_boundary(hip_lib):
    pts, h = mr.unit_grid(21)
    f = mr.sphere_sdf(pts, centre=(0.1, 0.5, 0.95), r=0.3)
    m, ref = _check(f, 0.0, -1, (0, 0, 0), (h, h, h), what="cut sphere")
    got, want = mr.edge_topology(m.faces.cpu().numpy())["boundary"], mr.edge_topology(ref["faces"])["boundary"]
    assert len(want) > 20 and got == want


def test_grid_normals_of_the_sphere(hip_lib, noisy_sphere):
    """|n_gpu - n_ref|_inf <= 16 * 2^-24 * max|v| / (min h * |g_ref|) + 4 * 2^-24: the absolute rounding of a difference quotient of
    values up to max|v| over 2 h, through the interpolation, divided by the norm it is normalised with; plus the normalisation's own
    roundings.  Asserted where |g_ref| >= 1e-3 max|v| / min h; at most 1 % of the vertices may fall below that."""
    _, lo, h = noisy_sphere
    shape = (67, 66, 65)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    centre = np.asarray(lo) + 0.5 * (np.array(shape) - 1) * np.asarray(h)
    field = (np.linalg.norm(np.asarray(lo) + idx * np.asarray(h) - centre, axis=-1) - 0.33).astype(np.float32)
    m, ref = _check(field, 0.0, -1, lo, h, normals=True, what="67x66x65 sphere, normals")
    n, g = m.normals.cpu().numpy().astype(np.float64), ref["grad"]
    gn = np.linalg.norm(g, axis=1)
    vmax, hmin = float(np.abs(field).max()), float(min(h))
    keep = gn >= 1e-3 * vmax / hmin
    assert (~keep).sum() <= 0.01 * len(gn)
    err = np.abs(n - ref["normals"]).max(1)
    bound = 16 * EPS * vmax / (hmin * gn) + 4 * EPS
    print("normals: %d vertices, %d skipped, worst error / bound %.3f, |g| in [%.3f, %.3f]"
          % (len(gn), int((~keep).sum()), float((err[keep] / bound[keep]).max()), gn.min(), gn.max()))
    assert (err[keep] <= bound[keep]).all()
    rad = m.vertices.cpu().numpy() - centre
    assert ((n * rad).sum(1) / np.linalg.norm(rad, axis=1)).min() > 0.99          # outwards: the SDF grows away from the centre


def test_zero_gradient_gives_a_zero_normal(hip_lib):
    """v = (-1)^i: every central difference of an interior point vanishes, so the interpolated gradient is exactly zero there."""
    f = np.broadcast_to(np.where(np.arange(8) % 2 == 0, 1.0, -1.0)[:, None, None], (8, 5, 4)).astype(np.float32)
    m, ref = _check(f, 0.0, +1, normals=True, what="alternating planes")
    zero = (ref["grad"] == 0).all(1)
    n = m.normals.cpu().numpy()
    assert zero.sum() > 50 and (~zero).sum() > 50
    assert (n[zero] == 0).all()
    gn = np.linalg.norm(ref["grad"][~zero], axis=1)                       # the same bound as for the sphere: max|v| = 1, h = 1
    assert (np.abs(n[~zero] - ref["normals"][~zero]).max(1) <= 16 * EPS / gn + 4 * EPS).all()


# ---- model level -------------------------------------------------------------------------------------------------------------------
def _tiny_model(kind):
    from modules.networks import NGP, VoxelGrid
    torch.manual_seed(31)
    if kind == "svox":
        model = VoxelGrid(scale=0.5, grid_size=16).to(DEV)
        with torch.no_grad():
            model.density_fields.uniform_(0.0, 1.0)
        return model, ((-0.08, -0.08, -0.08), (0.09, 0.09, 0.09))              # inside the 16^3 grid (radius 0.0125 around the origin)
    model = NGP(scale=0.5, pos_encoder_type=kind, levels=4, log2_T=12, max_res=64).to(DEV)
    with torch.no_grad():
        for p in model.pos_encoder.parameters():
            p.uniform_(-0.5, 0.5)
    return model, None


@pytest.mark.parametrize("kind", ["hash", "triplane", "svox"])
def test_extract_mesh_from_a_model(hip_lib, kind):
    from ngp_hip import mesh
    model, bounds = _tiny_model(kind)
    b = bounds or (model.xyz_min.reshape(3).tolist(), model.xyz_max.reshape(3).tolist())
    lo, h = mesh.grid_spacing(b[0], b[1], 24)
    with torch.no_grad():
        whole = model.density(mesh.grid_points(lo, h, (25, 25, 25), 0, 25**3, DEV)).float().view(25, 25, 25)
    thr = float(whole.median())
    msh, grid = mesh.extract_mesh(model, resolution=24, threshold=thr, bounds=bounds, return_grid=True, chunk=1000)   # 1000 does not divide 25^3
    assert grid.shape == (25, 25, 25) and torch.equal(grid.view(torch.int32), whole.view(torch.int32))
    ref = mr.marching_tetrahedra(grid.cpu().numpy(), thr, +1, lo, h, normals=True)
    assert len(ref["faces"]) > 0
    assert np.array_equal(msh.faces.cpu().numpy(), ref["faces"]) and msh.vertices.shape[0] == len(ref["vertices"])
    bound = 4 * EPS * (np.abs(np.asarray(lo, np.float32).astype(np.float64)) + 25 * np.asarray(h, np.float32).astype(np.float64))
    assert (np.abs(msh.vertices.cpu().numpy().astype(np.float64) - ref["vertices"]).max(0) <= bound).all()
    assert msh.normals.shape == msh.vertices.shape
    assert mesh.extract_mesh(model, 24, thr, bounds=bounds, normals=None, chunk=4096).normals is None
    if kind == "hash":
        a = mesh.extract_mesh(model, 24, thr, normals="analytic")
        assert torch.equal(a.vertices.view(torch.int32), msh.vertices.view(torch.int32)) and torch.equal(a.faces, msh.faces)
        want = model.density_normals(msh.vertices)[1]
        assert torch.equal(a.normals.view(torch.int32), want.view(torch.int32))
    else:
        with pytest.raises(NotImplementedError):
            mesh.extract_mesh(model, 24, thr, bounds=bounds, normals="analytic")


def test_plain_callable_needs_bounds_and_takes_a_sign(hip_lib):
    from ngp_hip import mesh
    sdf = lambda x: torch.linalg.norm(x - 0.5, dim=1) - 0.3
    with pytest.raises(ValueError, match="bounds"):
        mesh.extract_mesh(sdf, 16, 0.0, sign=-1)
    m, grid = mesh.extract_mesh(sdf, 16, 0.0, bounds=((0, 0, 0), (1, 1, 1)), sign=-1, return_grid=True, chunk=777)
    ref = mr.marching_tetrahedra(grid.cpu().numpy(), 0.0, -1, (0, 0, 0), (1 / 16,) * 3)
    assert np.array_equal(m.faces.cpu().numpy(), ref["faces"]) and mr.euler(m.vertices.shape[0], ref["faces"]) == 2
    assert mesh.topology(m) == {"vertices": len(ref["vertices"]), "faces": len(ref["faces"]), "euler": 2, "boundary_edges": 0}


def test_example_extracts_the_fitted_sphere(hip_lib, tmp_path, capsys):
    """examples/extract_mesh.py --sdf with a small fit.  The SDF is 1-Lipschitz and the ends of a cut edge straddle zero to within
    err = max |f - sdf| over the grid points, so every vertex lies within err + sqrt(3) h (the longest lattice edge) of the sphere."""
    spec = importlib.util.spec_from_file_location("extract_mesh_example", os.path.join(ROOT, "examples", "extract_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = str(tmp_path / "sphere.ply")
    info = ex.main(["--sdf", "--steps", "300", "--n", "4096", "--log2_T", "14", "--levels", "8", "--max_res", "128", "--resolution", "48",
                    "--out", out])
    grid, msh = info["grid"], info["mesh"]
    h = 1.0 / 48
    a = torch.linspace(0, 1, 49, dtype=torch.float64)
    pts = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1)
    sdf = torch.linalg.norm(pts - 0.5, dim=-1) - 0.3
    err = float((grid.cpu().double() - sdf).abs().max())
    dist = (torch.linalg.norm(msh.vertices.cpu().double() - 0.5, dim=1) - 0.3).abs()
    print("fit error %.4f, worst vertex distance %.4f, bound %.4f, chi %d, boundary edges %d"
          % (err, float(dist.max()), err + math.sqrt(3) * h, info["euler"], info["boundary_edges"]))
    assert msh.vertices.shape[0] > 0 and float(dist.max()) <= err + math.sqrt(3) * h
    assert err < 0.2                   # then f > 0 on the whole boundary of [0,1]^3 (sdf >= 0.2 there): the surface cannot reach it
    assert info["boundary_edges"] == 0 and info["euler"] == 2             # one closed sphere, what the example's JSON line reports
    assert os.path.getsize(out) > 0 and '"euler"' in capsys.readouterr().out
