"""Mesh simplification on the GPU (csrc/mesh_simplify.hip through ngp_hip.simplify_mesh) against the serial reference of the contract
(tests/mesh_simplify_reference.py).

THE STANDARD ASSERTION (_check): vertex_map, face_map, the output faces, n_clusters, the bad counts and the grid equal the reference;
positions are within the reference's `bound` per coordinate and normals within `normal_bound` (both derived in the reference's module
docstring: one float32 rounding plus the float64 sums pushed through a system of condition at most (1 + eps) / eps)."""
import numpy as np
import pytest
import torch

import mesh_components_reference as C
import mesh_sdf_reference as M
import mesh_simplify_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
INF = float("inf")


def _mesh(v, f):
    from ngp_hip import mesh
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return mesh.Mesh(t(np.asarray(v, np.float32).reshape(-1, 3)), t(np.asarray(f, np.int32).reshape(-1, 3)), None)


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t.contiguous().view(torch.int32))


def _compare(got, ref, what=""):
    assert (got.n_clusters, got.bad_faces, got.bad_vertices) == (ref["n_clusters"], ref["bad_faces"], ref["bad_vertices"])
    assert got.vertex_map.dtype == torch.int32 and got.face_map.dtype == torch.int32 and got.mesh.faces.dtype == torch.int32
    assert np.array_equal(_np(got.vertex_map), ref["vertex_map"]) and np.array_equal(_np(got.face_map), ref["face_map"])
    assert got.mesh.faces.shape == (ref["n_faces"], 3) and np.array_equal(_np(got.mesh.faces), ref["faces"])
    assert got.mesh.vertices.shape == (ref["n_vertices"], 3) and got.mesh.vertices.dtype == torch.float32
    err = np.abs(_np(got.mesh.vertices).astype(np.float64) - ref["vertices"].astype(np.float64))
    worst = float((err / ref["bound"]).max()) if err.size else 0.0
    worst_n = 0.0
    if got.mesh.normals is not None:
        assert got.mesh.normals.shape == got.mesh.vertices.shape
        nerr = np.linalg.norm(_np(got.mesh.normals).astype(np.float64) - ref["normals"].astype(np.float64), axis=1)
        worst_n = float((nerr / ref["normal_bound"]).max()) if nerr.size else 0.0
    print("%s: C %d V' %d T' %d; worst |device - reference| / bound: position %.3g, normal %.3g"
          % (what, got.n_clusters, ref["n_vertices"], ref["n_faces"], worst, worst_n))
    assert worst <= 1.0 and worst_n <= 1.0


def _check(v, f, bounds, what="", regularization=1e-3, normals=True, **grid_kw):
    import ngp_hip
    from ngp_hip import mesh
    lo, h, n = mesh.simplify_grid(bounds, **grid_kw)
    got = ngp_hip.simplify_mesh(_mesh(v, f), bounds=bounds, regularization=regularization, normals=normals, **grid_kw)
    assert got.grid == n and got.lo == tuple(lo.tolist()) and got.h == tuple(h.tolist())
    assert (got.mesh.normals is None) == (not normals)
    ref = R.simplify(v, f, lo, h, n, regularization=regularization)
    _compare(got, ref, what)
    return got, ref


# ---- sizes around every boundary of the implementation: the 64-lane wave, the 512-slot scan chunk, many chunks ------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 20000])
def test_disjoint_triangles(n):
    v, f = C.disjoint_triangles(n, seed=n)
    got, ref = _check(v, f, UNIT, "disjoint %d, fine cells" % n, cell=2.0**-12)
    assert ref["n_faces"] == n and ref["n_vertices"] == 3 * n          # a face's corners are ~0.08 apart, a cell 0.0002: all survive
    got, ref = _check(v, f, UNIT, "disjoint %d, one cell" % n, resolution=1)
    assert got.mesh.faces.shape == (0, 3) and got.mesh.vertices.shape == (0, 3) and got.n_clusters == min(n, 1)
    assert (got.face_map == -1).all() and (got.vertex_map == -1).all()


def test_no_vertices_and_no_faces():
    import ngp_hip
    empty_v, empty_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    got = ngp_hip.simplify_mesh(_mesh(empty_v, empty_f), cell=0.1)
    assert got.mesh.vertices.shape == (0, 3) and got.mesh.faces.shape == (0, 3) and got.vertex_map.shape == (0,) and got.face_map.shape == (0,)
    assert (got.n_clusters, got.bad_faces, got.bad_vertices) == (0, 0, 0)
    got, _ = _check(M.cube()[0], empty_f, UNIT, "V 8, T 0", cell=0.1)                      # V > 0, T = 0
    assert got.n_clusters == 8 and _np(got.vertex_map).tolist() == [-1] * 8 and got.mesh.vertices.shape == (0, 3)
    got = ngp_hip.simplify_mesh(_mesh(empty_v, M.cube()[1]), resolution=4)                   # V = 0, T > 0: every face is bad
    assert got.bad_faces == 12 and _np(got.face_map).tolist() == [-1] * 12 and got.mesh.faces.shape == (0, 3)
    got = ngp_hip.simplify_mesh(_mesh(empty_v, M.cube()[1]), target_faces=5)
    assert got.bad_faces == 12 and got.grid == (1, 1, 1)


# ---- one cluster with every incidence; many clusters with a few ---------------------------------------------------------------------------------
def test_fan_hub_owns_every_incidence():
    v, f = R.hub_fan(10**4)
    got, ref = _check(v, f, R.box_of(v), "fan", cell=0.05)
    hub = int(ref["vertex_cluster"][0])
    assert (ref["face_cluster"] == hub).any(1).all() and ref["n_clusters"] > 100              # the rim: many cells
    assert 0 < ref["n_faces"] < 10**4 and ref["vertex_map"][0] >= 0


def test_strip_across_thousands_of_cells():
    v, f = C.strip(2**16 + 3, "random", seed=5)
    got, ref = _check(v, f, R.box_of(v), "strip", cell=(8.0, 0.5, 1.0))
    assert ref["n_clusters"] > 8000 and 1000 < ref["n_faces"] < len(f) // 4                   # a face survives where the strip crosses a cell


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [0.06, 0.17])
@pytest.mark.parametrize("name", sorted(R.NAMED))
def test_named_shapes(name, cell):
    v, f = R.NAMED[name]()
    got, ref = _check(v, f, R.box_of(v), "%s, cell %.2f" % (name, cell), cell=cell)
    assert ref["n_faces"] <= len(f) and ref["n_vertices"] <= len(v)
    vm = ref["vertex_map"]
    moved = np.abs(_np(got.mesh.vertices)[vm[vm >= 0]].astype(np.float64) - v[vm >= 0])
    assert (moved <= np.float32(cell) + 2.0**-20).all()               # no vertex leaves its cell (found by a few float32 roundings of values below 1)


@pytest.mark.parametrize("h", [0.07, 0.11])
def test_the_quadric_point_keeps_the_cube(h):
    import ngp_hip
    v, f = R.tessellated_cube()
    got, ref = _check(v, f, UNIT, "tessellated cube, h %.2f" % h, cell=h)
    mean = ngp_hip.simplify_mesh(_mesh(v, f), cell=h, bounds=UNIT, regularization=INF)
    cq, cm = R.corner_distance(_np(got.mesh.vertices)), R.corner_distance(_np(mean.mesh.vertices))
    vq, vm = R.volume(_np(got.mesh.vertices), _np(got.mesh.faces)), R.volume(_np(mean.mesh.vertices), _np(mean.mesh.faces))
    print("h %.2f: corner %.5f against %.5f (mean); volume %.6f against %.6f" % (h, cq, cm, vq, vm))
    assert cq < 0.1 * cm and abs(vq - 0.125) < 0.1 * abs(vm - 0.125) and vq > 0
    assert torch.equal(got.mesh.faces, mean.mesh.faces)


@pytest.mark.parametrize("cells", [2, 4])
def test_extracted_sphere(cells):
    import ngp_hip
    from ngp_hip import mesh
    a = np.linspace(0.0, 1.0, 33)
    field = (np.linalg.norm(np.stack(np.meshgrid(a, a, a, indexing="ij"), -1) - 0.5, axis=-1) - 0.3).astype(np.float32)
    m = mesh.marching_tetrahedra(torch.from_numpy(field).to(DEV), 0.0, sign=-1, lo=(0.0, 0.0, 0.0), h=(1 / 32,) * 3)
    v, f = _np(m.vertices), _np(m.faces)
    got, ref = _check(v, f, UNIT, "sphere at 33^3, %d grid cells" % cells, cell=cells / 32)
    assert 0 < got.mesh.faces.shape[0] < len(f) // 2
    cc = ngp_hip.components(got.mesh)
    assert cc.n >= 1 and cc.bad_faces == 0 and cc.unused_vertices == 0
    radius = np.linalg.norm(_np(got.mesh.vertices) - 0.5, axis=1)
    assert np.abs(radius - 0.3).max() < cells / 32


# ---- the edges of the grid ----------------------------------------------------------------------------------------------------------------------
def test_cell_faces_clamping_and_huge_coordinates():
    """Vertices exactly on cell faces (multiples of the dyadic cell 1/8), outside the bounds (clamped into the boundary cells) and at
    +-3e38: data the contract defines."""
    v0, f0 = M.icosphere(1)
    a = np.arange(0, 9) / 8.0
    on_faces = np.stack(np.meshgrid(a, a, [0.0, 0.5, 1.0], indexing="ij"), -1).reshape(-1, 3)
    outside = np.array([[-1.0, 0.5, 0.5], [2.0, 0.5, 0.5], [0.5, -7.0, 3.0], [1.0 + 2.0**-20, 1.0, 1.0], [-2.0**-30, 0.0, 0.0]])
    huge = np.array([[3e38, 0.1, 0.1], [-3e38, 0.9, 0.2], [0.3, 3e38, -3e38], [3e38, 3e38, 3e38], [-3e38, -3e38, -3e38]])
    v = np.concatenate([v0, on_faces, outside, huge]).astype(np.float32)
    base = len(v0)
    rng = np.random.default_rng(21)
    extra = rng.integers(base, len(v), (400, 3))
    mixed = np.stack([rng.integers(0, base, 60), rng.integers(base, len(v), 60), rng.integers(len(v) - 10, len(v), 60)], 1)
    f = np.concatenate([f0, extra, mixed]).astype(np.int32)
    got, ref = _check(v, f, UNIT, "faces of cells, clamped, huge", cell=0.125)
    assert ref["bad_vertices"] == 0 and ref["bad_faces"] == 0 and ref["n_faces"] > 100
    key, q = R.keys(v, np.zeros(3, np.float32), np.full(3, 0.125, np.float32), (8, 8, 8))
    assert q.min() == 0 and q.max() == 7 and q[base + len(on_faces)].tolist() == [0, 4, 4] and q[-1].tolist() == [0, 0, 0] and q[-2].tolist() == [7, 7, 7]
    assert np.isfinite(_np(got.mesh.vertices)).all() and _np(got.mesh.vertices).min() >= 0.0 and _np(got.mesh.vertices).max() <= 1.0


def test_bad_input_is_counted_and_leaves_the_neighbours_alone():
    v, f = M.icosphere(2)
    V = len(v)
    clean, _ = _check(v, f, UNIT, "clean", cell=0.12)
    v_bad = np.concatenate([v, [[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, -np.inf]]]).astype(np.float32)
    bad = np.array([[0, 1, -1], [2, V + 3, 3], [4, R.INT_MIN, 5], [2**31 - 1, 6, 7], [0, 1, V], [V + 1, 2, 3], [V + 2, V + 2, V + 2]], np.int32)
    f_bad = np.concatenate([f[:5], bad[:3], f[5:], bad[3:]]).astype(np.int32)
    got, ref = _check(v_bad, f_bad, UNIT, "with bad faces and vertices", cell=0.12)
    assert (got.bad_vertices, got.bad_faces) == (3, 7)
    assert torch.equal(got.vertex_map[:V], clean.vertex_map) and (got.vertex_map[V:] == -1).all()
    for name in ("vertices", "faces", "normals"):                                             # the neighbours' bytes are unchanged
        assert np.array_equal(_bits(getattr(got.mesh, name)), _bits(getattr(clean.mesh, name))), name


# ---- invariance and determinism ---------------------------------------------------------------------------------------------------------------
def test_two_runs_write_the_same_bytes():
    import ngp_hip
    v, f = C.join(M.extracted_torus(), M.soup(500, 11), R.tessellated_cube(12))
    m = _mesh(v, f)
    runs = []
    for _ in range(2):
        got = ngp_hip.simplify_mesh(m, cell=0.05)
        runs.append([got.mesh.vertices, got.mesh.faces, got.mesh.normals, got.vertex_map, got.face_map])
        assert got.mesh.faces.shape[0] > 500
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def test_face_order_and_vertex_names_do_not_matter():
    v, f = M.extracted_torus()
    bounds = R.box_of(v)
    base, ref = _check(v, f, bounds, "torus", cell=0.07)
    rng = np.random.default_rng(12)
    perm = rng.permutation(len(f))
    got, _ = _check(v, f[perm], bounds, "torus, faces permuted", cell=0.07)
    assert torch.equal(got.vertex_map, base.vertex_map) and got.n_clusters == base.n_clusters
    fm, fm0 = _np(got.face_map), _np(base.face_map)[perm]
    assert np.array_equal(fm >= 0, fm0 >= 0) and np.array_equal(_np(got.mesh.faces)[fm[fm >= 0]], _np(base.mesh.faces)[fm0[fm0 >= 0]])
    assert (np.abs(_np(got.mesh.vertices).astype(np.float64) - _np(base.mesh.vertices)) <= 2 * ref["bound"]).all()      # each within one bound of the reference
    names = rng.permutation(len(v))                                                          # vertex i is now called names[i]
    v2, f2 = C.renumber(v, f, names)
    got2, _ = _check(v2, f2, bounds, "torus, vertices renamed", cell=0.07)
    assert np.array_equal(_np(got2.vertex_map)[names], _np(base.vertex_map))
    assert torch.equal(got2.face_map, base.face_map) and torch.equal(got2.mesh.faces, base.mesh.faces)
    assert (np.abs(_np(got2.mesh.vertices).astype(np.float64) - _np(base.mesh.vertices)) <= 2 * ref["bound"]).all()


def test_infinite_regularization_is_the_cluster_mean():
    v, f = M.icosphere(3)
    got, ref = _check(v, f, R.box_of(v), "icosphere, mean", regularization=INF, normals=False, resolution=7)
    quadric, _ = _check(v, f, R.box_of(v), "icosphere, quadric", resolution=7)
    assert torch.equal(got.mesh.faces, quadric.mesh.faces) and not torch.equal(got.mesh.vertices, quadric.mesh.vertices)
    vm = ref["vertex_map"]
    sums = np.zeros((ref["n_vertices"], 3))
    np.add.at(sums, vm[vm >= 0], v[vm >= 0].astype(np.float64))
    mean = sums / np.bincount(vm[vm >= 0], minlength=ref["n_vertices"])[:, None]
    assert np.abs(_np(got.mesh.vertices) - mean).max() < 1e-6


# ---- target_faces and the example ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, target", [("icosphere", 200), ("cube", 500), ("cube", 10**6)])
def test_target_faces(shape, target):
    import ngp_hip
    from ngp_hip import mesh
    v, f = M.icosphere(3) if shape == "icosphere" else R.tessellated_cube()
    got = ngp_hip.simplify_mesh(_mesh(v, f), target_faces=target)
    bounds = R.box_of(v)
    r = mesh.target_resolution(lambda r: R.count(v, f, *mesh.simplify_grid(bounds, resolution=r))["n_faces"], target, len(f))
    lo, h, n = mesh.simplify_grid(bounds, resolution=r)
    assert got.grid == n and got.mesh.faces.shape[0] <= target                                # the search the reference's counts give
    _compare(got, R.simplify(v, f, lo, h, n), "%s, target %d -> resolution %d" % (shape, target, r))
    if target >= len(f):                                                                      # the finest grid: nothing merges, nothing moves by more than a cell
        assert got.mesh.faces.shape[0] == len(f) and (got.mesh.vertices[got.vertex_map.long()].cpu() - torch.from_numpy(v)).abs().max() <= h.max()


def test_example_writes_at_most_the_target(tmp_path, capsys):
    """examples/extract_mesh.py --sdf --resolution 32 --target_faces 2000 on the small sphere fit of tests/test_gpu_mesh.py."""
    import importlib.util
    import os
    from conftest import ROOT
    from ngp_hip import mesh
    spec = importlib.util.spec_from_file_location("extract_mesh_example", os.path.join(ROOT, "examples", "extract_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = str(tmp_path / "sphere.ply")
    info = ex.main(["--sdf", "--steps", "300", "--n", "4096", "--log2_T", "14", "--levels", "8", "--max_res", "128", "--resolution", "32",
                    "--out", out, "--target_faces", "2000"])
    printed = capsys.readouterr().out
    written = mesh.read_ply(out)
    assert 0 < written.faces.shape[0] <= 2000 and written.faces.shape[0] == info["faces"] == info["simplify"]["faces"]
    assert info["simplify"]["before"]["faces"] > 2000 and "simplify_mesh:" in printed
    assert int(written.faces.max()) < written.vertices.shape[0] and written.normals is not None
