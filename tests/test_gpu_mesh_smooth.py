"""Mesh smoothing on the GPU (csrc/mesh_smooth.hip through ngp_hip.adjacency, smooth_mesh and vertex_normals) against the serial
reference of the contract (tests/mesh_smooth_reference.py).

THE STANDARD ASSERTION (_check): the adjacency arrays, the vertex flags and the four counts equal the reference; every coordinate is
within the reference's `bound` (derived in its module docstring: one float32 spacing per pass, compounded by |1 - factor| + |factor|);
the normals are within `normal_bound` of the reference's normals OF THE DEVICE'S POSITIONS (the bound is one for identical inputs);
vertices the reference does not move keep the bits of the input.  Each check prints the worst ratios, and the module counts how many
checks were bit-identical in positions and normals.

vertex_normals weights by area, mesh_sdf.pseudonormals by angle: agreement in direction between the two is NOT asserted."""
import numpy as np
import pytest
import torch

import mesh_sdf_reference as M
import mesh_smooth_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TALLY = {"checks": 0, "positions_identical": 0, "normals_identical": 0}


def _mesh(v, f, normals=None):
    from ngp_hip import mesh
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return mesh.Mesh(t(np.asarray(v, np.float32).reshape(-1, 3)), t(np.asarray(f, np.int32).reshape(-1, 3)), normals)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = _np(a) if torch.is_tensor(a) else np.asarray(a, np.float32)
    return np.ascontiguousarray(a).view(np.int32)


def _same_adjacency(got, ref):
    assert got.row_start.dtype == torch.int32 and got.neighbours.dtype == torch.int32
    assert got.multiplicity.dtype == torch.uint8 and got.vertex_flags.dtype == torch.uint8
    e2, bad_faces, bad_vertices, boundary = ref["counts"]
    assert (int(got.neighbours.shape[0]), got.bad_faces, got.bad_vertices, got.boundary_vertices) == (e2, bad_faces, bad_vertices, boundary)
    for k in ("row_start", "neighbours", "multiplicity", "vertex_flags"):
        assert np.array_equal(_np(getattr(got, k)), ref[k]), k
    assert np.array_equal(_np(got.degree), np.diff(ref["row_start"])) and np.array_equal(_np(got.boundary), (ref["vertex_flags"] & R.BOUNDARY) != 0)


def _check(v, f, what="", adj=None, **kw):
    """The standard assertion on smooth_mesh(v, f, **kw) -> (the device's result, the reference's)."""
    import ngp_hip
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)
    fixed = kw.get("fixed")
    dev_kw = dict(kw, fixed=None if fixed is None else torch.from_numpy(np.asarray(fixed)).to(DEV))
    msh = _mesh(v, f)
    got = ngp_hip.smooth_mesh(msh, **dev_kw)
    ref = R.smooth(v, f, adj=adj, **{k: x for k, x in kw.items() if k != "normals"})
    assert got.mesh.faces is msh.faces and got.mesh.vertices.dtype == torch.float32 and got.mesh.vertices.shape == (len(v), 3)
    assert (got.bad_faces, got.bad_vertices) == ref["adjacency"]["counts"][1:3]
    _same_adjacency(got.adjacency, ref["adjacency"])
    x = _np(got.mesh.vertices)
    finite = np.isfinite(ref["vertices"])
    assert np.array_equal(_bits(x)[~finite], _bits(ref["vertices"])[~finite])
    err = np.abs(x[finite].astype(np.float64) - ref["vertices"][finite].astype(np.float64))
    worst = float(err.max() / ref["bound"]) if err.size and ref["bound"] > 0 else float(err.max() if err.size else 0.0)
    still = (_bits(ref["vertices"]) == _bits(v)).all(1)
    assert np.array_equal(_bits(x)[still], _bits(v)[still]), "a vertex the reference leaves alone moved"
    worst_n = 0.0
    nrm_same = True
    if kw.get("normals", True):
        n_ref, n_bound = R.vertex_normals(x, f)
        n = _np(got.mesh.normals)
        assert n.shape == x.shape and n.dtype == np.float32
        worst_n = float((np.linalg.norm(n.astype(np.float64) - n_ref.astype(np.float64), axis=1) / n_bound).max()) if len(n) else 0.0
        nrm_same = np.array_equal(_bits(n), _bits(n_ref))
    else:
        assert got.mesh.normals is None
    pos_same = np.array_equal(_bits(x), _bits(ref["vertices"]))
    TALLY["checks"] += 1
    TALLY["positions_identical"] += pos_same
    TALLY["normals_identical"] += nrm_same
    print("%s: V %d T %d passes %d; worst |device - reference| / bound: position %.3g, normal %.3g; bit-identical: positions %s, normals %s "
          "(so far %d / %d and %d / %d checks)" % (what, len(v), len(f), ref["passes"], worst, worst_n, pos_same, nrm_same,
                                                   TALLY["positions_identical"], TALLY["checks"], TALLY["normals_identical"], TALLY["checks"]))
    assert worst <= 1.0 and worst_n <= 1.0
    return got, ref


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 20000])
def test_disjoint_triangles_around_every_block_boundary(hip_lib, n):
    """Sizes around the 64-lane wave, the 256-lane block and the 512-slot chunk of the scan; every vertex is a boundary vertex of degree
    2.  "free" moves them all, "fixed" none."""
    v, f = R.disjoint_triangles(n)
    got, ref = _check(v, f, "disjoint_triangles(%d) free" % n, iterations=2, boundary="free")
    assert ref["adjacency"]["counts"] == (6 * n, 0, 0, 3 * n)
    got, _ = _check(v, f, "disjoint_triangles(%d) fixed" % n, iterations=2, boundary="fixed", adj=ref["adjacency"])
    assert np.array_equal(_bits(got.mesh.vertices), _bits(v))


def test_long_strip_in_random_face_order(hip_lib):
    n = 2**16 + 3
    v, f = R.strip(n)
    f = f[np.random.default_rng(3).permutation(n)]
    _, ref = _check(v, f, "strip curve", iterations=2, boundary="curve")
    _check(v, f, "strip free", iterations=1, boundary="free", max_move=0.05, adj=ref["adjacency"])


def test_empty_sides(hip_lib):
    """V > 0 with T = 0 (every vertex unused: nothing moves, the normals are 0) and V = 0 with T > 0 (every face bad)."""
    import ngp_hip
    v = np.random.default_rng(0).random((70, 3)).astype(np.float32)
    got, ref = _check(v, np.zeros((0, 3), np.int32), "no faces", iterations=3, boundary="free")
    assert np.array_equal(_bits(got.mesh.vertices), _bits(v)) and not _np(got.mesh.normals).any()
    assert (_np(got.adjacency.vertex_flags) == R.UNUSED).all() and ref["adjacency"]["counts"] == (0, 0, 0, 0)
    got, ref = _check(np.zeros((0, 3), np.float32), M.cube()[1], "no vertices", iterations=3)
    assert got.bad_faces == 12 and got.mesh.vertices.shape == (0, 3) and got.adjacency.row_start.tolist() == [0]
    assert ngp_hip.vertex_normals(_mesh(v, np.zeros((0, 3), np.int32))).shape == (70, 3)


@pytest.mark.parametrize("mode", R.MODES)
def test_hub_fan(hip_lib, mode):
    """One row of 10^4 neighbours (one lane walks it), a rim of 10^4 boundary vertices."""
    v, f, adj = R.case("fan")
    assert adj["row_start"][1] == 10**4 and adj["counts"][3] == 10**4
    got, ref = _check(v, f, "hub_fan " + mode, adj=adj, iterations=2, boundary=mode)
    assert (_bits(got.mesh.vertices)[0] != _bits(v)[0]).any()                      # the hub is interior: it moves in every mode
    assert (mode != "fixed") == bool((_bits(got.mesh.vertices)[1:] != _bits(v)[1:]).any())


@pytest.mark.parametrize("iterations", [1, 10])
@pytest.mark.parametrize("name", sorted(R.CLOSED))
def test_closed_shapes(hip_lib, name, iterations):
    v, f, adj = R.case(name)
    assert adj["counts"][3] == 0
    _check(v, f, "%s x %d" % (name, iterations), adj=adj, iterations=iterations)
    if iterations == 10:
        _check(v, f, "%s x 10, mu=None, bounded" % name, adj=adj, iterations=10, mu=None, max_move=(0.01, 0.02, 0.005))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", ["patch", "cylinder", "open_quad"])
def test_open_shapes_in_every_boundary_mode(hip_lib, name, mode):
    v, f, adj = R.case(name)
    assert adj["counts"][3] > 0
    _check(v, f, "%s %s" % (name, mode), adj=adj, iterations=5, boundary=mode)
    _check(v, f, "%s %s laplacian" % (name, mode), adj=adj, iterations=3, mu=0.0, boundary=mode, normals=False)


@pytest.mark.parametrize("duplicates", [3, 300])
def test_messy_mesh(hip_lib, duplicates):
    """Duplicate faces, both orientations, three faces on an edge, indices out of range, repeated indices, an isolated vertex, a NaN
    vertex in good faces; 300 copies of one face take its edges past the uint8 multiplicity's cut at 255."""
    import ngp_hip
    v, f = R.messy(duplicates)
    ref = R.brute_force_adjacency(v, f) if duplicates == 3 else R.adjacency(v, f)
    _same_adjacency(ngp_hip.adjacency(_mesh(v, f)), ref)
    assert (ref["multiplicity"].max() == 255) == (duplicates == 300)
    for mode in R.MODES:
        _check(v, f, "messy(%d) %s" % (duplicates, mode), adj=ref, iterations=3, boundary=mode)


def test_bad_input_keeps_good_output(hip_lib):
    """NaN and +-inf vertices and faces with wild indices mixed into a good mesh: every good vertex gets the reference's bytes (two
    passes from identical inputs: bit identity is what the same IEEE operations in the same order give)."""
    rng = np.random.default_rng(4)
    v, f = R.noisy_icosphere(3)
    v = v.copy()
    hit = rng.choice(len(v), 12, replace=False)
    v[hit[:4], 0], v[hit[4:8], 1], v[hit[8:], 2] = np.nan, np.inf, -np.inf
    wild = np.array([[0, 1, len(v)], [-5, 2, 3], [2**31 - 1, -2**31, 0], [7, 7, 8], [9, 10, 9], [-1, -1, -1]], np.int32)
    f = np.concatenate([f[:100], wild[:3], f[100:], wild[3:]]).astype(np.int32)
    got, ref = _check(v, f, "bad input", iterations=1)
    assert (got.bad_faces, got.bad_vertices) == (6, 12)
    good = np.isfinite(v).all(1)
    assert np.array_equal(_bits(got.mesh.vertices)[good], _bits(ref["vertices"])[good])
    assert np.array_equal(_bits(got.mesh.vertices)[~good], _bits(v)[~good]) and np.isfinite(_np(got.mesh.vertices)[good]).all()
    assert np.isfinite(_np(got.mesh.normals)).all()


def test_fixed_mask(hip_lib):
    v, f, adj = R.case("noisy_icosphere")
    pinned = np.zeros(len(v), bool)
    pinned[::3] = True
    got, ref = _check(v, f, "pinned", adj=adj, iterations=4, fixed=pinned.astype(np.uint8))
    free, _ = _check(v, f, "not pinned", adj=adj, iterations=4)
    x = _bits(got.mesh.vertices)
    assert np.array_equal(x[pinned], _bits(v)[pinned]) and (x[~pinned] != _bits(v)[~pinned]).any(1).all()
    assert (x[~pinned] != _bits(free.mesh.vertices)[~pinned]).any()                # the neighbours see the pinned positions


def test_identities(hip_lib):
    """iterations=0: the input's bits; two runs: the same bytes; face permutation and corner rotation: the same bytes; a precomputed
    adjacency: the same bytes as none, and with it smooth_mesh reads nothing back (torch's sync debug mode raises on a host read)."""
    import ngp_hip
    rng = np.random.default_rng(6)
    v, f, _ = R.case("noisy_icosphere")
    msh = _mesh(v, f)
    kw = dict(iterations=6, max_move=0.004)
    zero = ngp_hip.smooth_mesh(msh, iterations=0)
    assert np.array_equal(_bits(zero.mesh.vertices), _bits(v)) and zero.mesh.vertices.data_ptr() != msh.vertices.data_ptr()
    a, b = ngp_hip.smooth_mesh(msh, **kw), ngp_hip.smooth_mesh(msh, **kw)
    assert (_bits(a.mesh.vertices) != _bits(v)).any()
    assert np.array_equal(_bits(a.mesh.vertices), _bits(b.mesh.vertices)) and np.array_equal(_bits(a.mesh.normals), _bits(b.mesh.normals))
    g = np.stack([np.roll(t, k) for t, k in zip(f[rng.permutation(len(f))], rng.integers(0, 3, len(f)))]).astype(np.int32)
    c = ngp_hip.smooth_mesh(_mesh(v, g), **kw)
    assert np.array_equal(_bits(a.mesh.vertices), _bits(c.mesh.vertices))
    for k in ("row_start", "neighbours", "multiplicity", "vertex_flags"):
        assert torch.equal(getattr(a.adjacency, k), getattr(c.adjacency, k)), k
    adj = ngp_hip.adjacency(msh)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d = ngp_hip.smooth_mesh(msh, adjacency=adj, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert d.adjacency is adj and np.array_equal(_bits(a.mesh.vertices), _bits(d.mesh.vertices))
    assert np.array_equal(_bits(a.mesh.normals), _bits(d.mesh.normals))
    assert ngp_hip.smooth_mesh(msh, normals=False, **kw).mesh.normals is None


def test_octahedron_known_answer(hip_lib):
    """lam 0.5, mu -0.5, free: every coordinate is +-0.75^n or 0, bit for bit (tests/test_mesh_smooth_reference.py derives it)."""
    import ngp_hip
    v, f = R.octahedron()
    for n in (1, 5, 10, 15):
        got = ngp_hip.smooth_mesh(_mesh(v, f), iterations=n, lam=0.5, mu=-0.5, boundary="free")
        assert np.array_equal(_bits(got.mesh.vertices), _bits(v * np.float32(0.75 ** n))), n
        assert np.array_equal(_bits(got.mesh.normals), _bits(v)), n                 # the normals of an octahedron are its vertices


def test_dyadic_patch_known_answer(hip_lib):
    import ngp_hip
    v, f = R.dyadic_patch(8)
    for n in (1, 7, 30):
        got = ngp_hip.smooth_mesh(_mesh(v, f), iterations=n, boundary="fixed")
        assert np.array_equal(_bits(got.mesh.vertices), _bits(v)), n
    free = _bits(ngp_hip.smooth_mesh(_mesh(v, f), iterations=1, mu=0.0, boundary="free").mesh.vertices)
    assert (free[[0, 8, 72, 80]] != _bits(v)[[0, 8, 72, 80]]).any(1).all() and np.array_equal(free[40], _bits(v)[40])


def test_max_move_is_exact_after_fifty_iterations(hip_lib):
    """fl(x0 - max_move) <= x <= fl(x0 + max_move) in float32 on every coordinate, and a nonzero share of them sits on a bound."""
    import ngp_hip
    v, f = R.noisy_icosphere(3, amplitude=0.01)
    for mm in (0.004, (0.002, 0.004, 0.0)):
        got = ngp_hip.smooth_mesh(_mesh(v, f), iterations=50, max_move=mm)
        share = R.max_move_holds(_np(got.mesh.vertices), v, mm)
        print("max_move %r: %.1f %% of the coordinates on the bound" % (mm, 100 * share))
        assert share > 0.02
    _check(v, f, "50 iterations, bounded", iterations=50, max_move=0.004)


@pytest.mark.parametrize("name", sorted(R.CLOSED) + sorted(R.OPEN) + ["cancelling", "messy"])
def test_vertex_normals(hip_lib, name):
    """ngp_hip.vertex_normals against the reference, within normal_bound; twice the same bytes; exact zeros where the area vectors
    cancel.  (Area weights: no comparison with the angle-weighted mesh_sdf.pseudonormals.)"""
    import ngp_hip
    v, f = {"cancelling": R.cancelling, "messy": R.messy}[name]() if name in ("cancelling", "messy") else R.case(name)[:2]
    msh = _mesh(v, f)
    n = ngp_hip.vertex_normals(msh)
    ref, bound = R.vertex_normals(v, f)
    ratio = float((np.linalg.norm(_np(n).astype(np.float64) - ref.astype(np.float64), axis=1) / bound).max())
    same = np.array_equal(_bits(n), _bits(ref))
    print("%s: V %d; worst normal error / bound %.3g; bit-identical %s" % (name, len(v), ratio, same))
    assert n.dtype == torch.float32 and n.shape == (len(v), 3) and ratio <= 1.0
    assert np.array_equal(_bits(n), _bits(ngp_hip.vertex_normals(msh.vertices, msh.faces)))
    if name == "cancelling":
        assert not _np(n)[0].any() and np.array_equal(_np(n)[3], np.array([0, 0, 1], np.float32))


def test_example_smooths_between_cleaning_and_simplification(hip_lib, tmp_path, capsys, monkeypatch):
    """examples/extract_mesh.py --sdf --smooth 5 on the small sphere fit of tests/test_gpu_mesh.py: the new line is reported, V, T and
    the faces are what they are without the flag, no coordinate moves farther than half a cell.  And the flag's plumbing changes nothing
    else: with the smoothing call itself routed around (it hands the mesh back), --smooth 5 writes the bytes that no flag writes.  The
    fit runs once and is shared: the runs differ in the flag alone."""
    import importlib.util
    import os
    from conftest import ROOT
    from ngp_hip import mesh
    spec = importlib.util.spec_from_file_location("extract_mesh_example_smooth", os.path.join(ROOT, "examples", "extract_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    fits = []
    fit = ex.fit_sphere_sdf

    def fit_once(args, dev):
        if not fits:
            fits.append(fit(args, dev))
        return fits[0]
    monkeypatch.setattr(ex, "fit_sphere_sdf", fit_once)
    base = ["--sdf", "--steps", "300", "--n", "4096", "--log2_T", "14", "--levels", "8", "--max_res", "128", "--resolution", "32"]
    plain, smooth, around = [str(tmp_path / n) for n in ("plain.ply", "smooth.ply", "around.ply")]
    ex.main(base + ["--out", plain])
    assert "smooth_mesh:" not in capsys.readouterr().out
    info = ex.main(base + ["--out", smooth, "--smooth", "5"])
    assert "smooth_mesh:" in capsys.readouterr().out
    a, b = mesh.read_ply(plain), mesh.read_ply(smooth)
    rep = info["smooth"]
    assert a.vertices.shape == b.vertices.shape and torch.equal(a.faces, b.faces) and a.faces.shape[0] > 0 and b.normals is not None
    assert not torch.equal(a.vertices, b.vertices) and float((a.vertices - b.vertices).abs().max()) * 32 <= 0.5 + 1e-4
    assert rep["iterations"] == 5 and rep["seconds"] > 0 and rep["boundary_vertices"] == 0 and 0 < rep["mean_displacement_cells"] <= rep["max_displacement_cells"] <= 0.5 + 1e-4
    assert set(rep["sphere_distance_cells"]) == set(rep["face_normal_error_degrees"]) == {"before", "after"}
    assert rep["face_normal_error_degrees"]["after"] < rep["face_normal_error_degrees"]["before"]
    print("example --smooth 5:", rep)

    class Around:
        def __init__(self, m):
            self.mesh, self.adjacency, self.bad_faces, self.bad_vertices = m, mesh.adjacency(m), 0, 0
    monkeypatch.setattr(mesh, "smooth_mesh", lambda m, **kw: Around(m))
    ex.main(base + ["--out", around, "--smooth", "5"])
    assert open(around, "rb").read() == open(plain, "rb").read()
