"""Distance to a triangle mesh on the GPU (csrc/mesh_sdf.hip through ngp_hip.MeshSDF) against the numpy brute force of the contract
(tests/mesh_sdf_reference.py: float64 is the truth, the serial float32 restatement gives E32).

THE STANDARD ASSERTION (mesh_sdf_reference.judge; every test asserts it unless it says otherwise): | |sdf| - d64 | and, per axis,
|closest - closest64 on the returned face| within 4 x E32 of the set (E32 at least one float32 ulp of the quantity's scale: the floor
of tests/sdf_trace_reference.py); the returned face is A nearest face (its float64 distance within that bound of the minimum, indices
are not compared); the closest point lies on the feature the code names; the sign is exact on every decided point.  Sets named
on_surface are judged on the distance and on |x - closest| only."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_sdf_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mesh_sdf(case, **kw):
    from ngp_hip import MeshSDF
    return MeshSDF(torch.from_numpy(case.vertices), torch.from_numpy(case.faces), signed=case.signed_mode, **kw)


def _outputs(d):
    return tuple(x.cpu().numpy() for x in (d.sdf, d.closest, d.face, d.feature))


def _check(case, **kw):
    m = _mesh_sdf(case, **kw)
    d = m(_t(case.points))
    assert d.sdf.dtype == torch.float32 and d.closest.shape == (len(case.points), 3) and d.face.dtype == d.feature.dtype == torch.int32
    assert not d.sdf.requires_grad
    out = _outputs(d)
    R.judge(case, *out)
    return m, out


@pytest.mark.parametrize("name", R.CASES)
def test_named_cases(hip_lib, name):
    """One triangle (all seven regions, off the plane on both sides, in the plane, signed and unsigned), the needle tetrahedron, the
    cube, the icosphere and the extracted torus with points uniform in the box, near the surface, 10 x and 1000 x the box away, and the
    on-surface sets at vertices, edge midpoints and face centroids."""
    c = R.case(name)
    _, (sdf, _, _, feature) = _check(c)
    if name.startswith("triangle/regions"):
        assert set(feature.tolist()) == set(range(7))


def test_needle_needs_the_pseudonormals(hip_lib):
    """The test aimed at the obvious wrong implementation: on the needle's apex set the normal of the face the kernel returns, used
    alone, signs points wrongly (measured: 217 of 768 for the reference's faces, 232 for the kernel's; asserted > 0), while the
    kernel's sign is exact on every decided point (the standard assertion) and the whole set is decided and outside."""
    c = R.case("needle/apex")
    _, (sdf, closest, face, feature) = _check(c)
    assert c.undecided_fraction() == 0.0 and (sdf > 0).all()
    tri = c.vertices[c.faces[face]].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    by_face_normal = np.where((n * (c.points.astype(np.float64) - closest)).sum(1) >= 0, 1.0, -1.0)
    wrong = int((by_face_normal != c.ref()["sign"]).sum())
    print("needle/apex: the returned face's own normal would sign %d of %d points wrongly" % (wrong, len(sdf)))
    assert wrong > 0


_SOUPS = {}


def _soup_case(n_faces, **kw):
    key = (n_faces, tuple(sorted(kw.items())))
    if key not in _SOUPS:
        v, f = R.soup(n_faces, seed=n_faces, **kw)
        rng = np.random.default_rng(n_faces + 1)
        x = np.concatenate([R.pts_uniform(v, 320, rng), R.pts_near(v, f, 320, rng), v[rng.permutation(len(v))[:64]]])
        _SOUPS[key] = R.Case("soup%d%s" % (n_faces, "/same centroid" if kw else ""), v, f, x, signed_mode=False)
    return _SOUPS[key]


@pytest.mark.parametrize("leaf_size", [1, 4, 8])
@pytest.mark.parametrize("n_faces", [1, 2, 3, 5, 13, 4097])
def test_face_counts_and_leaf_sizes(hip_lib, n_faces, leaf_size):
    """Trees of one node up to 4097 leaves of one face (depth 13, 4095 of the 8192 leaves padding), unsigned triangle soups."""
    m, _ = _check(_soup_case(n_faces), leaf_size=leaf_size)
    leaves = -(-n_faces // leaf_size)
    assert m.boxes.shape == (2 * (1 << max(leaves - 1, 0).bit_length()) - 1, 6)


@pytest.mark.parametrize("leaf_size", [1, 8])
def test_signed_icosphere_other_leaf_sizes(hip_lib, leaf_size):
    _check(R.case("icosphere/uniform"), leaf_size=leaf_size)
    _check(R.case("icosphere/near"), leaf_size=leaf_size)


def test_mesh_far_from_the_origin(hip_lib):
    """The icosphere moved to lo = 100: coordinates lose 8 bits, the bound follows through E32 (r is formed in the face's frame, so the
    distance keeps its bits; closest carries the coordinates' rounding)."""
    v, f = R.icosphere()
    v = (v.astype(np.float64) + 100.0).astype(np.float32)
    rng = np.random.default_rng(100)
    c = R.Case("icosphere at 100", v, f, np.concatenate([R.pts_uniform(v, 512, rng), R.pts_near(v, f, 512, rng)]))
    assert c.undecided_fraction() <= R.MAX_UNDECIDED
    _check(c)
    print("icosphere at 100: E32 distance %.3g, closest %.3g" % (c.ref()["e32_d"], c.ref()["e32_c"]))


def test_one_morton_code_and_duplicated_faces(hip_lib):
    """200 faces around one centroid (the sort cannot separate them: the tree is as bad as it gets, the answer the same), and a cube one
    of whose faces is there 65 times."""
    _check(_soup_case(200, same_centroid=True, size=0.3))
    v, f = R.cube()
    f = np.concatenate([np.repeat(f[:1], 64, axis=0), f])
    rng = np.random.default_rng(64)
    c = R.Case("cube + 64 copies of a face", v, f, np.concatenate([R.pts_uniform(v, 384, rng), R.pts_near(v, f, 384, rng, 0.05)]), signed_mode=False)
    _check(c)
    _check(c, leaf_size=1)


def test_zero_area_face_is_never_returned(hip_lib):
    """Three collinear points with distinct indices (not dropped: `n_dropped` counts repeated indices only), laid through the surface of
    the icosphere, first in the face list; the points hug that segment.  The face has no area in float32, so no distance: it is never
    returned although it is nearer than any proper face, and no output is NaN (part of the standard assertion)."""
    v, f = R.icosphere()
    v = np.concatenate([v, [[0.5, 0.5, 0.75], [0.5, 0.5, 0.875], [0.5, 0.5, 1.0]]]).astype(np.float32)
    f = np.concatenate([[[len(v) - 3, len(v) - 2, len(v) - 1]], f]).astype(np.int32)
    rng = np.random.default_rng(9)
    x = np.stack([0.5 + 0.01 * rng.standard_normal(512), 0.5 + 0.01 * rng.standard_normal(512), rng.uniform(0.7, 1.05, 512)], 1).astype(np.float32)
    c = R.Case("icosphere + a zero-area face", v, f, np.concatenate([x, v[-3:]]))
    for leaf_size in (1, 4):
        m, (sdf, closest, face, _) = _check(c, leaf_size=leaf_size)
        assert m.n_dropped == 0 and m.n_faces == len(f)
        assert (face != 0).all()
        assert np.abs(sdf[:512]).max() > 0.05                         # the segment itself would have been within ~0.03 of every point


def test_open_quad_signs_by_the_side_of_the_nearest_feature(hip_lib):
    """An open mesh, the documented rule: the sign is the side of the nearest feature -- of the quad's plane, also beyond its border."""
    v, f = R.open_quad()
    rng = np.random.default_rng(4)
    x = rng.uniform(-0.2, 1.2, (1024, 3))
    x[:, 2] = 0.5 + np.where(rng.random(1024) < 0.5, -1.0, 1.0) * rng.uniform(0.02, 0.6, 1024)
    c = R.Case("open quad", v, f, x.astype(np.float32))
    assert c.undecided_fraction() <= R.MAX_UNDECIDED
    _, (sdf, _, _, feature) = _check(c)
    assert (np.sign(sdf) == np.sign(c.points[:, 2] - 0.5)).all()
    assert (feature > 0).sum() > 200                                  # beyond the border: edges and corners


@pytest.mark.parametrize("n_faces,leaf_size", [(1, 1), (13, 4), (4097, 1), (4097, 4), (4097, 8), (1280, 4)])
def test_hierarchy_invariants(hip_lib, n_faces, leaf_size):
    """Read back from the build: every face in exactly one leaf; every leaf box contains its faces' vertices and every inner box equals
    the union of its children's; padding is inverted; two builds give the same bytes."""
    from ngp_hip import MeshSDF
    v, f = R.icosphere() if n_faces == 1280 else R.soup(n_faces, seed=3)
    m = MeshSDF(torch.from_numpy(v), torch.from_numpy(f), leaf_size=leaf_size)
    again = MeshSDF(torch.from_numpy(v), torch.from_numpy(f), leaf_size=leaf_size)
    assert torch.equal(m.boxes.view(torch.int32), again.boxes.view(torch.int32)) and torch.equal(m.order, again.order)
    order, boxes = m.order.cpu().numpy(), m.boxes.cpu().numpy()
    assert np.array_equal(np.sort(order), np.arange(n_faces))
    leaves = -(-n_faces // leaf_size)
    P = (len(boxes) + 1) // 2
    assert P >= leaves and P & (P - 1) == 0 and (P == 1 or P // 2 < leaves)
    lo, hi = boxes[:, :3], boxes[:, 3:]
    for k in range(leaves):
        pts = v[f[order[k * leaf_size:(k + 1) * leaf_size]]].reshape(-1, 3)
        assert (lo[P - 1 + k] < pts.min(0)).all() and (hi[P - 1 + k] > pts.max(0)).all()               # widened: strictly
        side = (pts.max(0) - pts.min(0)).max()
        assert (pts.min(0) - lo[P - 1 + k]).max() <= side * 2.0**-17 + 2 * np.spacing(np.abs(pts).max())
    assert np.isposinf(lo[P - 1 + leaves:]).all() and np.isneginf(hi[P - 1 + leaves:]).all()
    inner = np.arange(P - 1)
    assert np.array_equal(lo[inner], np.minimum(lo[2 * inner + 1], lo[2 * inner + 2]))
    assert np.array_equal(hi[inner], np.maximum(hi[2 * inner + 1], hi[2 * inner + 2]))
    empty = np.isposinf(lo[:, 0])
    assert np.array_equal(empty[inner], empty[2 * inner + 1] & empty[2 * inner + 2]) and not empty[0]


@pytest.mark.parametrize("n", [0, 1, 65, 4096])
def test_batch_sizes_permutations_and_null_outputs(hip_lib, n):
    """A result depends on its point and the mesh alone: the same bits under a permutation of the batch, between two calls, and with
    closest / face / feature not asked for."""
    c = R.case("torus/uniform")
    m = _mesh_sdf(c)
    rng = np.random.default_rng(n)
    x = _t(np.concatenate([R.pts_uniform(c.vertices, n - n // 2, rng), R.pts_near(c.vertices, c.faces, n // 2, rng)]).astype(np.float32))
    a, b = m(x), m(x)
    assert a.sdf.shape == (n,) and a.closest.shape == (n, 3) and a.face.shape == (n,) and a.feature.shape == (n,)
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    perm = torch.from_numpy(rng.permutation(n)).to(DEV)
    s = m(x[perm].contiguous())
    for p, q in zip(a, s):
        assert torch.equal(p[perm].view(torch.int32), q.view(torch.int32))
    only = m(x, details=False)
    assert only.closest is None and only.face is None and only.feature is None
    assert torch.equal(only.sdf.view(torch.int32), a.sdf.view(torch.int32))
    if n:
        assert torch.isfinite(a.sdf).all() and int(a.face.min()) >= 0


def test_entries_refuse_bad_arguments(hip_lib):
    """-1, nothing launched or written: null pointers, n_faces < 1, a leaf_size outside 1..8, one normal array without the other, a
    tree deeper than the walk's 24 levels.  (Face indices are never out of range here: the entries trust them.)"""
    lib = hip_lib
    assert lib.ngp_mesh_bvh_bytes(1, 1) == 24 and lib.ngp_mesh_bvh_bytes(4097, 1) == 24 * (2 * 8192 - 1)
    assert lib.ngp_mesh_bvh_bytes(2**24, 1) == 24 * (2**25 - 1) and lib.ngp_mesh_bvh_bytes(2**24 + 1, 1) == -1
    assert lib.ngp_mesh_bvh_bytes(8 * 2**24, 8) > 0 and lib.ngp_mesh_bvh_bytes(8 * 2**24 + 1, 8) == -1
    assert lib.ngp_mesh_bvh_bytes(0, 4) == -1 and lib.ngp_mesh_bvh_bytes(10, 0) == -1 and lib.ngp_mesh_bvh_bytes(10, 9) == -1
    v, f = R.cube()
    tv, tf, order = _t(v), _t(f), torch.arange(12, device=DEV, dtype=torch.int32)
    boxes = torch.full((7, 6), 7.0, device=DEV)
    p = lambda t: t.data_ptr()
    assert lib.ngp_mesh_bvh_build(0, p(tf), p(order), 12, 4, p(boxes), 0) == -1
    assert lib.ngp_mesh_bvh_build(p(tv), 0, p(order), 12, 4, p(boxes), 0) == -1
    assert lib.ngp_mesh_bvh_build(p(tv), p(tf), 0, 12, 4, p(boxes), 0) == -1
    assert lib.ngp_mesh_bvh_build(p(tv), p(tf), p(order), 12, 4, 0, 0) == -1
    assert lib.ngp_mesh_bvh_build(p(tv), p(tf), p(order), 0, 4, p(boxes), 0) == -1
    assert lib.ngp_mesh_bvh_build(p(tv), p(tf), p(order), 12, 9, p(boxes), 0) == -1
    torch.cuda.synchronize()
    assert (boxes == 7.0).all()
    assert lib.ngp_mesh_bvh_build(p(tv), p(tf), p(order), 12, 4, p(boxes), 0) == 0
    x, sdf = torch.rand(8, 3, device=DEV), torch.full((8,), 7.0, device=DEV)
    en, vn = torch.zeros(12, 3, 3, device=DEV), torch.zeros(8, 3, device=DEV)
    q = lambda **kw: lib.ngp_mesh_sdf_query(*[kw.get(k, d) for k, d in (
        ("points", p(x)), ("n", 8), ("vertices", p(tv)), ("faces", p(tf)), ("order", p(order)), ("boxes", p(boxes)), ("n_faces", 12),
        ("leaf_size", 4), ("edge_normals", 0), ("vertex_normals", 0), ("sdf", p(sdf)), ("closest", 0), ("face", 0), ("feature", 0), ("stream", 0))])
    for bad in (dict(points=0), dict(vertices=0), dict(faces=0), dict(order=0), dict(boxes=0), dict(sdf=0), dict(n_faces=0), dict(n=-1),
                dict(leaf_size=0), dict(edge_normals=p(en)), dict(vertex_normals=p(vn))):
        assert q(**bad) == -1, bad
    torch.cuda.synchronize()
    assert (sdf == 7.0).all()
    assert q(n=0) == 0
    torch.cuda.synchronize()
    assert (sdf == 7.0).all()
    assert q() == 0 and q(edge_normals=p(en), vertex_normals=p(vn)) == 0
    torch.cuda.synchronize()
    assert (sdf != 7.0).all()


def test_meshsdf_validates_before_any_launch(hip_lib, monkeypatch):
    from ngp_hip import MeshSDF, mesh, ops

    def boom(*a, **k):
        raise AssertionError("a launch for a mesh that must be refused")
    monkeypatch.setattr(ops, "mesh_bvh_build", boom)
    v, f = R.cube()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    bad = tf.clone()
    bad[3, 1] = 8
    with pytest.raises(ValueError, match="indices"):
        MeshSDF(tv, bad)
    bad[3, 1] = -1
    with pytest.raises(ValueError, match="indices"):
        MeshSDF(tv, bad)
    with pytest.raises(ValueError, match="twice"):
        MeshSDF(tv, torch.tensor([[0, 0, 1], [2, 3, 3]], dtype=torch.int32))
    with pytest.raises(ValueError, match="empty"):
        MeshSDF(tv, torch.zeros(0, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        MeshSDF(tv.double(), tf)
    with pytest.raises(ValueError):
        MeshSDF(tv, tf.float())
    with pytest.raises(ValueError):
        MeshSDF(tv, tf, leaf_size=9)
    monkeypatch.undo()
    m = MeshSDF(tv, torch.cat([tf, torch.tensor([[0, 0, 1]], dtype=torch.int32)]))          # one face dropped, the others keep their numbers
    assert m.n_dropped == 1 and m.n_faces == 12
    c = R.case("cube/uniform")
    R.judge(c, *_outputs(m(_t(c.points))))
    soup = MeshSDF.from_mesh(mesh.Mesh(torch.from_numpy(v[f].reshape(-1, 3)), torch.arange(36, dtype=torch.int32).view(12, 3), None), weld=True)
    assert soup.vertices.shape == (8, 3)
    R.judge(c, *_outputs(soup(_t(c.points))))


def test_normal_sample_and_surface_distance(hip_lib):
    from ngp_hip import MeshSDF, mesh, surface_distance
    c = R.case("icosphere/uniform")
    m = _mesh_sdf(c)
    d = m(_t(c.points))
    radial = torch.nn.functional.normalize(_t(c.points) - 0.5, dim=1)
    assert float((d.normal() * radial).sum(1).min()) > 0.99                      # outwards on both sides of the surface
    on = m(_t(c.vertices[:100]))
    assert (on.sdf == 0).all() and (on.normal() == 0).all()
    g = lambda: torch.Generator().manual_seed(11)
    a, b = m.sample(4096, 0.01, 0.25, g()), m.sample(4096, 0.01, 0.25, g())
    assert a.shape == (4096, 3) and a.dtype == torch.float32 and a.is_cuda and torch.equal(a, b)
    da = m(a).sdf.abs()
    assert float(da[:3072].max()) < 0.06 and float(da[:3072].mean()) < 0.012 and float(da[3072:].mean()) > 0.05
    lo, hi = m.lo - 0.1 * 0.7, m.hi + 0.1 * 0.7
    assert (a[3072:] >= lo - 1e-6).all() and (a[3072:] <= hi + 1e-6).all()
    v, f = R.icosphere(radius=0.36)
    near = mesh.Mesh(torch.from_numpy(c.vertices), torch.from_numpy(c.faces), None)
    far = mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), None)
    sd = surface_distance(near, far, 8192, torch.Generator().manual_seed(2))
    print("surface_distance of two icospheres 0.01 apart:", sd)
    for key in ("a_to_b_mean", "a_to_b_max", "b_to_a_mean", "b_to_a_max", "mean", "max"):
        assert 0.0099 <= sd[key] <= 0.0112                                     # concentric: 0.01 along the normals, at most + a sagitta
    same = surface_distance(near, near, 4096, torch.Generator().manual_seed(2))
    assert same["max"] <= 1e-6


def test_fit_example_closes_the_loop(hip_lib, capsys):
    """examples/fit_sdf_mesh.py, 200 steps with small tables: mesh -> MeshSDF -> SDFField -> mesh.  The SDF loss falls, and the surface
    distance between the target torus and the extracted result falls below that of the untrained field (a sphere of radius 0.25) by a
    margin.  Measured on the MI355X (profiles/mesh_sdf_fit.json): mean distance 3.68 cells of the 48^3 extraction untrained (maximum
    12.7), 0.041 cells (maximum 0.24) after the 200 steps, SDF loss 0.068 -> 0.0015.  Asserted: the mean below a QUARTER of the
    untrained value (0.92 cells) -- a field that had not moved towards the torus would stay at 3.7, and a fit that is merely rough
    (a cell off on average) fails -- and the SDF loss below half its first value."""
    spec = importlib.util.spec_from_file_location("fit_sdf_mesh_example", os.path.join(ROOT, "examples", "fit_sdf_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    info = ex.main(["--steps", "200", "--n", "4096", "--log2_T", "14", "--levels", "8", "--max_res", "128", "--target_resolution", "32",
                    "--resolution", "48", "--compare_n", "8192"])
    before, after = info["surface_distance_untrained"], info["surface_distance"]
    print("fit: sdf loss %.4f -> %.4f, surface distance %.3f -> %.3f cells (max %.3f -> %.3f), query %.3f ms"
          % (info["sdf_loss_first"], info["sdf_loss_last"], before["mean_cells"], after["mean_cells"], before["max_cells"],
             after["max_cells"], info["query_ms_per_step"]))
    assert info["sdf_loss_last"] < 0.5 * info["sdf_loss_first"]
    assert after["mean_cells"] < 0.25 * before["mean_cells"]
    assert info["topology_target"]["euler"] == 0 and info["topology_target"]["boundary_edges"] == 0
    assert '"surface_distance"' in capsys.readouterr().out


def test_extract_example_compares_with_a_file(hip_lib, tmp_path, capsys):
    """examples/extract_mesh.py --compare PATH.ply: the fitted sphere (radius 0.3) against an icosphere of that radius read back from a
    file, with the fit of tests/test_gpu_mesh.py::test_example_extracts_the_fitted_sphere (300 steps: fewer leave no zero level at
    all).  That test bounds every vertex by fit error + sqrt(3) h with a fit error below 0.2; here: finite, mean below 0.1, maximum
    below 0.3, both ways."""
    from ngp_hip import mesh
    spec = importlib.util.spec_from_file_location("extract_mesh_example_compare", os.path.join(ROOT, "examples", "extract_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    v, f = R.icosphere(radius=0.3)
    ref = str(tmp_path / "sphere.ply")
    mesh.write_ply(ref, mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), None))
    info = ex.main(["--sdf", "--steps", "300", "--n", "4096", "--log2_T", "14", "--levels", "8", "--max_res", "128", "--resolution", "48",
                    "--out", str(tmp_path / "fit.obj"), "--compare", ref])
    sd = info["surface_distance"]
    print("extract_mesh --compare:", sd)
    assert all(np.isfinite(x) for x in sd.values()) and 0 < sd["mean"] < 0.1 and sd["max"] < 0.3
    assert '"surface_distance"' in capsys.readouterr().out
    back = mesh.read_obj(str(tmp_path / "fit.obj"))
    assert torch.equal(back.vertices.view(torch.int32), info["mesh"].vertices.cpu().view(torch.int32)) and torch.equal(back.faces, info["mesh"].faces.cpu())
