"""The numpy reference of the distance-to-mesh contract (tests/mesh_sdf_reference.py) against analytic truths, the conditions its named
sets must meet, and the host side of ngp_hip.mesh_sdf / ngp_hip.mesh (pseudonormals, welding, sampling, the mesh readers).  No GPU."""
import numpy as np
import pytest
import torch

import mesh_sdf_reference as R


def test_cube_mesh_is_the_exact_box_sdf():
    """Twelve faces with exactly representable corners: the float64 brute force with the pseudonormal sign IS max-norm box arithmetic,
    to the rounding of float64 (1e-12), inside, outside, next to faces, edges and corners."""
    for name in ("cube/uniform", "cube/near"):
        c = R.case(name)
        ref = c.ref()
        got = ref["sign"] * ref["r64"]["d"]
        want = R.box_sdf(c.points)
        assert (want < 0).sum() > 20 and (want > 0).sum() > 20
        assert np.abs(got - want).max() <= 1e-12, name
        assert set(np.unique(ref["r64"]["feature"])) == set(range(7)) or name == "cube/near"


def test_icosphere_is_the_sphere_within_the_sagitta():
    """1280 faces inscribed in the sphere: the mesh lies between the sphere and the sphere shrunk by the sagitta s = r - (the smallest
    distance of a face's plane from the centre), so |x - c| - r <= sdf <= |x - c| - r + s, and the sign is the sphere's wherever
    the point is not inside that shell."""
    v, f = R.icosphere()
    assert len(f) == 1280
    tri = v[f].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    plane = np.abs(((tri[:, 0] - 0.5) * n).sum(1)) / np.linalg.norm(n, axis=1)
    s = 0.35 - plane.min()
    assert 0 < s < 0.002
    for name in ("icosphere/uniform", "icosphere/near", "icosphere/far10"):
        c = R.case(name)
        ref = c.ref()
        got = ref["sign"] * ref["r64"]["d"]
        want = np.linalg.norm(c.points.astype(np.float64) - 0.5, axis=1) - 0.35
        assert (got >= want - 1e-6).all() and (got <= want + s + 1e-6).all(), name
        clear = (want > 0) | (want < -s - 1e-6)
        assert (np.sign(got[clear]) == np.sign(want[clear])).all()


def _inside_tetrahedron(x, v, f):
    tri = v[f].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return ((x[:, None, :].astype(np.float64) - tri[None, :, 0]) * n[None]).sum(-1).max(1) < 0


def test_needle_face_normals_sign_wrongly_pseudonormals_do_not():
    """Around the apex of the needle tetrahedron the nearest feature is the apex or a long edge (no point of the set is nearest to the
    base).  The normal of the nearest FACE alone gives the wrong side for 217 of the 768 points (whichever of the faces that share the
    feature the minimum falls on decides); the pseudonormal of the feature gives the half-space truth for every one."""
    c = R.case("needle/apex")
    ref = c.ref()
    truth = np.where(_inside_tetrahedron(c.points, c.vertices, c.faces), -1.0, 1.0)
    feature = ref["r64"]["feature"]
    assert (feature >= 4).sum() > 100 and ((feature >= 1) & (feature <= 3)).sum() > 100
    wrong_face = int((R.face_normal_sign(ref["r64"]) != truth).sum())
    print("needle/apex: the face normal signs %d of %d points wrongly" % (wrong_face, len(truth)))
    assert wrong_face == 217
    assert (ref["sign"] == truth).all()
    u = R.case("needle/uniform")
    truth_u = np.where(_inside_tetrahedron(u.points, u.vertices, u.faces), -1.0, 1.0)
    assert (u.ref()["sign"] == truth_u).all()


@pytest.mark.parametrize("name", R.SIGNED_SETS)
def test_named_sets_are_decided(name):
    """The cap of tests/test_gpu_sdf_trace.py: at most 2 % of a set may be left undecided, by the float64 reference alone."""
    c = R.case(name)
    assert c.undecided_fraction() <= R.MAX_UNDECIDED, (name, c.undecided_fraction())
    ref = c.ref()
    assert np.isfinite(ref["r32"]["d"]).all() and ref["e32_d"] > 0 and ref["e32_c"] > 0


def test_serial_float32_stays_near_float64():
    """E32 is an error, not a blunder: on the sets away from slivers it is a few ulps of the coordinates."""
    for name in ("icosphere/uniform", "cube/uniform", "triangle/regions", "torus/near"):
        ref = R.case(name).ref()
        scale = max(np.abs(R.case(name).points).max(), 1.0)
        assert ref["e32_d"] <= 64 * R.EPS * scale and ref["e32_c"] <= 64 * R.EPS * scale, name


def test_zero_area_face_has_no_distance():
    p = np.array([[0.3, 0.4, 0.5]], np.float32)
    a, b, c = (np.array([x], np.float32) for x in ([0, 0, 0], [0.5, 0, 0], [1, 0, 0]))
    for T in (np.float32, np.float64):
        assert np.isnan(R.closest_on_triangle(p, a, b, c, T)["d2"]).all()
        assert np.isnan(R.closest_on_triangle(p, a, a, c, T)["d2"]).all()
    v = np.concatenate([R.cube()[0], [[0.5, 0.9, 0.5], [0.5, 1.0, 0.5], [0.5, 1.1, 0.5]]]).astype(np.float32)
    f = np.concatenate([[[8, 9, 10]], R.cube()[1]]).astype(np.int32)
    out = R.brute_force(np.array([[0.5, 0.95, 0.5]], np.float32), v, f, np.float64)
    assert out["face"][0] != 0 and abs(out["d"][0] - 0.2) < 1e-7


# ---- the package's host side ----------------------------------------------------------------------------------------------------------
def test_pseudonormals_of_a_closed_mesh():
    """Edge normals are the sum of the two adjacent unit normals; the vectorised construction equals the reference's dictionaries."""
    from ngp_hip import mesh_sdf
    for v, f in (R.cube(), R.icosphere(1), R.needle_tetrahedron()):
        edge, vertex = mesh_sdf.pseudonormals(v, f)
        want_e, want_v = R.pseudonormals(v, f)
        assert np.abs(edge - want_e).max() <= 1e-12 and np.abs(vertex - want_v).max() <= 1e-12
        tri = v[f].astype(np.float64)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        unit = n / np.linalg.norm(n, axis=1, keepdims=True)
        for t in range(len(f)):
            for e in range(3):
                i, j = f[t, e], f[t, (e + 1) % 3]
                other = [u for u in range(len(f)) if u != t and i in f[u] and j in f[u]]
                assert len(other) == 1
                assert np.abs(edge[t, e] - (unit[t] + unit[other[0]])).max() <= 1e-12
    v, f = R.cube()
    _, vertex = mesh_sdf.pseudonormals(v, f)
    d = (v.astype(np.float64) - 0.5) / np.linalg.norm(v.astype(np.float64) - 0.5, axis=1, keepdims=True)
    assert np.abs(vertex / np.linalg.norm(vertex, axis=1, keepdims=True) - d).max() <= 1e-12          # a cube's corners: the diagonal


def test_weld_turns_a_soup_back_into_the_indexed_mesh():
    from ngp_hip import mesh_sdf
    v, f = R.icosphere(2)
    soup_v = v[f].reshape(-1, 3)
    soup_f = np.arange(len(soup_v)).reshape(-1, 3)
    welded, index = mesh_sdf.weld_vertices(soup_v)
    assert len(welded) == len(v) and np.array_equal(welded[index], soup_v)
    edge, vertex = mesh_sdf.pseudonormals(welded, index[soup_f])
    want_e, want_v = mesh_sdf.pseudonormals(v, f)
    assert np.abs(edge - want_e).max() <= 1e-12                                  # the faces keep their order
    back = index[soup_f].reshape(-1)                                              # welded index of every corner of the indexed mesh
    assert np.abs(vertex[back] - want_v[f.reshape(-1)]).max() <= 1e-12
    loose_e, _ = mesh_sdf.pseudonormals(soup_v, soup_f)                         # without welding every edge has one face
    assert np.abs(np.linalg.norm(loose_e, axis=2) - 1.0).max() <= 1e-12


def test_ply_and_obj_round_trip(tmp_path):
    from ngp_hip import mesh
    v, f = R.icosphere(1)
    rng = np.random.default_rng(3)
    v = (v * rng.uniform(0.1, 1000.0, v.shape)).astype(np.float32)
    n = rng.standard_normal(v.shape).astype(np.float32)
    for normals in (None, n):
        m = mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), None if normals is None else torch.from_numpy(normals))
        mesh.write_ply(str(tmp_path / "a.ply"), m)
        back = mesh.read_ply(str(tmp_path / "a.ply"))
        assert back.vertices.dtype == torch.float32 and back.faces.dtype == torch.int32
        assert np.array_equal(back.vertices.numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(back.faces.numpy(), f)
        assert (back.normals is None) == (normals is None)
        if normals is not None:
            assert np.array_equal(back.normals.numpy().view(np.uint32), n.view(np.uint32))
        mesh.write_obj(str(tmp_path / "a.obj"), m)
        back = mesh.read_obj(str(tmp_path / "a.obj"))
        assert np.array_equal(back.vertices.numpy().view(np.uint32), v.view(np.uint32))        # nine digits carry a float32
        assert np.array_equal(back.faces.numpy(), f) and (back.normals is None) == (normals is None)
        if normals is not None:
            assert np.array_equal(back.normals.numpy().view(np.uint32), n.view(np.uint32))
    empty = mesh.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), None)
    mesh.write_ply(str(tmp_path / "e.ply"), empty)
    assert mesh.read_ply(str(tmp_path / "e.ply")).faces.shape == (0, 3)


def test_readers_refuse_what_the_writers_do_not_produce(tmp_path):
    from ngp_hip import mesh
    p = tmp_path / "x.ply"
    p.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nelement face 0\n"
                  b"property list uchar int vertex_indices\nend_header\n")
    with pytest.raises(ValueError):
        mesh.read_ply(str(p))
    p.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                  b"element face 0\nproperty list uchar int vertex_indices\nend_header\n\0\0\0\0")              # a short body
    with pytest.raises(ValueError):
        mesh.read_ply(str(p))
    p.write_bytes(b"not a ply")
    with pytest.raises(ValueError):
        mesh.read_ply(str(p))
    o = tmp_path / "x.obj"
    for text in ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3 1\n", "v 0 0 0\nvt 0 0\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/1 2/2 3/3\n",
                 "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//2 3//3\n"):
        o.write_text(text)
        with pytest.raises(ValueError):
            mesh.read_obj(str(o))


def test_sample_surface_is_deterministic_and_on_the_faces():
    from ngp_hip import mesh_sdf
    v, f = R.cube()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    a, ia = mesh_sdf.sample_surface(tv, tf, 4096, torch.Generator().manual_seed(5))
    b, ib = mesh_sdf.sample_surface(tv, tf, 4096, torch.Generator().manual_seed(5))
    c, _ = mesh_sdf.sample_surface(tv, tf, 4096, torch.Generator().manual_seed(6))
    assert torch.equal(a, b) and torch.equal(ia, ib) and not torch.equal(a, c)
    assert np.abs(R.box_sdf(a.numpy())).max() <= 1e-6
    counts = np.bincount(ia.numpy(), minlength=12)                 # twelve equal areas: 341 each, five standard deviations = 90
    assert counts.min() > 250 and counts.max() < 432
    stretched = tv * torch.tensor([1.0, 1.0, 8.0])                 # the four long sides now hold 8/9 of the area... of each pair
    _, idx = mesh_sdf.sample_surface(stretched, tf, 4096, torch.Generator().manual_seed(5))
    share = np.bincount(idx.numpy(), minlength=12)[[0, 1, 2, 3, 4, 5, 6, 7]].sum() / 4096.0            # the faces of the -x +x -y +y sides
    assert abs(share - 16.0 / 17.0) < 0.02                          # areas 4 x (0.5 x 4) against 2 x (0.5 x 0.5)
