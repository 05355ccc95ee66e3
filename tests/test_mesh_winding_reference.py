"""The numpy reference of the winding-number contract (tests/mesh_winding_reference.py) against analytic truth, and the conditions its
named sets must meet, without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_sdf_reference as M
import mesh_winding_reference as W
from conftest import ROOT


def test_cube_is_one_inside_and_zero_outside():
    """Twelve faces, counter-clockwise seen from the outside (cross(b - a, c - a) outward): +1 inside, 0 outside -- the orientation for
    which the pseudonormal sign is negative inside."""
    v, f = M.cube()
    x = M.pts_uniform(v, 2048, np.random.default_rng(1))
    inside = M.box_sdf(x) < 0
    w = W.exact(x, v, f)
    assert 200 < inside.sum() < 1800
    assert np.abs(w - inside).max() <= 1e-12
    ref = M.brute_force(x, v, f, np.float64)
    sign = M.signed(ref, f, *M.pseudonormals(v, f))
    assert np.array_equal(sign < 0, inside) and np.array_equal(w >= 0.5, inside)


def test_icosphere_between_its_two_radii():
    v, f = M.icosphere()
    tri = v[f].astype(np.float64)
    centre = np.full((1, 3), 0.5)
    r_in = float(np.sqrt(M.closest_on_triangle(centre, tri[:, 0], tri[:, 1], tri[:, 2], np.float64)["d2"].min()))
    r_out = float(np.linalg.norm(v.astype(np.float64) - 0.5, axis=1).max())
    x = M.pts_uniform(v, 2048, np.random.default_rng(2))
    radius = np.linalg.norm(x.astype(np.float64) - 0.5, axis=1)
    w = W.exact(x, v, f)
    assert (radius < r_in).sum() > 200 and (radius > r_out).sum() > 200
    assert np.abs(w[radius < r_in] - 1.0).max() <= 1e-9 and np.abs(w[radius > r_out]).max() <= 1e-9


def test_single_triangle_against_the_octant():
    """(1,0,0), (0,1,0), (0,0,1) seen from the origin spans one octant: a solid angle of pi / 2, w = 1 / 8; from the other side of its
    plane the sign turns; on a vertex and for a face without area the term is 0 in both arithmetics."""
    a, b, c = np.eye(3, dtype=np.float32)
    for T, tol in ((np.float64, 1e-15), (np.float32, 4 * W.ULP1)):
        assert abs(float(W.solid_angle(np.zeros(3), a, b, c, T)) - np.pi / 2) <= tol * np.pi
        assert abs(float(W.solid_angle(np.zeros(3), a, c, b, T)) + np.pi / 2) <= tol * np.pi
        assert float(W.solid_angle(a, a, b, c, T)) == 0.0
        assert float(W.solid_angle(np.zeros(3), a, a, b, T)) == 0.0
        assert np.isfinite(W.solid_angle(np.array([[0.5, 0.5, 0.0], [1 / 3, 1 / 3, 1 / 3], [0.0, 0.0, 1.0]]), a, b, c, T)).all()
    assert abs(float(W.exact(np.zeros((1, 3)), np.eye(3, dtype=np.float32), np.array([[0, 1, 2]]))[0]) - 0.125) <= 1e-15
    assert float(W.solid_angle(np.full(3, 2.0), a, b, c, np.float64)) < 0


@pytest.mark.parametrize("name", ["cube/uniform", "icosphere/near", "soup500/uniform", "open_quad/near", "two_spheres/uniform"])
def test_tree_without_acceptance_is_the_exact_sum(name):
    c = W.case(name)
    for leaf_size in (1, 4):
        r = c.ref(W.INF, 2, leaf_size=leaf_size)
        err = np.abs(r["tree64"] - r["exact"]).max()
        print("%s leaf %d: |tree64(inf) - exact| %.3g, %d terms per point" % (name, leaf_size, err, r["terms"]))
        assert r["decided"].all() and r["terms"] == len(c.faces)
        assert err <= 1e-13 * max(1.0, len(c.faces) / 100)


def test_moments_of_the_root_and_the_radius():
    """Root of the icosphere: A = the area, N = 0 (closed), p = the centre, every r bounds the vertices below its node; the float32 rows
    follow the float64 rows."""
    c = W.case("icosphere/uniform")
    box, m64, m32 = c.moments()
    tri = c.vertices[c.faces].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert abs(m64[0, 7] - area.sum()) <= 1e-12 and np.abs(m64[0, 4:7]).max() <= 1e-12 and np.abs(m64[0, 0:3] - 0.5).max() <= 1e-6
    assert abs(m64[0, 8] + m64[0, 12] + m64[0, 16] - 3 * 4 / 3 * np.pi * 0.35**3) < 0.02                # trace T = 3 x the volume
    order = c.order()
    P, depth = W.shape(len(order), 4)
    below = {P - 1 + k: c.faces[order[4 * k:4 * k + 4]].reshape(-1) for k in range(P)}
    for i in range(P - 2, -1, -1):
        below[i] = np.concatenate([below[2 * i + 1], below[2 * i + 2]])
    for m in (m64, m32.astype(np.float64)):
        for i, idx in below.items():
            assert (m[i, 3] >= 0) == (len(idx) > 0) == (m[i, 17] == 1)
            if len(idx):
                assert m[i, 3] >= np.linalg.norm(c.vertices[idx].astype(np.float64) - m[i, 0:3], axis=1).max()
    assert np.abs(m32 - m64).max() <= 1e-5


@pytest.mark.parametrize("name", W.CASES)
def test_approximation_error_and_undecided_fraction(name):
    """A_set at beta = 2 is printed (profiles/microbench/mesh_winding.py writes the same figures to profiles/mesh_winding.json);
    the undecided fraction is a condition."""
    c = W.case(name)
    for terms in (1, 2):
        r = c.ref(2.0, terms)
        undecided = 1.0 - float(r["decided"].mean())
        print("%s order %d: A_set %.3g (mean %.3g), E32 %.3g, undecided %.4f, %.1f terms per point of %d faces"
              % (name, terms, r["a_set"], np.abs(r["tree64"] - r["exact"]).mean(), r["e32"], undecided, r["terms"], len(c.faces)))
        assert undecided <= W.MAX_UNDECIDED
        assert r["a_set"] <= 0.1 and r["e32"] <= 1e-4 and np.isfinite(r["tree32"]).all()
    if name.startswith("cube/"):
        assert c.ref(2.0, 2)["a_set"] <= 1e-12                        # a tree of three leaves never accepts from this near


def test_two_spheres_is_where_the_pseudonormal_sign_fails():
    v, f = W.two_spheres()
    x = np.concatenate([W.case("two_spheres/uniform").points, W.case("two_spheres/near").points])
    judged = W.two_spheres_judged(x)
    inside = W.two_spheres_sdf(x) < 0
    w = W.exact(x, v, f)
    assert judged.sum() > 600 and 100 < (inside & judged).sum()
    assert np.array_equal((w >= 0.5)[judged], inside[judged])
    ref = M.brute_force(x, v, f, np.float64)
    sign = M.signed(ref, f, *M.pseudonormals(v, f))
    wrong = judged & ((sign < 0) != inside)
    print("two spheres: %d judged points, %d inside the union, the pseudonormal sign is wrong on %d (all inside: %s), the winding number on 0"
          % (judged.sum(), (inside & judged).sum(), wrong.sum(), bool(inside[wrong].all())))
    assert wrong.sum() > 0 and inside[wrong].all()
    assert np.abs(w[judged & inside] - np.round(w[judged & inside])).max() <= 1e-9 and w[judged].max() <= 2 + 1e-9


def test_holed_sphere_degrades_gracefully():
    v, f = W.holed_sphere()
    assert 0 < 1280 - len(f) < 100
    rng = np.random.default_rng(5)
    hole = (np.array([0.5, 0.5, 0.85]) + np.concatenate([0.03 * rng.uniform(-1, 1, (64, 2)), 0.02 * rng.uniform(-1, 1, (64, 1))], 1)).astype(np.float32)
    w = W.exact(hole, v, f)
    print("holed sphere: %d faces removed; w near the hole %.3f .. %.3f" % (1280 - len(f), w.min(), w.max()))
    assert w.min() > 0.1 and w.max() < 0.9
    d = rng.standard_normal((256, 3))
    d[:, 2] = -np.abs(d[:, 2])
    far = (0.5 + 0.25 * rng.uniform(0, 1, (256, 1)) * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    far = np.concatenate([far, [[0.5, 0.5, 0.5]]]).astype(np.float32)
    w = W.exact(far, v, f)
    print("holed sphere: w at the centre %.4f, on the side away from the hole %.4f .. %.4f" % (w[-1], w.min(), w.max()))
    assert np.abs(w - 1.0).max() <= 0.05 and w.max() < 1.0


def test_boxes_restate_the_hierarchy():
    """The float32 boxes hold every vertex below them, widened; padding is inverted."""
    c = W.case("soup500/uniform")
    order = c.order()
    box = W.boxes(c.vertices, c.faces, order, 4)
    P, _ = W.shape(500, 4)
    assert box.shape == (2 * P - 1, 6) and np.isposinf(box[P - 1 + 125:, :3]).all() and np.isneginf(box[P - 1 + 125:, 3:]).all()
    for k in (0, 7, 124):
        pts = c.vertices[c.faces[order[4 * k:4 * k + 4]].reshape(-1)]
        assert (box[P - 1 + k, :3] < pts.min(0)).all() and (box[P - 1 + k, 3:] > pts.max(0)).all()
    assert (box[0, :3] < c.vertices.min(0)).all() and (box[0, 3:] > c.vertices.max(0)).all()


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    assert re.search(r"#define\s+NGP_ABI_VERSION\s+3\s", text)
    proto = re.search(r"int\s+ngp_mesh_winding_query\s*\(([^;]*)\)\s*;", text)
    assert proto
    args = [re.sub(r"\s+", " ", a).strip() for a in re.sub(r"/\*.*?\*/", "", proto.group(1)).split(",")]
    assert args == ["const float* points", "int n", "const float* vertices", "const int32_t* faces", "const int32_t* order",
                    "const float* moments", "int n_faces", "int leaf_size", "float beta", "int order_terms", "float* winding", "void* stream"]
    from ngp_hip import lib
    assert len(lib.SIGNATURES["ngp_mesh_winding_build"]) == 8 and len(lib.SIGNATURES["ngp_mesh_winding_query"]) == 12
    assert lib.RESTYPES["ngp_mesh_winding_bytes"] is ctypes.c_longlong and "mesh_winding.hip" in lib.SOURCES
    assert os.path.exists(os.path.join(lib.CSRC, "mesh_winding.hip"))


def test_meshsdf_refuses_an_unknown_sign_without_a_device():
    from ngp_hip import MeshSDF
    v, f = M.cube()
    with pytest.raises(ValueError, match="sign"):
        MeshSDF(v, f, sign="parity", device="cpu")
