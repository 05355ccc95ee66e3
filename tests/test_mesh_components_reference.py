"""The numpy reference of the connected-components contract (tests/mesh_components_reference.py) held to things that are not itself --
mesh.topology(), known meshes, exact areas and volumes -- and the binding of csrc/mesh_components.hip, without a GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_components_reference as R
import mesh_sdf_reference as M
from conftest import ROOT


def _topology(v, f):
    from ngp_hip import mesh
    return mesh.topology(mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), None))


@pytest.mark.parametrize("name", sorted(R.NAMED))
def test_the_table_adds_up_to_topology(name):
    """topology() counts every vertex and one chi for the whole soup: the rows sum to it once the unused vertices are added."""
    v, f, lab, tab = R.case(name)
    top = _topology(v, f)
    assert lab["bad_faces"] == 0
    assert int(tab["euler"].sum()) + lab["unused_vertices"] == top["euler"]
    assert int(tab["boundary_edges"].sum()) == top["boundary_edges"]
    assert int(tab["vertices"].sum()) + lab["unused_vertices"] == top["vertices"] and int(tab["faces"].sum()) == top["faces"]
    assert np.array_equal(tab["euler"], tab["vertices"] - tab["edges"] + tab["faces"])


def test_cube_exactly():
    v, f, lab, tab = R.case("cube")
    assert lab["n"] == 1 and tab["euler"].tolist() == [2] and tab["boundary_edges"].tolist() == [0] and tab["nonmanifold_edges"].tolist() == [0]
    assert tab["area"][0] == 6 * 0.25 and tab["volume"][0] == 0.125            # 0.25, 0.75 and every product are exact in binary
    assert tab["lo"].tolist() == [[0.25] * 3] and tab["hi"].tolist() == [[0.75] * 3]


def test_icosphere_torus_quad_needle():
    _, _, lab, tab = R.case("icosphere")
    assert lab["n"] == 1 and tab["euler"].tolist() == [2] and tab["boundary_edges"].tolist() == [0]
    assert 0.9 * 4 / 3 * math.pi * 0.35**3 < tab["volume"][0] < 4 / 3 * math.pi * 0.35**3        # inscribed, outward
    _, _, lab, tab = R.case("torus")
    assert lab["n"] == 1 and tab["euler"].tolist() == [0] and tab["boundary_edges"].tolist() == [0] and lab["unused_vertices"] == 0
    assert abs(tab["volume"][0] - 2 * math.pi**2 * 0.2 * 0.07**2) < 0.05 * tab["volume"][0]
    _, _, lab, tab = R.case("open_quad")
    assert lab["n"] == 1 and tab["boundary_edges"].tolist() == [4] and tab["euler"].tolist() == [1] and abs(tab["area"][0] - 0.36) < 1e-7
    _, _, lab, tab = R.case("needle")
    assert lab["n"] == 1 and tab["euler"].tolist() == [2] and tab["volume"][0] > 0


def test_shapes_with_shared_vertices_and_edges():
    _, _, lab, tab = R.case("two_apart")
    assert lab["n"] == 2 and tab["euler"].tolist() == [2, 2] and tab["vertices"].tolist() == [4, 4]
    assert np.allclose(tab["volume"], [8 / 3 * 0.1**3, 8 / 3 * 0.2**3], rtol=1e-6, atol=0)               # outward: positive
    v, f, lab, tab = R.case("two_sharing")
    assert len(v) == 7 and lab["n"] == 1 and tab["euler"].tolist() == [3] and tab["faces"].tolist() == [8] and tab["edges"].tolist() == [12]
    _, _, lab, tab = R.case("three_on_edge")
    assert lab["n"] == 1 and tab["nonmanifold_edges"].tolist() == [1] and tab["boundary_edges"].tolist() == [6] and tab["edges"].tolist() == [7]
    _, _, lab, tab = R.case("soup500")
    assert lab["n"] == 500 and (tab["boundary_edges"] == 3).all() and (tab["euler"] == 1).all()
    assert lab["vertex_component"].tolist() == [i // 3 for i in range(1500)]


def test_disjoint_icospheres_each_within_the_bound_of_its_own_sum():
    """k icospheres: C = k, numbered in the order they were joined, and a sphere alone has the table row it has in the union (the float
    fields within the bound; the union's vertices are the same float32 numbers)."""
    v, f, lab, tab = R.case("icospheres4")
    assert lab["n"] == 4 and tab["euler"].tolist() == [2] * 4 and tab["boundary_edges"].tolist() == [0] * 4
    for i in range(4):
        vi, fi = M.icosphere(1, centre=(float(i), 0.25 * i, -0.5 * i), radius=0.2 + 0.03 * i)
        one = R.table(vi, fi, R.label(fi, len(vi)))
        assert abs(one["area"][0] - tab["area"][i]) <= tab["area_bound"][i] and abs(one["volume"][0] - tab["volume"][i]) <= tab["volume_bound"][i]
        assert np.array_equal(one["lo"][0], tab["lo"][i]) and np.array_equal(one["hi"][0], tab["hi"][i])
        r = 0.2 + 0.03 * i
        assert 0.7 * 4 / 3 * math.pi * r**3 < tab["volume"][i] < 4 / 3 * math.pi * r**3


def test_bad_faces_unused_vertices_and_numbering():
    v, f = R.two_tetrahedra_apart()
    f = np.concatenate([f, [[0, 1, 8], [-1, 2, 3], [4, R.INT_MIN, 5], [5, 5, 6]]]).astype(np.int32)
    v = np.concatenate([v, np.ones((2, 3), np.float32)])               # vertices 8, 9
    lab = R.label(f, 10)                                                # (0, 1, 8) is good and uses 8; (5, 5, 6) is good; 9 is unused
    assert lab["bad_faces"] == 2 and lab["unused_vertices"] == 1 and lab["n"] == 2 and lab["vertex_component"].tolist() == [0] * 4 + [1] * 4 + [0, -1]
    lab = R.label(f, 8)
    assert lab["bad_faces"] == 3 and lab["face_component"].tolist() == [0] * 4 + [1] * 4 + [-1, -1, -1, 1]
    perm = np.random.default_rng(3).permutation(len(f))
    lab_p = R.label(f[perm], 8)
    assert np.array_equal(lab_p["vertex_component"], lab["vertex_component"]) and np.array_equal(lab_p["face_component"], lab["face_component"][perm])
    # the numbering follows the smallest vertex: swap the vertex names of the two tetrahedra
    swap = np.array([4, 5, 6, 7, 0, 1, 2, 3])
    _, f2 = R.renumber(v[:8], f[:8], swap)
    assert R.label(f2, 8)["face_component"].tolist() == [1] * 4 + [0] * 4


def test_select_and_rule():
    v, f, lab, tab = R.case("three_rankings")
    assert lab["n"] == 3
    pick = lambda by: R.rule(tab, keep_largest=1, by=by).tolist()
    assert pick("volume") == [True, False, False] and pick("faces") == [False, True, False] and pick("area") == [False, False, True]
    assert R.rule(tab).all() and R.rule(tab, closed_only=True).tolist() == [True, True, False]
    assert R.rule(tab, min_faces=81).tolist() == [False, True, False]
    s = R.select(v, None, f, lab, [False, True, False])
    assert len(s["vertices"]) == tab["vertices"][1] and len(s["faces"]) == tab["faces"][1] and s["faces"].min() == 0
    assert np.array_equal(s["vertices"][s["faces"]], v[f[lab["face_component"] == 1]])
    again = R.label(s["faces"], len(s["vertices"]))
    assert again["n"] == 1 and again["unused_vertices"] == 0


def test_the_package_rule_is_the_reference_rule():
    from ngp_hip import mesh
    _, _, _, tab = R.case("three_rankings")
    for kw in ({}, {"keep_largest": 1}, {"keep_largest": 2, "by": "faces"}, {"keep_largest": 1, "by": "volume"}, {"closed_only": True},
               {"min_faces": 81}, {"min_area_fraction": 0.3}, {"keep_largest": 0}):
        got = mesh.component_rule(tab["faces"], tab["boundary_edges"], tab["area"], tab["volume"], **kw)
        assert got.tolist() == R.rule(tab, **kw).tolist(), kw
    with pytest.raises(ValueError, match="by"):
        mesh.component_rule(tab["faces"], tab["boundary_edges"], tab["area"], tab["volume"], by="radius")


def test_binding():
    from ngp_hip import lib
    for name, n_args in (("ngp_mesh_components_rounds", 7), ("ngp_mesh_components_label", 9), ("ngp_mesh_components_edge_keys", 5),
                         ("ngp_mesh_components_table", 8), ("ngp_mesh_components_measure", 14), ("ngp_mesh_select_count", 11),
                         ("ngp_mesh_select_emit", 13)):
        assert len(lib.SIGNATURES[name]) == n_args, name
        assert lib.RESTYPES[name] is ctypes.c_int
    assert lib.RESTYPES["ngp_mesh_components_bytes"] is ctypes.c_longlong and lib.RESTYPES["ngp_mesh_components_partial_bytes"] is ctypes.c_longlong
    assert "mesh_components.hip" in lib.SOURCES and os.path.exists(os.path.join(lib.CSRC, "mesh_components.hip"))
    text = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    assert re.search(r"#define\s+NGP_ABI_VERSION\s+3\s", text)


def test_cpu_tensors_are_refused():
    import ngp_hip
    v, f = M.cube()
    m = ngp_hip.mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), None)
    with pytest.raises(RuntimeError, match="GPU"):
        ngp_hip.components(m)
    with pytest.raises(RuntimeError, match="GPU"):
        ngp_hip.clean_mesh(m)
    with pytest.raises(RuntimeError, match="GPU"):
        ngp_hip.ops.mesh_components_label(torch.from_numpy(f), 8)
    with pytest.raises(ValueError, match=r"\[T,3\]"):
        ngp_hip.ops.mesh_components_label(torch.from_numpy(f).reshape(-1), 8)
