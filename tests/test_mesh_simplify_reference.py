"""The serial reference of the simplification contract (tests/mesh_simplify_reference.py) held to things that are not itself -- the true
corners and volume of a cube, the plane of a planar patch, the cell size, the input's order -- and the binding of csrc/mesh_simplify.hip,
without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_sdf_reference as M
import mesh_simplify_reference as R
from conftest import ROOT

INF = float("inf")


def _grid(bounds, **kw):
    from ngp_hip import mesh
    return mesh.simplify_grid(bounds, **kw)


def _displacement_ok(v, out, h):
    """|x[vertex_map[v]] - v|_k <= h_k plus one float32 rounding of either side"""
    vm = out["vertex_map"]
    live = vm >= 0
    d = np.abs(out["vertices"][vm[live]].astype(np.float64) - np.asarray(v, np.float64)[live])
    slack = 2.0**-22 * np.maximum(np.abs(np.asarray(v, np.float64)[live]), np.abs(out["vertices"][vm[live]].astype(np.float64)))
    return bool((d <= np.asarray(h, np.float64) + slack).all())


def _size_ok(f, out):
    """T' <= T, V' <= C <= V, and the surviving faces are in input order with their corners renumbered, not reordered"""
    fm, vm = out["face_map"], out["vertex_map"]
    kept = fm[fm >= 0]
    f = np.asarray(f, np.int64)
    return out["n_faces"] <= len(f) and out["n_vertices"] <= out["n_clusters"] <= len(vm) and np.array_equal(kept, np.arange(out["n_faces"])) \
        and np.array_equal(out["faces"], vm[f[fm >= 0]])


_CUBE = {}


def cube_case(h, eps=1e-3):
    """The tessellated cube on the grid lo = 0, cell h: computed once per (h, regularization); callers must not modify it."""
    if (h, eps) not in _CUBE:
        v, f = R.tessellated_cube()
        lo, hh, n = _grid(((0, 0, 0), (1, 1, 1)), cell=h)
        _CUBE[(h, eps)] = (v, f, R.simplify(v, f, lo, hh, n, regularization=eps))
    return _CUBE[(h, eps)]


@pytest.mark.parametrize("h", [0.07, 0.11])
def test_the_quadric_point_keeps_the_cube(h):
    v, f, q = cube_case(h)
    _, _, m = cube_case(h, INF)
    assert len(v) == 3458 and len(f) == 6912 and R.volume(v, f) == pytest.approx(0.125, abs=1e-7)
    assert (q["n_vertices"], q["n_faces"]) == (m["n_vertices"], m["n_faces"]) and np.array_equal(q["faces"], m["faces"])
    cq, cm = R.corner_distance(q["vertices"]), R.corner_distance(m["vertices"])
    vq, vm = R.volume(q["vertices"], q["faces"]), R.volume(m["vertices"], m["faces"])
    print("h %.2f: V' %d T' %d; corner %.5f against %.5f (mean); volume %.6f against %.6f" % (h, q["n_vertices"], q["n_faces"], cq, cm, vq, vm))
    assert cq < 0.1 * cm                                                   # every true corner survives
    assert abs(vq - 0.125) < 0.1 * abs(vm - 0.125)
    assert vq > 0 and vm > 0                                               # the orientation is kept
    assert _displacement_ok(v, q, q_h(h)) and _displacement_ok(v, m, q_h(h)) and _size_ok(f, q)
    assert q["n_faces"] < len(f) // 4


def q_h(h):
    return np.full(3, np.float32(h), np.float64)


@pytest.mark.parametrize("h", [0.05, 0.083, 0.13])
def test_a_tilted_plane_stays_a_plane(h):
    v, f, nrm, p0 = R.tilted_patch()
    lo, hh, n = _grid(R.box_of(v), cell=h)
    out = R.simplify(v, f, lo, hh, n)
    assert out["n_faces"] > 0 and _displacement_ok(v, out, hh) and _size_ok(f, out)
    # the vertices lie exactly in the plane, so the exact representative is the cluster's mean, in the plane; the derived bound is what
    # the float64 sums and solve and the float32 rounding of the result may add (the reference's module docstring)
    off = np.abs((out["vertices"].astype(np.float64) - p0) @ nrm)
    allowed = np.linalg.norm(out["bound"], axis=1)
    print("h %.3f: V' %d, worst distance to the plane / allowed %.3g" % (h, out["n_vertices"], float((off / allowed).max())))
    assert (off <= allowed).all()
    assert np.abs(np.abs(out["normals"].astype(np.float64) @ nrm) - 1.0).max() < 1e-5


def test_every_vertex_alone_in_its_cell():
    v, f = R.spaced_triangles(40)
    lo, hh, n = _grid(R.box_of(v), cell=0.2)
    out = R.simplify(v, f, lo, hh, n)
    assert (out["n_vertices"], out["n_faces"], out["n_clusters"]) == (len(v), len(f), len(v))
    assert np.array_equal(out["face_map"], np.arange(len(f))) and _displacement_ok(v, out, hh) and _size_ok(f, out)
    assert np.abs(out["vertices"][out["vertex_map"]] - v).max() <= 0.1 + 1e-6          # inside its cell: half an edge


def test_everything_in_one_cell():
    v, f = M.icosphere(1)
    for kw in ({"resolution": 1}, {"cell": 10.0}):
        lo, hh, n = _grid(R.box_of(v), **kw)
        out = R.simplify(v, f, lo, hh, n)
        assert n == (1, 1, 1) and (out["n_clusters"], out["n_vertices"], out["n_faces"]) == (1, 0, 0)
        assert (out["vertex_map"] == -1).all() and (out["face_map"] == -1).all() and out["vertices"].shape == (0, 3) and _size_ok(f, out)


def test_bad_input_is_counted_and_leaves_the_neighbours_alone():
    v, f = M.icosphere(2)
    lo, hh, n = _grid(R.box_of(v), cell=0.12)
    clean = R.simplify(v, f, lo, hh, n)
    assert _displacement_ok(v, clean, hh) and _size_ok(f, clean)
    V = len(v)
    v_bad = np.concatenate([v, [[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, -np.inf]]]).astype(np.float32)
    bad = np.array([[0, 1, -1], [2, V + 3, 3], [4, R.INT_MIN, 5], [2**31 - 1, 6, 7], [0, 1, V], [V + 1, 2, 3], [V + 2, V + 2, V + 2]], np.int32)
    f_bad = np.concatenate([f[:5], bad[:3], f[5:], bad[3:]]).astype(np.int32)
    out = R.simplify(v_bad, f_bad, lo, hh, n)
    assert out["bad_vertices"] == 3 and out["bad_faces"] == 7 and out["n_clusters"] == clean["n_clusters"]
    assert (out["vertex_map"][V:] == -1).all() and np.array_equal(out["vertex_map"][:V], clean["vertex_map"])
    keep = np.concatenate([np.arange(5), np.arange(8, 8 + len(f) - 5)])
    assert np.array_equal(out["face_map"][keep], clean["face_map"]) and (np.delete(out["face_map"], keep) == -1).all()
    assert np.array_equal(out["faces"], clean["faces"])
    assert np.array_equal(out["vertices"].view(np.int32), clean["vertices"].view(np.int32))      # fsum: not a bit moves
    assert np.array_equal(out["normals"].view(np.int32), clean["normals"].view(np.int32))


def test_face_order_and_vertex_names_do_not_matter():
    v, f = M.extracted_torus()
    lo, hh, n = _grid(R.box_of(v), cell=0.07)
    base = R.simplify(v, f, lo, hh, n)
    assert _displacement_ok(v, base, hh) and _size_ok(f, base) and 0 < base["n_faces"] < len(f)
    rng = np.random.default_rng(12)
    perm = rng.permutation(len(f))
    out = R.simplify(v, f[perm], lo, hh, n)
    assert np.array_equal(out["vertex_cluster"], base["vertex_cluster"]) and np.array_equal(out["vertex_map"], base["vertex_map"])
    assert out["n_faces"] == base["n_faces"]
    assert np.array_equal(out["face_map"] >= 0, base["face_map"][perm] >= 0)
    assert np.array_equal(out["faces"][out["face_map"][out["face_map"] >= 0]], base["faces"][base["face_map"][perm][base["face_map"][perm] >= 0]])
    assert (np.abs(out["vertices"].astype(np.float64) - base["vertices"]) <= base["bound"]).all()
    names = rng.permutation(len(v))                                        # vertex i is now called names[i]
    v2 = np.empty_like(v)
    v2[names] = v
    out2 = R.simplify(v2, names[f.astype(np.int64)].astype(np.int32), lo, hh, n)
    assert np.array_equal(out2["vertex_cluster"][names], base["vertex_cluster"]) and np.array_equal(out2["vertex_map"][names], base["vertex_map"])
    assert np.array_equal(out2["face_map"], base["face_map"]) and np.array_equal(out2["faces"], base["faces"])
    assert (np.abs(out2["vertices"].astype(np.float64) - base["vertices"]) <= base["bound"]).all()


@pytest.mark.parametrize("shape, target", [("icosphere", 200), ("icosphere", 37), ("cube", 500), ("cube", 0)])
def test_target_faces(shape, target):
    from ngp_hip import mesh
    v, f = M.icosphere(3) if shape == "icosphere" else R.tessellated_cube()
    bounds, passes = R.box_of(v), []

    def count(r):
        passes.append(r)
        return R.count(v, f, *_grid(bounds, resolution=r))["n_faces"]
    r = mesh.target_resolution(count, target, len(f))
    got = R.count(v, f, *_grid(bounds, resolution=r))["n_faces"]
    print("%s target %d: resolution %d leaves %d faces after %d passes" % (shape, target, r, got, len(passes)))
    assert got <= target and len(passes) <= mesh.SIMPLIFY_MAX_PASSES and r >= 1
    assert target == 0 or got > target // 4                                # not a trivial answer
    assert mesh.target_resolution(count, len(f), len(f)) == mesh.SIMPLIFY_MAX_RESOLUTION and len(passes) <= mesh.SIMPLIFY_MAX_PASSES
    with pytest.raises(ValueError, match="target_faces"):
        mesh.target_resolution(count, -1, len(f))


def test_the_grid_the_host_chooses():
    lo, h, n = _grid(((0, 0, 0), (1, 2, 0.5)), resolution=8)
    assert n == (4, 8, 2) and h.dtype == np.float32 and h.tolist() == [0.25] * 3 and lo.tolist() == [0.0] * 3
    lo, h, n = _grid(((0, 0, 0), (1, 1, 1)), cell=(0.5, 0.25, 0.3))
    assert n == (2, 4, 4)
    assert _grid(((1, 1, 1), (1, 1, 1)), resolution=5)[2] == (1, 1, 1)
    for kw in ({}, {"cell": 0.1, "resolution": 3}, {"cell": 0.0}, {"cell": -1.0}, {"resolution": 0}, {"resolution": 2**21}, {"cell": 1e-9}):
        with pytest.raises(ValueError):
            _grid(((0, 0, 0), (1, 1, 1)), **kw)
    with pytest.raises(ValueError, match="bounds"):
        _grid(((0, 0, 0), (1, np.nan, 1)), cell=0.1)


def test_binding():
    from ngp_hip import lib
    for name, n_args in (("ngp_mesh_simplify_keys", 9), ("ngp_mesh_simplify_count", 12), ("ngp_mesh_simplify_incidence_keys", 7),
                         ("ngp_mesh_simplify_emit", 25)):
        assert len(lib.SIGNATURES[name]) == n_args, name
        assert lib.RESTYPES[name] is ctypes.c_int
    assert lib.RESTYPES["ngp_mesh_simplify_bytes"] is ctypes.c_longlong and lib.RESTYPES["ngp_mesh_simplify_runs_bytes"] is ctypes.c_longlong
    assert lib.SIGNATURES["ngp_mesh_simplify_emit"][19] is ctypes.c_double
    assert "mesh_simplify.hip" in lib.SOURCES and os.path.exists(os.path.join(lib.CSRC, "mesh_simplify.hip"))
    text = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    assert re.search(r"#define\s+NGP_ABI_VERSION\s+3\s", text)


def test_cpu_tensors_and_bad_arguments_are_refused():
    import ngp_hip
    v, f = M.cube()
    m = ngp_hip.mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f), None)
    assert ngp_hip.simplify_mesh is ngp_hip.mesh.simplify_mesh and ngp_hip.SimplifiedMesh._fields[:3] == ("mesh", "vertex_map", "face_map")
    with pytest.raises(RuntimeError, match="GPU"):
        ngp_hip.simplify_mesh(m, cell=0.1)
    with pytest.raises(RuntimeError, match="GPU"):
        ngp_hip.ops.mesh_simplify_count(m.vertices, m.faces, (0, 0, 0), (0.1,) * 3, (10,) * 3)
    for kw in ({}, {"cell": 0.1, "resolution": 4}, {"resolution": 4, "target_faces": 10}):
        with pytest.raises(ValueError, match="exactly one"):
            ngp_hip.simplify_mesh(m, **kw)
    with pytest.raises(ValueError, match=r"\[V,3\]"):
        ngp_hip.simplify_mesh((m.vertices.reshape(-1), m.faces), cell=0.1)
