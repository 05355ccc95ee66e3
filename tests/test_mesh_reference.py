"""CPU tier of the isosurface extraction: the numpy reference (tests/mesh_reference.py) is pinned to the values a serial loop prototype
of the same contract gave, the mesh writers round-trip, and the host side of the new entry points (source list, header, argument
checks) is in place.  The kernels themselves are held to this reference in test_gpu_mesh.py."""
import os
import re

import numpy as np
import pytest

import mesh_reference as mr
from conftest import ROOT


@pytest.fixture(scope="module")
def sphere():
    pts, h = mr.unit_grid(17)
    field = mr.sphere_sdf(pts)
    return field, h, mr.marching_tetrahedra(field, 0.0, -1, (0, 0, 0), (h, h, h), normals=True)


def test_sphere_sdf_is_a_closed_oriented_sphere(sphere):
    _, _, m = sphere
    v, f = m["vertices"], m["faces"]
    assert v.shape == (1302, 3) and f.shape == (2600, 3) and f.dtype == np.int32
    topo = mr.edge_topology(f)
    assert set(topo["undirected"].values()) == {2} and set(topo["directed"].values()) == {1}
    assert topo["closed"] and not topo["boundary"]
    assert mr.euler(len(v), f) == 2
    vol, true = mr.signed_volume(v, f), 4 * np.pi * 0.3**3 / 3
    assert abs(vol - 0.11063) < 5e-6
    assert 0 < (true - vol) / true < 0.05                     # the chords of a convex body lie inside it
    # outward normals: along the radius
    rad = v - np.array([0.5, 0.47, 0.52])
    assert ((m["normals"] * rad).sum(1) / np.linalg.norm(rad, axis=1)).min() > 0.99


def test_serial_f32_mode_stays_within_one_ulp_of_the_unit_box(sphere):
    field, h, m = sphere
    m32 = mr.marching_tetrahedra(field, 0.0, -1, (0, 0, 0), (h, h, h), dtype=np.float32)
    assert m32["vertices"].dtype == np.float32 and np.array_equal(m32["faces"], m["faces"])
    assert np.abs(m32["vertices"].astype(np.float64) - m["vertices"]).max() <= 2.0**-24


def test_the_same_field_as_a_density_gives_identical_faces(sphere):
    field, h, m = sphere
    d = mr.marching_tetrahedra(np.float32(1) - np.float32(10) * field, 1.0, +1, (0, 0, 0), (h, h, h))
    assert np.array_equal(d["faces"], m["faces"])
    assert np.abs(d["vertices"] - m["vertices"]).max() < 1e-5


def test_torus_has_genus_one():
    pts, h = mr.unit_grid(17)
    m = mr.marching_tetrahedra(mr.torus_sdf(pts), 0.0, -1, (0, 0, 0), (h, h, h))
    assert mr.edge_topology(m["faces"])["closed"] and mr.euler(len(m["vertices"]), m["faces"]) == 0
    assert mr.signed_volume(m["vertices"], m["faces"]) > 0


def test_random_field_padded_with_outside_is_closed():
    f = mr.padded_random()
    assert f.shape == (9, 8, 7)
    m = mr.marching_tetrahedra(f, 0.0, +1)
    assert len(m["vertices"]) == 886 and len(m["faces"]) == 1776
    assert mr.edge_topology(m["faces"])["closed"]


def test_non_finite_values_keep_the_mesh_closed_and_finite():
    f = mr.nonfinite_field()
    assert np.isnan(f).sum() == 1 and np.isposinf(f).sum() == 1 and np.isneginf(f).sum() == 1 and (f[1:-1, 1:-1, 1:-1] == 0).sum() == 1
    for dtype in (np.float64, np.float32):
        m = mr.marching_tetrahedra(f, 0.0, +1, normals=True, dtype=dtype)
        assert mr.edge_topology(m["faces"])["closed"]
        assert np.isfinite(m["vertices"]).all() and np.isfinite(m["normals"]).all()
    ins = mr.inside_mask(f, 0.0, +1)
    assert not ins[3, 3, 3] and ins[4, 2, 3] and not ins[2, 4, 2] and not ins[5, 3, 4]        # NaN, +inf, -inf, == iso


def test_all_256_corner_masks_of_one_cell():
    mag = np.random.default_rng(3).uniform(0.5, 2.0, 8).astype(np.float32)
    for mask in range(256):
        bits = np.array([(mask >> c) & 1 for c in range(8)], dtype=bool).reshape(2, 2, 2)       # corner code 4 dx + 2 dy + dz
        for sign in (+1, -1):
            field = np.where(bits, sign, -sign).astype(np.float32) * mag.reshape(2, 2, 2)
            m = mr.marching_tetrahedra(field, 0.0, sign)
            if mask in (0, 255):
                assert len(m["vertices"]) == 0 and len(m["faces"]) == 0
                continue
            assert len(m["faces"]) > 0
            assert np.array_equal(np.unique(m["faces"]), np.arange(len(m["vertices"])))        # every vertex is referenced
            assert (m["vertices"] >= 0).all() and (m["vertices"] <= 1).all()
    # complementary masks cut the same edges, with the opposite orientation
    a = mr.marching_tetrahedra(np.where(np.arange(8) < 3, 1, -1).astype(np.float32).reshape(2, 2, 2), 0.0, +1)
    b = mr.marching_tetrahedra(np.where(np.arange(8) < 3, -1, 1).astype(np.float32).reshape(2, 2, 2), 0.0, +1)
    assert np.array_equal(a["vertices"], b["vertices"]) and len(a["faces"]) == len(b["faces"])
    assert set(mr.edge_topology(a["faces"])["directed"]) == {(q, p) for p, q in mr.edge_topology(b["faces"])["directed"]}


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int(re.search(r"element vertex (\d+)", head.decode()).group(1))
    nf = int(re.search(r"element face (\d+)", head.decode()).group(1))
    props = [ln.split()[-1] for ln in lines if ln.startswith("property float")]
    v = np.frombuffer(body, dtype="<f4", count=nv * len(props)).reshape(nv, len(props))
    rows = np.frombuffer(body, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=nf, offset=4 * nv * len(props))
    assert len(body) == 4 * nv * len(props) + 13 * nf and (rows["n"] == 3).all()
    return props, v, rows["idx"]


def test_write_ply_and_obj_round_trip(sphere, tmp_path):
    from ngp_hip import mesh
    _, _, m = sphere
    v32, n32 = m["vertices"].astype(np.float32), m["normals"].astype(np.float32)
    for with_normals in (True, False):
        msh = mesh.Mesh(v32, m["faces"], n32 if with_normals else None)
        mesh.write_ply(str(tmp_path / "s.ply"), msh)
        props, v, f = _read_ply(str(tmp_path / "s.ply"))
        assert props == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
        assert np.array_equal(f, m["faces"]) and np.array_equal(v[:, :3], v32)                 # binary f32: exact
        assert not with_normals or np.array_equal(v[:, 3:], n32)
        mesh.write_obj(str(tmp_path / "s.obj"), msh)
        lines = open(str(tmp_path / "s.obj")).read().split("\n")
        ov = np.array([ln.split()[1:] for ln in lines if ln.startswith("v ")], dtype=np.float64).astype(np.float32)
        on = np.array([ln.split()[1:] for ln in lines if ln.startswith("vn ")], dtype=np.float64).astype(np.float32)
        of = np.array([[int(t.split("/")[0]) for t in ln.split()[1:]] for ln in lines if ln.startswith("f ")]) - 1
        assert np.array_equal(of, m["faces"]) and np.array_equal(ov, v32)                      # nine digits: an f32 survives
        assert (np.array_equal(on, n32) if with_normals else on.size == 0)


def test_library_surface_of_the_extraction(hip_lib):
    import torch
    from ngp_hip import lib, ops
    assert "mesh.hip" in lib.SOURCES
    hdr = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    for name in ("ngp_mesh_workspace_bytes", "ngp_mesh_count", "ngp_mesh_emit"):
        assert re.search(r"\b(?:int|long long)\s+%s\s*\(" % name, hdr) and name in lib.SIGNATURES and hasattr(hip_lib, name)
    assert hip_lib.ngp_abi_version() == 3
    # 4 bytes per point + 8 per 512-point chunk, every array rounded up to 16 bytes
    assert hip_lib.ngp_mesh_workspace_bytes(513, 513, 513) <= 8 * 513**3
    assert hip_lib.ngp_mesh_workspace_bytes(64, 64, 64) == 4 * 64**3 + 8 * 64**3 // 512
    assert hip_lib.ngp_mesh_workspace_bytes(1, 64, 64) == -1 and hip_lib.ngp_mesh_workspace_bytes(2048, 1024, 1024) == -1
    # the C entry points refuse bad arguments before any launch (no device needed to see that)
    import ctypes
    three = (ctypes.c_float * 3)(1, 1, 1)
    assert hip_lib.ngp_mesh_count(None, 4, 4, 4, 0.0, 1, None, None, None) == -1
    assert hip_lib.ngp_mesh_emit(None, 4, 4, 4, 0.0, 1, three, three, None, None, None, None, None) == -1
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mesh_count(torch.zeros(4, 4, 4), 0.0, 1)
    with pytest.raises(ValueError, match="N >= 2"):
        ops.mesh_count(torch.zeros(1, 4, 4), 0.0, 1)
    with pytest.raises(ValueError, match="sign"):
        ops.mesh_count(torch.zeros(4, 4, 4), 0.0, 0)
    with pytest.raises(ValueError, match="sign"):
        ops.mesh_emit(torch.zeros(4, 4, 4), 0.0, 2, (0, 0, 0), (1, 1, 1), torch.zeros(8, dtype=torch.uint8), 0, 0)
    with pytest.raises(ValueError, match="positive"):
        ops.mesh_emit(torch.zeros(4, 4, 4), 0.0, 1, (0, 0, 0), (1, 0, 1), torch.zeros(8, dtype=torch.uint8), 0, 0)
