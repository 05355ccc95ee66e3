"""The numpy reference of the ray-casting contract (tests/mesh_raycast_reference.py) against analytic truth, and the conditions its
named sets must meet, without a GPU."""
import os
import re

import numpy as np
import pytest

import mesh_raycast_reference as R
import mesh_sdf_reference as M
from conftest import ROOT


def test_cube_is_the_slab_intersection():
    """Twelve faces with exactly representable corners: the float64 brute force IS the slab intersection of the box, to the rounding of
    float64 (1e-12), from outside (the near wall, or nothing) and from inside (the far wall)."""
    v, f = M.cube()
    rng = np.random.default_rng(1)
    o, d = (np.concatenate(x) for x in zip(R.rays_outside_in(v, 2048, rng), R.rays_inside_out(v, 2048, rng, pad=0.5)))
    ref = R.brute_force(o, d, v, f, np.float64)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore"):
        t0, t1 = (0.25 - o64) / d64, (0.75 - o64) / d64
    near, far = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    hit = (near <= far) & (far >= 0)
    t = np.where(near > 0, near, far)
    assert hit.sum() > 2000 and (~hit).sum() > 100
    assert np.array_equal(ref["face"] >= 0, hit)
    assert np.abs(ref["t"][hit] - t[hit]).max() <= 1e-12
    inside = ((o64 > 0.25) & (o64 < 0.75)).all(1)
    assert inside.sum() > 100 and hit[inside].all()
    assert (ref["side"][hit] == np.where(inside[hit], -1, 1)).all()                                    # from outside the front, from inside the back
    x = o64[hit] + ref["t"][hit, None] * d64[hit]
    tri = v[f[ref["face"][hit]]].astype(np.float64)
    b = ref["bary"][hit]
    assert np.abs(tri[:, 0] + b[:, :1] * (tri[:, 1] - tri[:, 0]) + b[:, 1:] * (tri[:, 2] - tri[:, 0]) - x).max() <= 1e-12


def test_icosphere_is_the_sphere_within_the_sagitta():
    """1280 faces inscribed in the sphere of radius r: every hit point lies between r - s and r, s = r - (the least distance of a face
    from the centre); a ray whose line passes the centre nearer than r - s hits, one that passes farther than r misses."""
    v, f = M.icosphere()
    c, r = np.full(3, 0.5), 0.35
    tri = v[f].astype(np.float64)
    r_in = float(np.sqrt(M.closest_on_triangle(c[None], tri[:, 0], tri[:, 1], tri[:, 2], np.float64)["d2"].min()))
    r_out = float(np.linalg.norm(v.astype(np.float64) - c, axis=1).max())
    assert 0.0 < r - r_in < 0.005 and abs(r_out - r) < 1e-6
    rng = np.random.default_rng(2)
    o, d = R.rays_outside_in(v, 4096, rng)
    ref = R.brute_force(o, d, v, f, np.float64)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    impact = np.linalg.norm(np.cross(c - o64, d64), axis=1) / np.linalg.norm(d64, axis=1)
    hit = ref["face"] >= 0
    assert hit[impact < r_in - 1e-9].all() and not hit[impact > r_out + 1e-9].any() and (impact < r_in).sum() > 1000
    radius = np.linalg.norm(o64[hit] + ref["t"][hit, None] * d64[hit] - c, axis=1)
    assert radius.min() >= r_in - 1e-9 and radius.max() <= r_out + 1e-9
    b = np.sum((o64 - c) * d64, 1) / np.sum(d64 * d64, 1)                                     # the sphere itself: t = -b - sqrt(b^2 - c)
    with np.errstate(invalid="ignore"):
        t_sphere = -b - np.sqrt(b * b - (np.sum((o64 - c)**2, 1) - r_out**2) / np.sum(d64 * d64, 1))
    inner = impact < 0.9 * r_in
    assert ((ref["t"] >= t_sphere - 1e-9) & (ref["t"] <= t_sphere + 3 * (r - r_in) / np.linalg.norm(d64, axis=1)))[inner].all()


def moller_trumbore_misses(o, d, vertices, faces, chunk=512):
    """Plain Moller-Trumbore in float32, every operation rounded on its own, against all faces -> bool [n]: the ray hits no face.  The
    obvious implementation, kept here only: its barycentrics are computed per face from that face's own edges, so two faces disagree
    about a point on their common edge."""
    T = np.float32
    tri = np.asarray(vertices, T)[np.asarray(faces, np.int64)]
    a, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    miss = np.ones(len(o), bool)
    for s in range(0, len(o), chunk):
        oo, dd = np.asarray(o[s:s + chunk], T)[:, None], np.asarray(d[s:s + chunk], T)[:, None]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            p = M.cross(np.broadcast_to(dd, (len(dd),) + e2.shape[1:]), np.broadcast_to(e2, (len(dd),) + e2.shape[1:]))
            det = M.dot(e1, p)
            inv = T(1.0) / det
            tv = oo - a
            u = M.dot(tv, p) * inv
            q = M.cross(tv, np.broadcast_to(e1, tv.shape))
            w = M.dot(dd, q) * inv
            t = M.dot(e2, q) * inv
            ok = (det != 0) & (u >= 0) & (u <= 1) & (w >= 0) & (u + w <= 1) & (t >= 0) & (t < np.inf)
        miss[s:s + chunk] = ~ok.any(1)
    return miss


@pytest.mark.parametrize("origin", sorted(R.INSIDE_ORIGINS))
def test_no_ray_slips_between_faces_where_moller_trumbore_lets_some_through(origin):
    """From inside the 1280-face icosphere, aimed exactly at every vertex, every edge midpoint and a random point of every edge: 4482 rays,
    all of which hit something.  The float32 restatement of the kernel's test misses none; plain Moller-Trumbore in the same arithmetic
    misses some (the issue's prototype counted 206 from the centre and 273 off centre) -- the set discriminates."""
    v, f, o, d = R.watertight_set(R.INSIDE_ORIGINS[origin])
    assert len(o) == 642 + 2 * 1920
    r32 = R.brute_force(o, d, v, f, np.float32)
    mt = int(moller_trumbore_misses(o, d, v, f).sum())
    print("%s: watertight test misses %d of %d, Moller-Trumbore %d" % (origin, int((r32["face"] < 0).sum()), len(o), mt))
    assert (r32["face"] >= 0).all()
    assert mt > 0
    assert (R.brute_force(o, d, v, f, np.float64)["face"] >= 0).mean() > 0.5              # float64 without the tie rule loses some too


@pytest.mark.parametrize("distance", [2.0, 35.0, 3500.0])
def test_no_ray_slips_between_front_faces_from_far_away(distance):
    v, f, o, d = R.watertight_set(0.5 + distance * R.OUTSIDE_DIRECTION, front_only=True)
    assert len(o) > 1000
    r32 = R.brute_force(o, d, v, f, np.float32)
    assert (r32["face"] >= 0).all()
    c = R.Case("front@%g" % distance, v, f, o, d)
    assert np.abs(r32["t"].astype(np.float64) - 1.0).max() <= 4 * c.ref()["e32_t"]


@pytest.mark.parametrize("mesh", ["cube", "icosphere", "torus"])
def test_a_segment_between_two_outside_points_crosses_a_closed_mesh_an_even_number_of_times(mesh):
    v, f = M._mesh(mesh)
    rng = np.random.default_rng(7)
    lo, hi, ext, c = R._box(v)
    a = c + 1.5 * ext * R._unit(rng, 384)
    b = c - (a - c) + 0.8 * ext * R._unit(rng, 384)                          # roughly opposite: most segments pass through the box
    count = R.brute_force(a.astype(np.float32), (b - a).astype(np.float32), v, f, np.float64, 0.0, 1.0)["count"]
    assert (count % 2 == 0).all() and (count > 0).sum() > 50


@pytest.mark.parametrize("name", R.CASES)
def test_named_sets_are_decided(name):
    """At most 2 % of a set may be left undecided, by the float64 reference alone; and the float32 restatement passes its own judge."""
    c = R.case(name)
    assert c.undecided_fraction() <= R.MAX_UNDECIDED, (name, c.undecided_fraction())
    r32 = c.ref()["r32"]
    R.judge(c, r32["t"], r32["face"], r32["bary"], r32["side"])


def test_zero_area_and_nan_never_win():
    a, b, c = (np.array([x], np.float32) for x in ([0, 0, 1], [0.5, 0, 1], [1, 0, 1]))
    r = R.setup(np.array([[0.25, 0, 0]], np.float32), np.array([[0, 0, 1]], np.float32), np.float32)
    assert np.isnan(R.ray_face(r, a, b, c, np.float32)["t"]).all()
    v, f = M.cube()
    bad = np.array([[0, 0, 0], [np.nan, 1, 0], [np.inf, 1, 0], [1, 0, 0], [1, 0, 0]], np.float32)
    o = np.array([[0.5, 0.5, 0.5]] * 3 + [[np.nan, 0.5, 0.5], [np.inf, 0.5, 0.5]], np.float32)
    for T in (np.float32, np.float64):
        out = R.brute_force(o, bad, v, f, T)
        assert (out["face"] == -1).all() and np.isposinf(out["t"]).all() and (out["side"] == 0).all() and (out["bary"] == 0).all()


def test_header_declares_the_entry():
    text = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    assert re.search(r"#define\s+NGP_ABI_VERSION\s+3\s", text)
    proto = re.search(r"int\s+ngp_mesh_raycast\s*\(([^;]*)\)\s*;", text)
    assert proto
    args = [re.sub(r"\s+", " ", a).strip() for a in re.sub(r"/\*.*?\*/", "", proto.group(1)).split(",")]
    assert args == ["const float* rays_o", "const float* rays_d", "int n", "const float* vertices", "const int32_t* faces",
                    "const int32_t* order", "const float* boxes", "int n_faces", "int leaf_size", "float t_min", "float t_max", "int flags",
                    "float* t", "int32_t* face", "float* bary", "int32_t* side", "void* stream"]
    for name, value in (("NGP_RAYCAST_ANY_HIT", 1), ("NGP_RAYCAST_CULL_BACK", 2), ("NGP_RAYCAST_CULL_FRONT", 4)):
        assert re.search(r"#define\s+%s\s+%d\s" % (name, value), text)
    from ngp_hip import lib
    assert "ngp_mesh_raycast" in lib.SIGNATURES and len(lib.SIGNATURES["ngp_mesh_raycast"]) == 17 and "mesh_raycast.hip" in lib.SOURCES
