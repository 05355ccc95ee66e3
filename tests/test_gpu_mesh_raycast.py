"""Ray casting against a triangle mesh on the GPU (csrc/mesh_raycast.hip through ngp_hip.MeshSDF.raycast) against the numpy brute force of
the contract (tests/mesh_raycast_reference.py: float64 is the truth, the float32 restatement gives E32).

THE STANDARD ASSERTION (mesh_raycast_reference.judge; every test asserts it unless it says otherwise): on DECIDED rays hit or miss is
exact, |t - t64| <= 4 x E32_t, the returned face is a legitimate first face (its float64 t within that bound of the minimum, not clearly
missed), bary within 4 x E32_b of float64 on the returned face, side exact where that face is clearly hit; on undecided rays every output
is finite or the miss encoding and a reported t belongs to a face that is not clearly missed."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import mesh_raycast_reference as R
import mesh_sdf_reference as M
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
CULL = {0: None, R.CULL_BACK: "back", R.CULL_FRONT: "front"}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mesh(v, f, **kw):
    from ngp_hip import MeshSDF
    return MeshSDF(torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(np.ascontiguousarray(f)), signed=False, **kw)


def _outputs(h):
    return tuple(x.cpu().numpy() for x in (h.t, h.face, h.bary, h.side))


def _cast(m, case, **kw):
    h = m.raycast(_t(case.o), _t(case.d), t_min=case.t_min, t_max=case.t_max, cull=CULL[case.cull], **kw)
    n = len(case.o)
    assert h.t.dtype == torch.float32 and h.t.shape == (n,) and not h.t.requires_grad
    if h.face is not None:
        assert h.face.dtype == h.side.dtype == torch.int32 and h.bary.shape == (n, 2) and torch.equal(h.hit, h.face >= 0)
    return h


def _check(case, mesh=None, any_hit=False, **kw):
    m = mesh if mesh is not None else _mesh(case.vertices, case.faces, **kw)
    out = _outputs(_cast(m, case, any_hit=any_hit))
    R.judge(case, *out, any_face=any_hit)
    return m, out


@pytest.mark.parametrize("name", R.CASES)
def test_named_cases(hip_lib, name):
    """One triangle, the cube, the needle tetrahedron, the icosphere, the open quad and the extracted torus; rays from a shell into the
    box, from inside outwards, grazing a face, from 1000 diameters away, and with directions of length 1e-3 and 1e3."""
    c = R.case(name)
    assert c.undecided_fraction() <= R.MAX_UNDECIDED
    _check(c)


_SOUPS = {}


def _rays(v, f, rng, n=256):
    o, d = zip(R.rays_outside_in(v, n, rng), R.rays_inside_out(v, n, rng))
    return np.concatenate(o), np.concatenate(d)


def _soup_case(n_faces, **kw):
    key = (n_faces, tuple(sorted(kw.items())))
    if key not in _SOUPS:
        v, f = M.soup(n_faces, seed=n_faces, **kw)
        _SOUPS[key] = R.Case("soup%d%s" % (n_faces, "/same centroid" if kw else ""), v, f, *_rays(v, f, np.random.default_rng(n_faces + 1)))
    return _SOUPS[key]


@pytest.mark.parametrize("leaf_size", [1, 4, 8])
@pytest.mark.parametrize("n_faces", [1, 2, 3, 5, 13, 4097])
def test_face_counts_and_leaf_sizes(hip_lib, n_faces, leaf_size):
    """Trees of one node up to 4097 leaves of one face (depth 13, 4095 of the 8192 leaves padding), triangle soups."""
    _check(_soup_case(n_faces), leaf_size=leaf_size)


def test_mesh_far_from_the_origin(hip_lib):
    """The icosphere moved to lo = 100: coordinates lose 8 bits, the bound follows through E32."""
    v, f = M.icosphere()
    v = (v.astype(np.float64) + 100.0).astype(np.float32)
    c = R.Case("icosphere at 100", v, f, *_rays(v, f, np.random.default_rng(100)))
    assert c.undecided_fraction() <= R.MAX_UNDECIDED
    _check(c)
    print("icosphere at 100: E32 t %.3g, bary %.3g" % (c.ref()["e32_t"], c.ref()["e32_b"]))


def test_one_morton_code_and_duplicated_faces(hip_lib):
    """200 faces around one centroid (the sort cannot separate them), and a cube one of whose faces is there 65 times: any of the
    duplicates is a legitimate first face."""
    _check(_soup_case(200, same_centroid=True, size=0.3))
    v, f = M.cube()
    f = np.concatenate([np.repeat(f[:1], 64, axis=0), f])
    c = R.Case("cube + 64 copies of a face", v, f, *_rays(v, f, np.random.default_rng(64)))
    for leaf_size in (4, 1):
        _, (t, face, _, _) = _check(c, leaf_size=leaf_size)
        assert ((face <= 64) & (face >= 0)).sum() > 20


def test_zero_area_face_is_never_returned(hip_lib):
    """Three collinear points with distinct indices laid 0.05 above the top of the icosphere, first in the face list; the rays come
    straight down through that segment (half of them exactly through it).  The face has det = 0 and never wins: the sphere below it is
    returned, and no output is NaN."""
    v, f = M.icosphere()
    v = np.concatenate([v, [[0.4, 0.5, 0.9], [0.5, 0.5, 0.9], [0.6, 0.5, 0.9]]]).astype(np.float32)
    f = np.concatenate([[[len(v) - 3, len(v) - 2, len(v) - 1]], f]).astype(np.int32)
    rng = np.random.default_rng(9)
    o = np.stack([rng.uniform(0.4, 0.6, 512), np.where(np.arange(512) % 2 == 0, 0.5, 0.5 + 1e-3 * rng.standard_normal(512)), np.full(512, 1.5)], 1)
    c = R.Case("icosphere + a zero-area face", v, f, o, np.tile([0.0, 0.0, -1.0], (512, 1)))
    for leaf_size in (1, 4):
        m, (t, face, _, side) = _check(c, leaf_size=leaf_size)
        assert m.n_faces == len(f) and (face > 0).all() and (side == 1).all()
        assert t.min() > 0.62                                            # the segment would have been met at t = 0.6


@pytest.mark.parametrize("leaf_size", [1, 8])
@pytest.mark.parametrize("origin", sorted(R.INSIDE_ORIGINS))
def test_no_ray_slips_between_faces_from_inside(hip_lib, origin, leaf_size):
    """4482 rays from inside the icosphere aimed exactly at every vertex, every edge midpoint and a random point of every edge (plain
    Moller-Trumbore misses hundreds: tests/test_mesh_raycast_reference.py): every ray hits.  Neighbouring faces sit in different
    subtrees, so this holds the face test and the box test together."""
    v, f, o, d = R.watertight_set(R.INSIDE_ORIGINS[origin])
    h = _mesh(v, f, leaf_size=leaf_size).raycast(_t(o), _t(d))
    print("%s, leaf %d: %d of %d rays miss" % (origin, leaf_size, int((~h.hit).sum()), len(o)))
    assert bool(h.hit.all()) and bool((h.side == -1).all())


@pytest.mark.parametrize("distance", [2.0, 35.0, 3500.0])
def test_no_ray_slips_between_front_faces_from_far_away(hip_lib, distance):
    """The same targets where they face the origin (n . (o - x) > 0.3 |o - x|), d = x - o: every ray hits, at t = 1 within B_t."""
    v, f, o, d = R.watertight_set(0.5 + distance * R.OUTSIDE_DIRECTION, front_only=True)
    c = R.Case("front@%g" % distance, v, f, o, d)
    for leaf_size in (1, 8):
        t = _mesh(v, f, leaf_size=leaf_size).raycast(_t(o), _t(d), details=False).t.cpu().numpy().astype(np.float64)
        print("%s, leaf %d: %d of %d miss, |t - 1| <= %.3g (bound %.3g)" % (c.name, leaf_size, int(np.isinf(t).sum()), len(t), np.abs(t - 1).max(), 4 * c.ref()["e32_t"]))
        assert np.isfinite(t).all() and np.abs(t - 1.0).max() <= 4 * c.ref()["e32_t"]


@pytest.mark.parametrize("resolution", [32, 64])
def test_closed_loop_with_the_extractor(hip_lib, resolution):
    """extract_mesh of the sphere |x - c| - 0.3 -> MeshSDF -> rays, bounds from geometry alone: with r_in the least distance of a face from
    the centre (float64) and r_out the largest vertex radius, every ray from outside whose line passes the centre nearer than r_in hits,
    none that passes farther than r_out does, and every hit point lies between the two radii up to s = four float32 ulps of the scene's
    scale.  Culling the back faces changes nothing for these rays; culling the front faces returns the far wall."""
    from ngp_hip.mesh import extract_mesh
    c = np.array([0.52, 0.49, 0.5])
    centre = torch.tensor(c, dtype=torch.float32, device=DEV)
    mesh = extract_mesh(lambda x: torch.linalg.norm(x - centre, dim=1) - 0.3, resolution, 0.0, bounds=((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                        sign=-1, normals=None, device=torch.device(DEV))
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    c = centre.cpu().numpy().astype(np.float64)
    tri = v[f].astype(np.float64)
    r_in = float(np.sqrt(np.nanmin(M.closest_on_triangle(c[None], tri[:, 0], tri[:, 1], tri[:, 2], np.float64)["d2"])))
    r_out = float(np.linalg.norm(v.astype(np.float64) - c, axis=1).max())
    assert 0.29 < r_in < r_out < 0.31
    rng = np.random.default_rng(resolution)
    o = (c + 1.2 * R._unit(rng, 4096)).astype(np.float32)
    d = ((c + 0.45 * rng.uniform(-1, 1, (4096, 3))) - o).astype(np.float32)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    impact = np.linalg.norm(np.cross(c - o64, d64), axis=1) / np.linalg.norm(d64, axis=1)
    s = 4 * float(M.ulp32(max(np.abs(o).max(), np.abs(v).max())))
    from ngp_hip import MeshSDF
    m = MeshSDF.from_mesh(mesh, signed=False)
    plain, back, front = (m.raycast(_t(o), _t(d), cull=cull) for cull in (None, "back", "front"))
    t, hit = plain.t.cpu().numpy().astype(np.float64), plain.hit.cpu().numpy()
    print("%d^3: %d faces, r_in %.6f r_out %.6f, %d hit, %d inside r_in, %d outside r_out" % (resolution, len(f), r_in, r_out, hit.sum(), (impact < r_in).sum(), (impact > r_out).sum()))
    assert (impact < r_in).sum() > 500 and (impact > r_out).sum() > 500
    assert hit[impact < r_in].all() and not hit[impact > r_out].any()
    radius = np.linalg.norm(o64[hit] + t[hit, None] * d64[hit] - c, axis=1)
    assert radius.min() >= r_in - s and radius.max() <= r_out + s, (radius.min() - r_in, radius.max() - r_out, s)
    assert (plain.side[plain.hit] == 1).all()
    for p, q in zip(plain, back):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    tf, hf = front.t.cpu().numpy().astype(np.float64), front.hit.cpu().numpy()
    assert hf[impact < r_in].all() and not hf[impact > r_out].any() and (front.side[front.hit] == -1).all()
    both = hit & hf
    assert (tf[both] > t[both]).all()
    radius = np.linalg.norm(o64[hf] + tf[hf, None] * d64[hf] - c, axis=1)
    assert radius.min() >= r_in - s and radius.max() <= r_out + s


def test_any_hit_agrees_with_first_hit(hip_lib):
    for name in ("icosphere/outside_in", "torus/inside_out", "cube/grazing"):
        c = R.case(name)
        m, (t, face, _, _) = _check(c)
        _, (ta, fa, _, _) = _check(c, mesh=m, any_hit=True)
        dec = c.ref()["decided"]
        assert np.array_equal((face >= 0)[dec], (fa >= 0)[dec]) and (ta[fa >= 0] >= t[fa >= 0]).all()


def test_window_selects_the_second_wall_of_the_cube(hip_lib):
    """d = target - origin with the target inside the cube: the near wall is met before t = 1, the far wall after."""
    base = R.case("cube/outside_in")
    first = R.Case("cube, t <= 1", base.vertices, base.faces, base.o, base.d, 0.0, 1.0)
    second = R.Case("cube, t >= 1", base.vertices, base.faces, base.o, base.d, 1.0, np.inf)
    nothing = R.Case("cube, 1 <= t <= 1.0001", base.vertices, base.faces, base.o, base.d, 1.0, 1.0001)
    m, (t1, _, _, s1) = _check(first)
    _, (t2, _, _, s2) = _check(second, mesh=m)
    _, (t3, f3, _, _) = _check(nothing, mesh=m)
    assert (s1 == 1).all() and (s2 == -1).all() and (t1 < 1).all() and (t2 > 1).all() and (f3 == -1).sum() > 500


def test_visible_agrees_with_the_reference(hip_lib):
    v, f = M.icosphere()
    rng = np.random.default_rng(12)
    a = (0.5 + rng.uniform(0.05, 0.6, (2048, 1)) * R._unit(rng, 2048)).astype(np.float32)
    b = (0.5 + rng.uniform(0.05, 0.6, (2048, 1)) * R._unit(rng, 2048)).astype(np.float32)
    eps = 1e-4
    c = R.Case("segments at the icosphere", v, f, a, b - a, np.float32(eps), np.float32(1.0 - eps))
    assert c.undecided_fraction() <= R.MAX_UNDECIDED
    vis = _mesh(v, f).visible(_t(a), _t(b), eps=eps).cpu().numpy()
    dec = c.ref()["decided"]
    blocked = c.ref()["r64"]["face"] >= 0
    print("visible: %d of %d segments blocked, %d undecided" % (blocked.sum(), len(a), (~dec).sum()))
    assert vis.dtype == bool and np.array_equal(vis[dec], ~blocked[dec]) and 200 < blocked.sum() < 1900


@pytest.mark.parametrize("n", [0, 1, 65, 4096])
def test_batch_sizes_permutations_and_null_outputs(hip_lib, n):
    """A result depends on its ray and the mesh alone: the same bits under a permutation of the batch, between two calls, and with face /
    bary / side not asked for."""
    c = R.case("torus/outside_in")
    m = _mesh(c.vertices, c.faces)
    rng = np.random.default_rng(n)
    o, d = (_t(np.concatenate(x)) for x in zip(R.rays_outside_in(c.vertices, n - n // 2, rng), R.rays_inside_out(c.vertices, n // 2, rng)))
    a, b = m.raycast(o, d), m.raycast(o, d)
    assert a.t.shape == (n,) and a.face.shape == (n,) and a.bary.shape == (n, 2) and a.side.shape == (n,)
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    perm = torch.from_numpy(rng.permutation(n)).to(DEV)
    s = m.raycast(o[perm].contiguous(), d[perm].contiguous())
    for p, q in zip(a, s):
        assert torch.equal(p[perm].view(torch.int32), q.view(torch.int32))
    for any_hit in (False, True):
        full, only = m.raycast(o, d, any_hit=any_hit), m.raycast(o, d, any_hit=any_hit, details=False)
        assert only.face is None and only.bary is None and only.side is None
        assert torch.equal(only.t.view(torch.int32), full.t.view(torch.int32))
    if n > 1:
        assert 0 < int(a.hit.sum()) < n
        x = a.points(o, d)
        assert torch.equal(x[~a.hit], o[~a.hit]) and torch.isfinite(x).all()


def test_degenerate_rays_in_one_batch_with_good_ones(hip_lib):
    """Zero direction, NaN and +-inf components in origin or direction, denormal directions, and a window with t_min > t_max: all misses,
    written without a fault, and the good rays of the batch keep their bits.  (The stand-alone host build of the same kernel source ran
    these rays clean under the address and undefined-behaviour sanitizers first: DESIGN.md.)"""
    c = R.case("icosphere/inside_out")
    m = _mesh(c.vertices, c.faces)
    inf, nan = np.inf, np.nan
    bad = np.array([[.5, .5, .5, 0, 0, 0], [.5, .5, .5, -0.0, -0.0, -0.0], [.5, .5, .5, nan, 1, 0], [.5, .5, .5, inf, 1, 0], [.5, .5, .5, 1, -inf, 0],
                    [nan, .5, .5, 1, 0, 0], [inf, .5, .5, -1, 0, 0], [.5, -inf, .5, 0, 1, 0], [.5, .5, .5, nan, nan, nan], [nan, nan, nan, nan, nan, nan],
                    [3e38, 3e38, 3e38, -1, -1, -1], [.5, .5, nan, 0, 0, 1]], np.float32)
    soft = np.array([[.5, .5, .5, 1e-42, 0, 0], [.5, .5, .5, 1e-42, 1e-44, 1], [1e-40, 1e-41, -2, 0, 0, 1], [.5, .5, .5, 3e38, 1, 1]], np.float32)
    k = len(bad) + len(soft)
    o = np.concatenate([bad[:, :3], soft[:, :3], c.o])
    d = np.concatenate([bad[:, 3:], soft[:, 3:], c.d])
    pos = np.random.default_rng(3).permutation(len(o))
    mixed = m.raycast(_t(o[pos]), _t(d[pos]))
    alone = m.raycast(_t(c.o), _t(c.d))
    inv = np.argsort(pos)
    for p, q in zip(mixed, alone):
        p = p[torch.from_numpy(inv).to(DEV)]
        assert torch.equal(p[k:].view(torch.int32), q.view(torch.int32))
    t, face, bary, side = (x[torch.from_numpy(inv).to(DEV)].cpu().numpy() for x in mixed)
    n_bad = len(bad)
    assert np.isposinf(t[:n_bad]).all() and (face[:n_bad] == -1).all() and (bary[:n_bad] == 0).all() and (side[:n_bad] == 0).all()
    assert not np.isnan(t[:k]).any() and np.isfinite(bary[:k]).all() and (np.isfinite(t[:k]) == (face[:k] >= 0)).all()
    R.judge(c, t[k:], face[k:], bary[k:], side[k:])
    for window in ((1.0, 0.5), (nan, inf), (0.0, nan), (inf, inf)):
        h = m.raycast(_t(c.o), _t(c.d), t_min=window[0], t_max=window[1])
        assert bool(torch.isposinf(h.t).all()) and bool((h.face == -1).all()) and bool((h.side == 0).all()) and bool((h.bary == 0).all())
    any_bad = m.raycast(_t(bad[:, :3]), _t(bad[:, 3:]), any_hit=True)
    assert bool(torch.isposinf(any_bad.t).all())


def test_entry_refuses_bad_arguments(hip_lib):
    """-1, nothing launched or written: null pointers, n < 0, n_faces < 1, a leaf_size outside 1..8, unknown flag bits; 0 and nothing
    written for n = 0."""
    lib = hip_lib
    v, f = M.cube()
    tv, tf, order = _t(v), _t(f), torch.arange(12, device=DEV, dtype=torch.int32)
    from ngp_hip import ops
    boxes = ops.mesh_bvh_build(tv, tf, order, 4)
    c = R.case("cube/outside_in")
    o, d = _t(c.o[:8]), _t(c.d[:8])
    t, face = torch.full((8,), 7.0, device=DEV), torch.full((8,), 7, device=DEV, dtype=torch.int32)
    bary, side = torch.full((8, 2), 7.0, device=DEV), torch.full((8,), 7, device=DEV, dtype=torch.int32)
    p = lambda x: x.data_ptr()
    q = lambda **kw: lib.ngp_mesh_raycast(*[kw.get(k, dflt) for k, dflt in (
        ("rays_o", p(o)), ("rays_d", p(d)), ("n", 8), ("vertices", p(tv)), ("faces", p(tf)), ("order", p(order)), ("boxes", p(boxes)),
        ("n_faces", 12), ("leaf_size", 4), ("t_min", 0.0), ("t_max", float("inf")), ("flags", 0), ("t", p(t)), ("face", p(face)),
        ("bary", p(bary)), ("side", p(side)), ("stream", 0))])
    for bad in (dict(rays_o=0), dict(rays_d=0), dict(vertices=0), dict(faces=0), dict(order=0), dict(boxes=0), dict(t=0), dict(n=-1),
                dict(n_faces=0), dict(n_faces=-3), dict(leaf_size=0), dict(leaf_size=9), dict(flags=8), dict(flags=-1), dict(flags=1 << 20)):
        assert q(**bad) == -1, bad
    assert q(n=0) == 0 and q(n=0, rays_o=0, rays_d=0, t=0) == 0
    torch.cuda.synchronize()
    assert (t == 7.0).all() and (face == 7).all() and (bary == 7.0).all() and (side == 7).all()
    assert q() == 0 and q(face=0, bary=0, side=0) == 0 and q(flags=7) == 0
    torch.cuda.synchronize()
    assert bool(torch.isposinf(t).all())                                  # both cull flags: nothing is left to hit
    assert q(flags=3) == 0
    torch.cuda.synchronize()
    assert (t != 7.0).all() and bool(torch.isfinite(t).all()) and (side == 1).all()


def test_ops_and_meshsdf_validate_before_any_launch(hip_lib, monkeypatch):
    from ngp_hip import ops
    c = R.case("cube/outside_in")
    m = _mesh(c.vertices, c.faces)
    o, d = _t(c.o), _t(c.d)

    class Boom:
        def __getattr__(self, name):
            if name == "ngp_mesh_bvh_bytes":
                return hip_lib.ngp_mesh_bvh_bytes
            raise AssertionError("a launch for arguments that must be refused")
    monkeypatch.setattr(ops, "_lib", lambda: Boom())
    args = (m.vertices, m.faces, m.order, m.boxes, m.leaf_size)
    with pytest.raises(ValueError):
        ops.mesh_raycast(o, d[:5], *args)
    with pytest.raises(ValueError):
        ops.mesh_raycast(o.view(-1), d.view(-1), *args)
    with pytest.raises(TypeError):
        ops.mesh_raycast(o.double(), d.double(), *args)
    with pytest.raises(RuntimeError):
        ops.mesh_raycast(o.cpu(), d.cpu(), *args)
    with pytest.raises(ValueError):
        ops.mesh_raycast(o.t().contiguous().t(), d, *args)
    with pytest.raises(ValueError):
        ops.mesh_raycast(o, d, m.vertices, m.faces, m.order, m.boxes[:-1], m.leaf_size)
    with pytest.raises(ValueError):
        ops.mesh_raycast(o, d, m.vertices, m.faces, m.order, m.boxes, 9)
    with pytest.raises(ValueError, match="cull"):
        ops.mesh_raycast(o, d, *args, cull="both")
    with pytest.raises(ValueError, match="cull"):
        m.raycast(o, d, cull="outside")
    with pytest.raises(AssertionError):
        m.raycast(o, d)                                                   # the guard itself: a good call does reach the library
    monkeypatch.undo()
    R.judge(c, *_outputs(m.raycast(o, d)))
    signed = __import__("ngp_hip").MeshSDF(torch.from_numpy(c.vertices), torch.from_numpy(c.faces))      # the signed tree casts the same rays
    for p, q in zip(signed.raycast(o, d), m.raycast(o, d)):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))


def _look_at(position, target=(0.5, 0.5, 0.5)):
    pos = torch.tensor(position, dtype=torch.float32)
    fwd = torch.nn.functional.normalize(torch.tensor(target) - pos, dim=0)
    right = torch.nn.functional.normalize(torch.cross(fwd, torch.tensor([0.0, 0.0, 1.0]), dim=0), dim=0)
    down = torch.cross(fwd, right, dim=0)
    return torch.cat([torch.stack([right, down, fwd], -1), pos[:, None]], -1)


def test_render_mesh_of_the_cube(hip_lib):
    """24 x 32 pixels: depth equals the float64 reference on decided pixels (the rays are the package's own, read back), the normal is
    one of the six axis directions and faces the camera, the mask is isfinite(depth)."""
    from ngp_hip import render_mesh
    from ngp_hip.mesh import Mesh
    from ngp_hip.rays import get_ray_directions, get_rays
    v, f = M.cube()
    w, h = 32, 24
    K = torch.tensor([[60.0, 0.0, 16.0], [0.0, 60.0, 12.0], [0.0, 0.0, 1.0]])
    c2w = _look_at((1.7, 1.3, 1.9))
    out = render_mesh(Mesh(torch.from_numpy(v), torch.from_numpy(f), None), K, c2w, (w, h))
    assert out["depth"].shape == (h, w) and out["normal"].shape == (h, w, 3) and out["mask"].shape == (h, w) and out["face"].shape == (h, w)
    assert out["mask"].dtype == torch.bool and out["face"].dtype == torch.int32
    assert torch.equal(out["mask"], torch.isfinite(out["depth"])) and torch.equal(out["mask"], out["face"] >= 0)
    rays_o, rays_d = get_rays(get_ray_directions(h, w, K, device=DEV), c2w.to(DEV))
    rays_d = rays_d / torch.linalg.norm(rays_d, dim=1, keepdim=True)
    c = R.Case("cube from a camera", v, f, rays_o.cpu().numpy(), rays_d.cpu().numpy())
    ref, dec = c.ref()["r64"], c.ref()["decided"]
    depth, mask = out["depth"].view(-1).cpu().numpy().astype(np.float64), out["mask"].view(-1).cpu().numpy()
    assert 100 < mask.sum() < w * h - 100 and (~dec).mean() <= R.MAX_UNDECIDED
    assert np.array_equal(mask[dec], (ref["face"] >= 0)[dec])
    on = dec & mask
    err = np.abs(depth[on] - ref["t"][on]).max()
    print("render_mesh: %d of %d pixels covered, %d undecided, depth err %.3g (bound %.3g)" % (mask.sum(), w * h, (~dec).sum(), err, 4 * c.ref()["e32_t"]))
    assert err <= 4 * c.ref()["e32_t"]
    nrm = out["normal"].view(-1, 3).cpu().numpy()
    assert (nrm[~mask] == 0).all()
    assert ((np.abs(nrm[mask]) == 1).sum(1) == 1).all() and ((nrm[mask] == 0).sum(1) == 2).all()
    assert ((nrm[mask] * rays_d.cpu().numpy()[mask]).sum(1) < 0).all()
    assert {tuple(x) for x in nrm[mask].astype(int).tolist()} == {(1, 0, 0), (0, 1, 0), (0, 0, 1)}                # the three faces this camera sees
    smooth = render_mesh(_mesh(v, f), K, c2w, (w, h), smooth=torch.nn.functional.normalize(torch.from_numpy(v) - 0.5, dim=1).to(DEV))
    assert torch.equal(smooth["depth"].view(torch.int32), out["depth"].view(torch.int32))
    length = torch.linalg.norm(smooth["normal"], dim=-1)
    assert torch.allclose(length[out["mask"]], torch.ones_like(length[out["mask"]]), atol=1e-5) and (length[~out["mask"]] == 0).all()
    culled = render_mesh(_mesh(v, f), K, c2w, (w, h), cull="front")
    assert bool((culled["depth"][out["mask"]] > out["depth"][out["mask"]]).all())


def test_render_example_against_a_fitted_field(hip_lib, tmp_path, capsys):
    """examples/render_mesh.py --against-field at a tiny setting: the 16^3-level torus, 300 steps with small tables, two 32 x 32 views.  It
    runs and writes its images; on the pixels that the mesh and both fields hit, the trained field's mean |t_trace - t_mesh| is smaller
    than the untrained field's (a sphere of radius 0.25).  No ratio is fixed: training must improve, and the figures are printed."""
    spec = importlib.util.spec_from_file_location("render_mesh_example", os.path.join(ROOT, "examples", "render_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = tmp_path / "views"
    info = ex.main(["--against-field", "300", "--n", "4096", "--log2_T", "14", "--levels", "8", "--max_res", "128", "--target_resolution", "16",
                    "--views", "2", "--wh", "32", "--out", str(out), "--json", str(tmp_path / "fit.json")])
    captured = capsys.readouterr().out
    u, t = info["untrained"], info["trained"]
    print("render_mesh --against-field: mask differs %.4f -> %.4f, mean |t_trace - t_mesh| %.5f -> %.5f (common pixels: %.5f -> %.5f, %d), max %.4f -> %.4f"
          % (u["mask_differs"], t["mask_differs"], u["t_mean"], t["t_mean"], u["t_mean_common"], t["t_mean_common"], t["pixels_common"], u["t_max"], t["t_max"]))
    assert len(info["views"]) == 2 and 0.02 < info["covered"] < 0.9 and t["pixels_common"] > 20
    assert math.isfinite(t["t_mean_common"]) and t["t_mean_common"] < u["t_mean_common"]
    assert info["sdf_loss_last"] < info["sdf_loss_first"]
    files = sorted(os.listdir(out))
    assert "view_00_depth.npy" in files and "view_01_depth.npy" in files and all(os.path.exists(p) for p in info["out"])
    depth = np.load(out / "view_00_depth.npy")
    assert depth.shape == (32, 32) and np.array_equal(np.isfinite(depth), info["views"][0]["mask"].cpu().numpy())
    assert '"trained"' in captured and os.path.exists(tmp_path / "fit.json")
