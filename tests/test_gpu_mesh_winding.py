"""Generalized winding numbers on the GPU (csrc/mesh_winding.hip through ngp_hip.MeshSDF.winding / inside / sign="winding") against the
numpy reference of the contract (tests/mesh_winding_reference.py: exact = the float64 sum over all faces, tree64 / tree32 = the walk
with the acceptance rule in float64 and in serial float32, over THE PACKAGE'S OWN ORDER of the faces).

THE STANDARD ASSERTION (_check; every test asserts it unless it says otherwise), per set, beta and number of far-field terms:
  beta = 2     on decided points |w - tree64| <= 4 E32; on every point |w - exact| <= 2 A_set + 4 E32 (a flipped acceptance test trades one
               node's approximation for its children's, each already within the set's error scale: hence the factor 2); inside() equals
               exact >= 0.5 wherever |exact - 0.5| > 2 A_set + 4 E32
  beta = inf   |w - exact| <= 4 E32 on every point: nothing is accepted, nothing can flip"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_sdf_reference as M
import mesh_winding_reference as W
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mesh(v, f, **kw):
    from ngp_hip import MeshSDF
    kw.setdefault("signed", False)
    return MeshSDF(torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(np.ascontiguousarray(f)), **kw)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _winding(m, x, **kw):
    w = m.winding(x, **kw)
    assert w.dtype == torch.float32 and w.shape == (x.shape[0],) and not w.requires_grad
    return w


def _check(c, mesh=None, leaf_size=4, terms=(1, 2), decided_too=True, exact=None):
    """THE STANDARD ASSERTION for the case c (module docstring); exact: judge against this truth instead of the case's own."""
    m = mesh if mesh is not None else _mesh(c.vertices, c.faces, leaf_size=leaf_size)
    assert m.n_faces == len(c.faces)
    order = m.order.cpu().numpy()
    x = _t(c.points)
    out = {}
    for k in terms:
        r = c.ref(2.0, k, order=order, leaf_size=leaf_size)
        truth = r["exact"] if exact is None else exact
        w = _winding(m, x, beta=2.0, order=k).cpu().numpy().astype(np.float64)
        dec = r["decided"]
        err_dec = float(np.abs(w - r["tree64"])[dec].max()) if dec.any() else 0.0
        err_all, bound = float(np.abs(w - truth).max()), 2 * r["a_set"] + 4 * r["e32"]
        print("%s leaf %d order %d: %d of %d decided, |w - tree64| %.3g on them (%.2f x E32 %.3g); |w - exact| %.3g (A_set %.3g, bound %.3g)"
              % (c.name, leaf_size, k, dec.sum(), len(w), err_dec, err_dec / r["e32"], r["e32"], err_all, r["a_set"], bound))
        assert np.isfinite(w).all()
        if decided_too:
            assert err_dec <= 4 * r["e32"], (c.name, k, err_dec, r["e32"])
        assert err_all <= bound, (c.name, k, err_all, bound)
        clear = np.abs(truth - 0.5) > bound
        inside = m.inside(x, beta=2.0, order=k)
        assert inside.dtype == torch.bool and np.array_equal(inside.cpu().numpy()[clear], (truth >= 0.5)[clear])
        out[k] = w
    r = c.ref(INF, 2, order=order, leaf_size=leaf_size)
    truth = r["exact"] if exact is None else exact
    for k in terms:
        w = _winding(m, x, beta=INF, order=k).cpu().numpy().astype(np.float64)
        err = float(np.abs(w - truth).max())
        print("%s leaf %d beta inf: |w - exact| %.3g (%.2f x E32 %.3g)" % (c.name, leaf_size, err, err / r["e32"], r["e32"]))
        assert err <= 4 * r["e32"], (c.name, err, r["e32"])
    out[INF] = w
    return m, out


@pytest.mark.parametrize("name", W.CASES)
def test_named_sets(hip_lib, name):
    """Cube, icosphere, the extracted torus, a soup of 500 faces, the open quad, two overlapping spheres and the sphere with a hole;
    points uniform in the padded box, near the surface, and 10 and 1000 diameters away."""
    c = W.case(name)
    m, _ = _check(c)
    for k in (1, 2):
        assert 1.0 - c.ref(2.0, k, order=m.order.cpu().numpy())["decided"].mean() <= W.MAX_UNDECIDED


_SOUPS = {}


def _soup_case(n_faces, **kw):
    key = (n_faces, tuple(sorted(kw.items())))
    if key not in _SOUPS:
        v, f = M.soup(n_faces, seed=n_faces, **kw)
        rng = np.random.default_rng(n_faces + 1)
        _SOUPS[key] = W.Case("soup%d%s" % (n_faces, "/same centroid" if kw else ""), v, f,
                             np.concatenate([M.pts_uniform(v, 96, rng), M.pts_near(v, f, 96, rng)]))
    return _SOUPS[key]


@pytest.mark.parametrize("leaf_size", [1, 4, 8])
@pytest.mark.parametrize("n_faces", [1, 2, 3, 5, 13, 4097])
def test_face_counts_and_leaf_sizes(hip_lib, n_faces, leaf_size):
    """Trees of one node up to 4097 leaves of one face (depth 13, 4095 of the 8192 leaves padding), triangle soups, beta = inf and 2."""
    _check(_soup_case(n_faces), leaf_size=leaf_size, terms=(2,))


def test_mesh_far_from_the_origin(hip_lib):
    """The icosphere moved to lo = 100: coordinates lose 8 bits.  The exact sum follows through E32 (the face terms are differences from
    the query point, the leaf moments are formed about a corner of the leaf, the levels combine by differences of centroids).  An ulp of
    the coordinates is now 8e-6, of the order of NEAR_ACCEPT x |d| itself, so `decided` as the reference defines it no longer says
    that float32 takes the same decisions: only the bound that allows flips is asserted at beta = 2."""
    v, f = M.icosphere()
    v = (v.astype(np.float64) + 100.0).astype(np.float32)
    rng = np.random.default_rng(100)
    c = W.Case("icosphere at 100", v, f, np.concatenate([M.pts_uniform(v, 384, rng), M.pts_near(v, f, 384, rng)]))
    _check(c, decided_too=False)
    inside = np.linalg.norm(c.points.astype(np.float64) - 100.5, axis=1) < 0.33
    assert inside.sum() > 50 and np.abs(c.exact()[inside] - 1.0).max() < 1e-9


def test_one_morton_code_and_duplicated_faces(hip_lib):
    """200 faces around one centroid (the sort cannot separate them), and a cube one of whose faces is there 65 times: every copy
    counts, the winding number is that of the face list."""
    _check(_soup_case(200, same_centroid=True, size=0.3))
    v, f = M.cube()
    f = np.concatenate([np.repeat(f[:1], 64, axis=0), f])
    c = W.Case("cube + 64 copies of a face", v, f, M.pts_uniform(v, 256, np.random.default_rng(64)))
    for leaf_size in (4, 1):
        _check(c, leaf_size=leaf_size)
    assert c.exact().max() > 2.0


def test_zero_area_face_changes_nothing(hip_lib):
    """Three collinear points with distinct indices, first in the face list of the icosphere: every result is finite and within the
    bounds of the icosphere WITHOUT that face."""
    v0, f0 = M.icosphere()
    v = np.concatenate([v0, [[0.4, 0.5, 0.9], [0.5, 0.5, 0.9], [0.6, 0.5, 0.9]]]).astype(np.float32)
    f = np.concatenate([[[len(v) - 3, len(v) - 2, len(v) - 1]], f0]).astype(np.int32)
    x = np.concatenate([W.case("icosphere/uniform").points, [[0.45, 0.5, 0.9], [0.7, 0.5, 0.9], [0.5, 0.5, 0.9]]]).astype(np.float32)
    c = W.Case("icosphere + a zero-area face", v, f, x)
    without = W.exact(x, v0, f0)
    for leaf_size in (1, 4):
        m, _ = _check(c, leaf_size=leaf_size, exact=without)
        assert m.n_faces == len(f)


@pytest.mark.parametrize("name,leaf_size", [("icosphere/uniform", 4), ("soup500/uniform", 1), ("soup500/uniform", 8), ("two_spheres/uniform", 4)])
def test_moments(hip_lib, name, leaf_size):
    """Every column of every row within 4 x the error of the serial float32 rows of the reference against its float64 rows (at least one
    float32 ulp of the column's largest entry); the boxes the reference restates are the device's, bit for bit; for every node with faces
    r (1 + 2^-20) >= the float64 distance from the DEVICE's p to every vertex below the node: the radius is never optimistic; two builds
    give the same bytes."""
    from ngp_hip import ops
    c = W.case(name)
    m = _mesh(c.vertices, c.faces, leaf_size=leaf_size)
    order = m.order.cpu().numpy()
    box, m64, m32 = c.moments(order, leaf_size)
    assert np.array_equal(m.boxes.cpu().numpy().view(np.uint32), box.view(np.uint32))
    got = m.moments
    assert got.shape == m64.shape and got.dtype == torch.float32 and got.data_ptr() % 16 == 0
    again = ops.mesh_winding_build(m.vertices, m.faces, m.order, m.boxes, leaf_size)
    assert torch.equal(_bits(got), _bits(again))
    g = got.cpu().numpy().astype(np.float64)
    e32 = np.maximum(np.abs(m32.astype(np.float64) - m64).max(0), M.ulp32(np.abs(m64).max(0)))
    err = np.abs(g - m64).max(0)
    print("%s leaf %d: %d rows; column errors / E32: %s" % (name, leaf_size, len(g), np.array2string(err / e32, precision=2)))
    assert (err <= 4 * e32).all(), (err / e32)
    assert np.array_equal(g[:, 17], (g[:, 3] >= 0).astype(np.float64)) and (g[:, 18:] == 0).all()
    P, _ = W.shape(len(order), leaf_size)
    below = {P - 1 + k: c.faces[order[leaf_size * k:leaf_size * (k + 1)]].reshape(-1) for k in range(P)}
    for i in range(P - 2, -1, -1):
        below[i] = np.concatenate([below[2 * i + 1], below[2 * i + 2]])
    slack = 0.0
    for i, idx in below.items():
        assert (g[i, 3] >= 0) == (len(idx) > 0), i
        if len(idx):
            reach = np.linalg.norm(c.vertices[idx].astype(np.float64) - g[i, 0:3], axis=1).max()
            assert g[i, 3] * (1 + 2.0**-20) >= reach, (i, g[i, 3], reach)
            slack = max(slack, reach / g[i, 3])
    print("%s leaf %d: the farthest vertex below a node reaches %.4f of its radius at most" % (name, leaf_size, slack))


@pytest.mark.parametrize("n", [0, 1, 65, 4096])
def test_batch_sizes_and_permutations(hip_lib, n):
    """A result depends on its point and the tree alone: the same bits between two calls, under a permutation of the batch, and as a
    part of a larger batch."""
    c = W.case("torus/near")
    m = _mesh(c.vertices, c.faces)
    rng = np.random.default_rng(n)
    x = _t(np.concatenate([M.pts_uniform(c.vertices, n - n // 2, rng), M.pts_near(c.vertices, c.faces, n // 2, rng)]).astype(np.float32).reshape(-1, 3))
    for kw in (dict(), dict(beta=3.0, order=1)):
        a, b = _winding(m, x, **kw), _winding(m, x, **kw)
        assert torch.equal(_bits(a), _bits(b))
        perm = torch.from_numpy(rng.permutation(n)).to(DEV)
        assert torch.equal(_bits(_winding(m, x[perm].contiguous(), **kw)), _bits(a[perm]))
        assert torch.equal(_bits(_winding(m, x[:n // 3].contiguous(), **kw)), _bits(a[:n // 3]))
    assert m.inside(x).shape == (n,)
    if n > 1:
        assert 0 < int(m.inside(x).sum()) < n


def test_special_points_in_one_batch_with_good_ones(hip_lib):
    """NaN and +-inf coordinates give NaN for their own point and leave the others' bits alone; points exactly on vertices, edge
    midpoints and face centroids give finite values (not judged: the winding number jumps there)."""
    c = W.case("icosphere/near")
    m = _mesh(c.vertices, c.faces)
    nan, inf = np.nan, np.inf
    bad = np.array([[nan, .5, .5], [.5, inf, .5], [.5, .5, -inf], [nan, nan, nan], [inf, -inf, nan], [inf, inf, inf]], np.float32)
    tri = c.vertices[c.faces].astype(np.float64)
    on = np.concatenate([c.vertices[:200], (0.5 * (tri[:200, 0] + tri[:200, 1])).astype(np.float32), tri[:200].mean(1).astype(np.float32)])
    x = np.concatenate([bad, on, c.points]).astype(np.float32)
    pos = np.random.default_rng(3).permutation(len(x))
    inv = torch.from_numpy(np.argsort(pos)).to(DEV)
    alone = _winding(m, _t(c.points))
    for kw in (dict(), dict(beta=INF), dict(order=1)):
        mixed = _winding(m, _t(x[pos]), **kw)[inv]
        assert bool(torch.isnan(mixed[:len(bad)]).all())
        assert bool(torch.isfinite(mixed[len(bad):]).all())
        if not kw:
            assert torch.equal(_bits(mixed[len(bad) + len(on):]), _bits(alone))
    inside = m.inside(_t(bad))
    assert not bool(inside.any())                                         # NaN >= 0.5 is false


def test_entries_refuse_bad_arguments(hip_lib):
    """-1, nothing launched or written: null pointers, n < 0, n_faces < 1, a leaf_size outside 1..8, beta below 1 or NaN, order_terms
    other than 1 or 2; 0 and nothing written for n = 0."""
    lib = hip_lib
    from ngp_hip import ops
    v, f = M.cube()
    tv, tf, order = _t(v), _t(f), torch.arange(12, device=DEV, dtype=torch.int32)
    boxes = ops.mesh_bvh_build(tv, tf, order, 4)
    assert lib.ngp_mesh_winding_bytes(12, 4) == 80 * 7 and lib.ngp_mesh_winding_bytes(4097, 1) == 80 * 16383
    for bad in ((0, 4), (-1, 4), (12, 0), (12, 9), (2**31, 8), (2**25, 1)):
        assert lib.ngp_mesh_winding_bytes(*bad) == -1 and lib.ngp_mesh_bvh_bytes(*bad) == -1
    moments = torch.full((7, 20), 7.0, device=DEV)
    p = lambda x: x.data_ptr()
    build = lambda **kw: lib.ngp_mesh_winding_build(*[kw.get(k, dflt) for k, dflt in (
        ("vertices", p(tv)), ("faces", p(tf)), ("order", p(order)), ("boxes", p(boxes)), ("n_faces", 12), ("leaf_size", 4),
        ("moments", p(moments)), ("stream", 0))])
    for bad in (dict(vertices=0), dict(faces=0), dict(order=0), dict(boxes=0), dict(moments=0), dict(n_faces=0), dict(n_faces=-3),
                dict(leaf_size=0), dict(leaf_size=9)):
        assert build(**bad) == -1, bad
    torch.cuda.synchronize()
    assert (moments == 7.0).all()
    assert build() == 0
    x = _t(W.case("cube/uniform").points[:8])
    w = torch.full((8,), 7.0, device=DEV)
    query = lambda **kw: lib.ngp_mesh_winding_query(*[kw.get(k, dflt) for k, dflt in (
        ("points", p(x)), ("n", 8), ("vertices", p(tv)), ("faces", p(tf)), ("order", p(order)), ("moments", p(moments)), ("n_faces", 12),
        ("leaf_size", 4), ("beta", 2.0), ("order_terms", 2), ("winding", p(w)), ("stream", 0))])
    for bad in (dict(points=0), dict(vertices=0), dict(faces=0), dict(order=0), dict(moments=0), dict(winding=0), dict(n=-1), dict(n_faces=0),
                dict(n_faces=-3), dict(leaf_size=0), dict(leaf_size=9), dict(beta=0.5), dict(beta=0.999), dict(beta=-2.0), dict(beta=float("nan")),
                dict(beta=-INF), dict(order_terms=0), dict(order_terms=3), dict(order_terms=-1)):
        assert query(**bad) == -1, bad
    assert query(n=0) == 0 and query(n=0, points=0, winding=0) == 0
    torch.cuda.synchronize()
    assert (w == 7.0).all()
    assert query() == 0 and query(beta=1.0, order_terms=1) == 0 and query(beta=INF) == 0
    torch.cuda.synchronize()
    truth = W.exact(x.cpu().numpy(), v, f)
    assert np.abs(w.cpu().numpy() - truth).max() <= 1e-5


def test_ops_and_meshsdf_validate_before_any_launch(hip_lib, monkeypatch):
    from ngp_hip import MeshSDF, ops
    c = W.case("cube/uniform")
    m = _mesh(c.vertices, c.faces)
    built = _mesh(c.vertices, c.faces)
    moments = built.moments
    x = _t(c.points)

    class Boom:
        def __getattr__(self, name):
            if name in ("ngp_mesh_bvh_bytes", "ngp_mesh_winding_bytes"):
                return getattr(hip_lib, name)
            raise AssertionError("a launch for arguments that must be refused")
    monkeypatch.setattr(ops, "_lib", lambda: Boom())
    args = (m.vertices, m.faces, m.order)
    with pytest.raises(ValueError):
        ops.mesh_winding_query(x.view(-1), *args, moments, 4)
    with pytest.raises(TypeError):
        ops.mesh_winding_query(x.double(), *args, moments, 4)
    with pytest.raises(RuntimeError):
        ops.mesh_winding_query(x.cpu(), *args, moments, 4)
    with pytest.raises(ValueError):
        ops.mesh_winding_query(x.t().contiguous().t(), *args, moments, 4)
    with pytest.raises(ValueError):
        ops.mesh_winding_query(x, *args, moments[:-1], 4)
    with pytest.raises(TypeError):
        ops.mesh_winding_query(x, *args, moments.double(), 4)
    with pytest.raises(ValueError):
        ops.mesh_winding_query(x, *args, moments, 9)
    for beta in (0.5, float("nan"), -INF):
        with pytest.raises(ValueError, match="beta"):
            ops.mesh_winding_query(x, *args, moments, 4, beta=beta)
        with pytest.raises(ValueError, match="beta"):
            m.winding(x, beta=beta)
    with pytest.raises(ValueError, match="order"):
        ops.mesh_winding_query(x, *args, moments, 4, order_terms=3)
    with pytest.raises(ValueError, match="order"):
        m.winding(x, order=3)
    with pytest.raises(ValueError):
        m.inside(x.view(-1))
    with pytest.raises(TypeError):
        m.winding(x.double())
    with pytest.raises(RuntimeError):
        m.winding(x.cpu())
    with pytest.raises(ValueError):
        ops.mesh_winding_build(m.vertices, m.faces, m.order, m.boxes[:-1], 4)
    with pytest.raises(TypeError):
        ops.mesh_winding_build(m.vertices, m.faces.long(), m.order, m.boxes, 4)
    with pytest.raises(ValueError, match="sign"):
        MeshSDF(torch.from_numpy(c.vertices), torch.from_numpy(c.faces), sign="parity")
    assert m._moments is None                                             # none of the refused calls built the moments
    with pytest.raises(AssertionError):
        m.winding(x)                                                      # the guard itself: a good call does reach the library
    monkeypatch.undo()
    assert torch.equal(_bits(m.winding(x)), _bits(built.winding(x))) and m._moments is not None


def _both_signs(v, f):
    return _mesh(v, f, signed=True, sign="winding"), _mesh(v, f, signed=True)


@pytest.mark.parametrize("name", ["icosphere/uniform", "icosphere/near", "torus/uniform", "torus/near"])
def test_sign_by_winding_agrees_with_the_pseudonormal_sign_on_closed_meshes(hip_lib, name):
    """|sdf| has the bits of the unsigned query, closest / face / feature those of either; on every decided point of
    mesh_sdf_reference the sign is the pseudonormal instance's (and the reference's); sign="pseudonormal" is the instance without the
    keyword, byte for byte."""
    c = M.case(name)
    win, pseudo = _both_signs(c.vertices, c.faces)
    assert win.edge_normals is None and win.vertex_normals is None and pseudo.edge_normals is not None
    x = _t(c.points)
    a, b, u = win(x), pseudo(x), _mesh(c.vertices, c.faces)(x)
    assert torch.equal(_bits(a.sdf.abs()), _bits(u.sdf)) and torch.equal(_bits(b.sdf.abs()), _bits(u.sdf))
    for p, q in zip(a[1:], u[1:]):
        assert torch.equal(_bits(p), _bits(q))
    dec = c.ref()["decided"]
    sa, sb = (np.where(s.sdf.cpu().numpy() < 0, -1.0, 1.0) for s in (a, b))
    print("%s: %d of %d decided, the two signs differ on %d of them (%d anywhere)" % (name, dec.sum(), len(dec), (sa != sb)[dec].sum(), (sa != sb).sum()))
    assert np.array_equal(sa[dec], sb[dec]) and np.array_equal(sa[dec], c.ref()["sign"][dec]) and (sa < 0).sum() > 10
    named = _mesh(c.vertices, c.faces, signed=True, sign="pseudonormal")(x)
    for p, q in zip(named, b):
        assert torch.equal(_bits(p), _bits(q))
    only = win(x, details=False)
    assert only.closest is None and torch.equal(_bits(only.sdf), _bits(a.sdf))
    assert torch.equal(_mesh(c.vertices, c.faces, sign="winding")(x).sdf, u.sdf)                  # signed=False stays unsigned


def test_sign_by_winding_is_right_where_the_pseudonormal_sign_is_not(hip_lib):
    """Two overlapping spheres: on every judged point (farther than the sagitta + 0.01 from both spheres) the winding sign is that of the
    analytic union; the pseudonormal instance, on the same device in the same test, is wrong on some -- all inside the union."""
    v, f = W.two_spheres()
    x = np.concatenate([W.case("two_spheres/uniform").points, W.case("two_spheres/near").points])
    judged, inside = W.two_spheres_judged(x), W.two_spheres_sdf(x) < 0
    win, pseudo = _both_signs(v, f)
    sw, sp = (s(_t(x), details=False).sdf.cpu().numpy() for s in (win, pseudo))
    wrong_w, wrong_p = judged & ((sw < 0) != inside), judged & ((sp < 0) != inside)
    print("two spheres: %d judged, %d inside the union; wrong signs: winding %d, pseudonormal %d" % (judged.sum(), (judged & inside).sum(), wrong_w.sum(), wrong_p.sum()))
    assert judged.sum() > 600 and wrong_w.sum() == 0
    assert wrong_p.sum() > 0 and inside[wrong_p].all()
    assert np.array_equal(np.abs(sw), np.abs(sp))
    assert np.array_equal(win.inside(_t(x)).cpu().numpy()[judged], inside[judged])


@pytest.mark.parametrize("resolution", [32, 64])
def test_closed_loop_with_the_extractor(hip_lib, resolution):
    """extract_mesh of the sphere |x - c| - 0.3 -> MeshSDF.inside: the analytic sign for every point farther than one cell from the
    surface, for both orders and for the exact sum."""
    from ngp_hip import MeshSDF
    from ngp_hip.mesh import extract_mesh
    centre = torch.tensor([0.52, 0.49, 0.5], dtype=torch.float32, device=DEV)
    mesh = extract_mesh(lambda x: torch.linalg.norm(x - centre, dim=1) - 0.3, resolution, 0.0, bounds=((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                        sign=-1, normals=None, device=torch.device(DEV))
    m = MeshSDF.from_mesh(mesh, signed=False)
    x = torch.rand(4096, 3, generator=torch.Generator().manual_seed(resolution)).to(DEV)
    d = (torch.linalg.norm(x.double() - centre.double(), dim=1) - 0.3).cpu().numpy()
    clear = np.abs(d) > 1.0 / resolution
    assert (clear & (d < 0)).sum() > 200 and (clear & (d > 0)).sum() > 2000
    for kw in (dict(), dict(order=1), dict(beta=INF)):
        w = m.winding(x, **kw).cpu().numpy()
        print("%d^3, %d faces, %s: w in %.4f .. %.4f inside and %.4f .. %.4f outside" % (resolution, m.n_faces, kw or "defaults", w[clear & (d < 0)].min(),
              w[clear & (d < 0)].max(), w[clear & (d > 0)].min(), w[clear & (d > 0)].max()))
        assert np.array_equal(m.inside(x, **kw).cpu().numpy()[clear], (d < 0)[clear])


def test_fit_example_on_two_spheres_by_winding(hip_lib, capsys):
    """examples/fit_sdf_mesh.py --target two_spheres --sign winding for a handful of steps at 32^3: it runs and prints its figures (a smoke
    run, no quality bar); the winding sign is right on its probe batch and the pseudonormal sign is not."""
    spec = importlib.util.spec_from_file_location("fit_sdf_mesh_example", os.path.join(ROOT, "examples", "fit_sdf_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    common = ["--target", "two_spheres", "--subdivisions", "2", "--steps", "5", "--n", "2048", "--log2_T", "14", "--levels", "8", "--max_res", "128",
              "--resolution", "32", "--compare_n", "4096"]
    info = ex.main(common + ["--sign", "winding"])
    other = ex.main(common + ["--steps", "1"])
    out = capsys.readouterr().out
    print("fit_sdf_mesh two_spheres: winding wrong on %.4f of the probe, pseudonormal on %.4f; the two differ on %.4f; sdf loss %.4f -> %.4f"
          % (info["sign_wrong"], other["sign_wrong"], info["sign_disagreement"], info["sdf_loss_first"], info["sdf_loss_last"]))
    assert info["sign"] == "winding" and info["target_name"] == "two_spheres" and info["target_faces"] == 640 and '"sign_wrong"' in out
    assert np.isfinite(info["sdf_loss_last"]) and info["sign_wrong"] == 0.0 and other["sign_wrong"] > 0.0
    assert info["sign_disagreement"] == other["sign_disagreement"] > 0.0
