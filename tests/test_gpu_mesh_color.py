"""Vertex colours on the GPU (csrc/mesh_color.hip through ngp_hip.bake_image_colors, bake_field_colors and render_mesh(colors=)) against
the numpy reference of the contract (tests/mesh_color_reference.py).

THE STANDARD ASSERTION is the reference's judge(): on the decided vertices of a named set views and filled are exact and colours and
weight lie within 4 x E32 of float64, E32 being the float32 restatement's own error on that set.  The sets are small (an icosphere of
162 vertices, 32 x 32 images, at most 7 cameras) and their references are computed once per process."""
import numpy as np
import pytest
import torch

import mesh_color_reference as R
import mesh_sdf_reference as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = np.float32, np.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(x):
    return x.detach().cpu().numpy()


def _bits(x):
    a = _np(x) if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.int32)


def _mesh(v, f, normals=None):
    from ngp_hip import mesh
    return mesh.Mesh(_t(np.asarray(v, F32).reshape(-1, 3)), _t(np.asarray(f, np.int32).reshape(-1, 3)), normals)


def _bake(case, vertices=None, normals=None, cameras=slice(None), **kw):
    """bake_image_colors on a named set (its eps and options), without fill rounds unless asked for."""
    import ngp_hip
    v = case.vertices if vertices is None else vertices
    n = case.normals if normals is None else normals
    K = case.K if case.K.ndim == 2 else case.K[cameras]
    kw.setdefault("fill_rounds", 0)
    return ngp_hip.bake_image_colors(_mesh(v, case.faces), _t(case.images[cameras]), _t(K), _t(case.c2w[cameras]), normals=_t(n), eps=case.eps,
                                     **dict(case.options, **kw))


def _judge(case, got):
    assert got.colors.dtype == torch.float32 and got.weight.dtype == torch.float32 and got.views.dtype == torch.int32 and got.filled.dtype == torch.uint8
    return R.judge(case, _np(got.colors), _np(got.weight), _np(got.views), _np(got.filled))


def _same(a, b, rows=slice(None)):
    return all(np.array_equal(_bits(x)[rows], _bits(y)[rows]) for x, y in zip(a, b))


def test_convex(hip_lib):
    """The icosphere from six cameras: the standard assertion, and underneath it the launches one by one -- the accepted set of the
    projection and the pairs that count after the ray cast are the reference's on every decided pair."""
    from ngp_hip import MeshSDF, ops
    case = R.case("convex")
    got = _bake(case)
    _judge(case, got)
    assert (_np(got.views) > 0).all() and (_np(got.views) >= 2).sum() > 50
    ref = case.ref()
    eps = torch.full((1,), case.eps, dtype=torch.float32).to(DEV)
    rays_o, rays_d, sample, weight, cosv = ops.mesh_color_project(_t(case.vertices), _t(case.normals), _t(case.K), _t(case.c2w), R.WH, eps)
    shape = ref["decided_pairs"].shape
    accept = _np(weight).reshape(shape) > 0
    dec = ref["decided_pairs"]
    assert np.array_equal(accept[dec], ref["r64"]["project"]["accept"][dec])
    t = MeshSDF(case.vertices, case.faces, signed=False).raycast(rays_o, rays_d, t_min=0.0, t_max=1.0, any_hit=True, details=False).t
    counts = accept & ~np.isfinite(_np(t).reshape(shape))
    assert np.array_equal(counts[dec], ref["r64"]["counts"][dec])
    p32 = ref["r32"]["project"]
    same = [int((_bits(x).reshape(shape + (-1,)) != _bits(p32[k].astype(F32)).reshape(shape + (-1,))).any(-1).sum())
            for x, k in ((sample[:, 0], "a"), (sample[:, 1], "b"), (weight, "weight"), (cosv, "cos"), (rays_o, "o"), (rays_d, "d"))]
    print("convex: pairs that differ in bits from the float32 restatement (a, b, weight, cos, o, d):", same)
    rejected = ~accept.reshape(-1)
    assert not _np(rays_d)[rejected].any() and not _np(rays_o)[rejected].any() and np.isinf(_np(t)[rejected]).all()


def test_occluder(hip_lib):
    """Two parallel squares: camera A sees four vertices of the far one only past the near one, camera B sees them freely -- they carry
    B's colour alone, bit for bit what a bake from B alone gives them."""
    case = R.case("occluder")
    got = _bake(case)
    _judge(case, got)
    far = case.vertices[:9]
    covered = np.flatnonzero((far[:, 0] >= 0.5) & (far[:, 1] >= 0.5))
    free = np.setdiff1d(np.arange(9), covered)
    assert len(covered) == 4 and (_np(got.views)[covered] == 1).all() and (_np(got.views)[free] == 2).all()
    only_b = _bake(case, cameras=slice(1, 2))
    assert (_np(only_b.views)[:9] == 1).all()
    assert _same(got[:2], only_b[:2], covered) and not np.array_equal(_bits(got.colors)[free], _bits(only_b.colors)[free])


def test_chunk_independence(hip_lib):
    """Seven cameras in chunks of 1, 3 and 7 (the workspace sized for exactly that many), in both modes: the same bytes.  Two runs: the
    same bytes.  The vertices permuted: the result permuted."""
    case = R.case("seven")
    per_camera = 44 * len(case.vertices)
    blend = None
    for mode in ("blend", "best"):
        whole = _bake(case, mode=mode, workspace_bytes=7 * per_camera)
        if mode == "blend":
            _judge(case, whole)
            blend = whole
        else:
            assert not _same(whole[:1], blend[:1])
        for k in (1, 3):
            assert _same(whole, _bake(case, mode=mode, workspace_bytes=k * per_camera + 5)), (mode, k)
        assert _same(whole, _bake(case, mode=mode, workspace_bytes=0)) and _same(whole, _bake(case, mode=mode)), mode
    perm = np.random.default_rng(9).permutation(len(case.vertices))
    inverse = np.argsort(perm)
    moved = R.Case("seven, permuted", case.vertices[perm], inverse[case.faces], case.normals[perm], case.images, case.K, case.c2w, eps=case.eps)
    got = _bake(moved)
    assert _same([x[_t(inverse)] for x in got], blend)


@pytest.mark.parametrize("name", ["v1", "v65", "one_camera", "per_camera_K", "flipped", "flipped_one_sided"])
def test_edges_of_the_mapping(hip_lib, name):
    """One vertex (and no face), 65 vertices (a wave and one lane), one camera, a K per camera with four-channel images, inward normals
    with and without two_sided."""
    case = R.case(name)
    got = _bake(case)
    _judge(case, got)
    if name == "flipped":
        assert _same(got, _bake(R.case("convex")))
    if name == "flipped_one_sided":
        assert not _np(got.views).any() and (_np(got.filled) == 255).all() and np.array_equal(_np(got.colors), np.full((162, 3), 0.5, F32))


def test_no_vertices_and_no_cameras(hip_lib):
    import ngp_hip
    case = R.case("convex")
    none = ngp_hip.bake_image_colors(_mesh(np.zeros((0, 3), F32), case.faces), _t(case.images), _t(case.K), _t(case.c2w),
                                     normals=_t(np.zeros((0, 3), F32)), eps=1e-3)
    assert none.colors.shape == (0, 3) and none.weight.shape == (0,) and none.views.shape == (0,) and none.filled.shape == (0,)
    blind = ngp_hip.bake_image_colors(_mesh(case.vertices, case.faces), _t(case.images[:0]), _t(case.K), _t(case.c2w[:0]), normals=_t(case.normals),
                                      default_color=(0.25, 0.5, 0.75))
    assert not _np(blind.views).any() and (_np(blind.filled) == 255).all() and np.array_equal(_np(blind.colors), np.tile(np.array([0.25, 0.5, 0.75], F32), (162, 1)))


def test_nan_vertex_and_nan_normal(hip_lib):
    """A vertex and, elsewhere, a normal that are not finite: views 0 there, not a bit changed anywhere else."""
    case = R.case("convex")
    clean = _bake(case)
    v, n = case.vertices.copy(), case.normals.copy()
    v[40, 1], n[100, 2], n[101, 0] = np.nan, np.nan, np.inf
    got = _bake(case, vertices=v, normals=n)
    bad = np.array([40, 100, 101])
    rest = np.setdiff1d(np.arange(len(v)), bad)
    assert not _np(got.views)[bad].any() and (_np(got.filled)[bad] == 255).all() and (_np(clean.views)[bad] > 0).all()
    assert _same(got, clean, rest) and np.isfinite(_np(got.colors)).all()


def test_fill(hip_lib):
    """Three cameras above the sphere: the lower cap has no view and is filled ring by ring -- from the device's own baked colours the
    reference's serial fill gives the same bytes; fill_rounds=0 leaves the default colour and 255."""
    import ngp_hip
    case = R.case("cap")
    default = (0.1, 0.2, 0.3)
    plain = _bake(case, default_color=default)
    _judge(case, plain)
    unseen = _np(plain.filled) == 255
    assert 10 <= unseen.sum() and np.array_equal(_np(plain.colors)[unseen], np.tile(np.asarray(default, F32), (unseen.sum(), 1)))
    for rounds in (1, 2, 8):
        got = _bake(case, default_color=default, fill_rounds=rounds)
        colors, filled = R.fill(_np(plain.colors), _np(plain.filled), case.faces, rounds, default)
        assert np.array_equal(_np(got.filled), filled) and np.array_equal(_bits(got.colors), _bits(colors)), rounds
        assert _same((got.weight, got.views), (plain.weight, plain.views)) and not _np(got.weight)[unseen].any()
        print("cap: %d unseen vertices, %d rounds: filled per round %s, %d left" % (unseen.sum(), rounds, np.bincount(filled[filled < 255])[1:].tolist(),
                                                                                   int((filled == 255).sum())))
    assert filled.max() == filled[filled < 255].max() >= 3 and (filled < 255).all()       # several rings, all reached within 8 rounds
    one = _np(_bake(case, fill_rounds=1).filled)
    assert (one == 255).any() and (one == 1).any()
    # the default mesh.normals / vertex_normals path and a given MeshSDF read nothing back
    target = ngp_hip.MeshSDF(case.vertices, case.faces, signed=False)
    msh = _mesh(case.vertices, case.faces)
    args = (_t(case.images), _t(case.K), _t(case.c2w))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        quiet = ngp_hip.bake_image_colors(msh, *args, target=target)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    loud = ngp_hip.bake_image_colors(msh, *args)
    assert _same(quiet, loud) and (_np(quiet.filled) < 255).all()
    ref = R.Case("cap, defaults", case.vertices, case.faces, _np(ngp_hip.vertex_normals(msh)), case.images, case.K, case.c2w)
    assert ref.eps == float(R.default_eps(case.vertices))
    R.judge(ref, *(_np(x) for x in ngp_hip.bake_image_colors(msh, *args, fill_rounds=0)))


@pytest.mark.parametrize("name", ["best", "tie"])
def test_best(hip_lib, name):
    case = R.case(name)
    got = _bake(case)
    _judge(case, got)
    assert (_np(got.views) <= 1).all()
    if name == "tie":                                                            # equal cos, bit for bit, in the middle column: camera 0 stays
        middle = np.flatnonzero(case.vertices[:, 0] == 0.5)
        first, second = _bake(case, cameras=slice(0, 1)), _bake(case, cameras=slice(1, 2))
        assert _same(got[:2], first[:2], middle) and not np.array_equal(_bits(got.colors)[middle], _bits(second.colors)[middle])
        assert np.array_equal(_bits(first.weight)[middle], _bits(second.weight)[middle])


def test_refusals(hip_lib):
    import ngp_hip
    case = R.case("convex")
    msh, args = _mesh(case.vertices, case.faces), (_t(case.images), _t(case.K), _t(case.c2w))
    kw = dict(normals=_t(case.normals))
    for bad in (dict(mode="mean"), dict(fill_rounds=255), dict(fill_rounds=-1), dict(cos_min=-0.1), dict(near=float("nan")), dict(default_color=(1, 2))):
        with pytest.raises(ValueError):
            ngp_hip.bake_image_colors(msh, *args, **dict(kw, **bad))
    with pytest.raises(ValueError):
        ngp_hip.bake_image_colors(msh, args[0], args[1], args[2][:5], **kw)
    with pytest.raises(ValueError):
        ngp_hip.bake_image_colors(msh, args[0][..., :2].contiguous(), args[1], args[2], **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ngp_hip.bake_image_colors(msh, args[0].cpu(), args[1], args[2], **kw)
    with pytest.raises(TypeError):
        ngp_hip.bake_image_colors(msh, *args, target=msh, **kw)


def test_bake_field_colors(hip_lib):
    """x = v + offset n, d = -n, chunk by chunk: the bits of the direct model call on the same chunks, for an NGP (autocast: the fused
    kernels), an SDFField and a plain callable."""
    import ngp_hip
    from modules.networks import NGP
    v, f = M.icosphere(2, centre=(0.0, 0.0, 0.0), radius=0.3)
    n = R.sphere_normals(v, (0.0, 0.0, 0.0))
    msh = _mesh(v, f, _t(n))
    torch.manual_seed(5)
    chunk, offset = 64, 0.01
    pieces = [(((_t(v)[s:s + chunk]) + offset * _t(n)[s:s + chunk]).contiguous(), (-_t(n)[s:s + chunk]).contiguous()) for s in range(0, len(v), chunk)]
    ngp = NGP(scale=0.5, log2_T=12, max_res=64).to(DEV)                        # 16 levels of 2 features: the fused MLP's width
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        want = torch.cat([ngp(x, d)[1].float() for x, d in pieces])
        got = ngp_hip.bake_field_colors(ngp, msh, offset=offset, chunk=chunk)
    assert got.dtype == torch.float32 and got.shape == (162, 3) and np.array_equal(_bits(got), _bits(want)) and float(got.std()) > 0
    field = ngp_hip.SDFField(scale=0.5, levels=4, log2_T=12, max_res=64).to(DEV)
    with torch.no_grad():
        want = []
        for x, d in pieces:
            _, feature, grad = field.sdf_and_grad(x)
            want.append(field.color(feature, grad / torch.linalg.norm(grad, dim=1).clamp_min(1e-12)[:, None], d).float())
        got = ngp_hip.bake_field_colors(field, msh, offset=offset, chunk=chunk)
    assert np.array_equal(_bits(got), _bits(torch.cat(want))) and float(got.std()) > 0
    plain = ngp_hip.bake_field_colors(lambda x, d: x * 0.5 + d, _mesh(v, f), chunk=100)           # no normals on the mesh: vertex_normals
    nv = ngp_hip.vertex_normals(_mesh(v, f))
    assert np.array_equal(_bits(plain), _bits(_t(v) * 0.5 + (-nv)))
    with pytest.raises(ValueError):
        ngp_hip.bake_field_colors(lambda x, d: x[:, :2], msh)


def test_render_mesh_colors(hip_lib):
    """rgb is the barycentric mean of the three vertex colours of the face hit, in float32 and in the order stated, 0 on a miss; without
    colors the dictionary has the keys it always had."""
    import ngp_hip
    from ngp_hip.rays import get_ray_directions, get_rays
    case = R.case("convex")
    target = ngp_hip.MeshSDF(case.vertices, case.faces, signed=False)
    col = np.random.default_rng(3).random((162, 3)).astype(F32)
    K, pose = _t(case.K), _t(case.c2w[2])
    plain = ngp_hip.render_mesh(target, K, pose, R.WH)
    out = ngp_hip.render_mesh(target, K, pose, R.WH, colors=_t(col))
    assert set(plain) == {"depth", "normal", "mask", "face"} and set(out) == set(plain) | {"rgb"}
    assert all(torch.equal(plain[k], out[k]) for k in plain) and out["rgb"].shape == (32, 32, 3) and out["rgb"].dtype == torch.float32
    rays_o, rays_d = get_rays(get_ray_directions(32, 32, K, device=DEV), pose)
    hit = target.raycast(rays_o.contiguous(), (rays_d / torch.linalg.norm(rays_d, dim=1, keepdim=True)).contiguous())
    face, bary = _np(hit.face), _np(hit.bary)
    assert np.array_equal(face, _np(out["face"]).reshape(-1)) and 0.2 < (face >= 0).mean() < 0.8
    c = col[case.faces[np.maximum(face, 0)]]
    v, w = bary[:, :1], bary[:, 1:]
    want = np.where((face >= 0)[:, None], (c[:, 0] * (F32(1.0) - v - w) + c[:, 1] * v) + c[:, 2] * w, F32(0.0))
    assert np.array_equal(_bits(out["rgb"].reshape(-1, 3)), _bits(want))
    with pytest.raises(ValueError):
        ngp_hip.render_mesh(target, K, pose, R.WH, colors=_t(col[:100]))
    both = ngp_hip.render_mesh(_mesh(case.vertices, case.faces), K, pose, R.WH, colors=col)          # a Mesh, host colours
    assert torch.equal(both["rgb"], out["rgb"])


def _closed_loop_bound(case):
    """Per vertex, a bound on |baked colour - linear_colour(v)| for the float64 contract, from the footprint of the texels it reads.

    The baked colour is a convex combination (over the views that count, then over the four texels of each) of image values, and a
    texel that hit the mesh holds L(h), L = linear_colour, h the first point of the mesh on the ray through the texel's centre.  So
    |colour - L(v)| <= |A|_2 max |h - v| over those texels, |A|_2 the spectral norm of L's matrix.  The mesh is convex with its
    vertices on the sphere of radius rho about m, and contains the ball of radius rho_in about m, rho_in = the smallest distance of a
    face's plane from m.  A ray that meets the inner ball therefore enters the mesh between its entry into the outer ball, p_out, and its
    entry into the inner ball, p_in, and |h - v| <= max(|p_out - v|, |p_in - v|): both in closed form from the camera, the texel and
    the two radii.  (That every such ray does meet the inner ball is asserted: cos_min = 0.7 keeps the views frontal.)  Roundings: a
    texel is stored in f32 (2^-24 of a value below 2), and the rays that drew the images had their directions rounded to f32, which
    turns them by at most sqrt(3) 2^-24 rad and moves h by at most (2.5 / 0.5) sqrt(3) 2^-24 < 1e-6 at these distances and angles."""
    r = case.ref()["r64"]
    p, counts = r["project"], r["counts"]
    v = case.vertices.astype(F64)
    rho = np.linalg.norm(v - R.CENTRE, axis=1).max()
    tri = v[case.faces]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    rho_in = ((tri[:, 0] - R.CENTRE) * nrm).sum(1) / np.linalg.norm(nrm, axis=1)
    assert rho_in.min() > 0.9 * rho
    rho_in = rho_in.min()
    lip = np.linalg.norm(R.linear_colour(np.zeros(3))[1], 2)
    bound = np.zeros(len(v))

    def enter(c, e, radius):
        oc = c - R.CENTRE
        b = (e * oc).sum(1)
        disc = b * b - ((oc * oc).sum() - radius * radius)
        assert (disc > 0).all()
        return c + (-b - np.sqrt(disc))[:, None] * e

    for j in range(len(case.c2w)):
        m = counts[j]
        x0, y0, x1, y1, _, _ = (x[m] for x in R.texels(p["a"][j], p["b"][j], R.WH[0], R.WH[1], F64))
        o, d = R.pixel_rays(case.K, case.c2w[j], *R.WH)
        for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
            e = d[yy, xx] / np.linalg.norm(d[yy, xx], axis=1, keepdims=True)
            far = np.maximum(np.linalg.norm(enter(o[0, 0], e, rho) - v[m], axis=1), np.linalg.norm(enter(o[0, 0], e, rho_in) - v[m], axis=1))
            bound[m] = np.maximum(bound[m], lip * far)
    return bound + lip * 1e-6 + 2.0**-24


def test_closed_loop(hip_lib):
    """Images of the icosphere painted with an affine function of the position, baked back: the device against the reference as
    everywhere, and the reference against the function itself within the footprint bound derived above."""
    case = R.case("closed_loop")
    got = _bake(case)
    _judge(case, got)
    r64 = case.ref()["r64"]
    seen = r64["views"] > 0
    truth = R.linear_colour(case.vertices)[0]
    bound = _closed_loop_bound(case)
    err = np.linalg.norm(r64["colors"] - truth, axis=1)
    dev_err = np.linalg.norm(_np(got.colors).astype(F64) - truth, axis=1)
    print("closed loop: %d vertices with a view; |reference - function| max %.3g, mean %.3g; the bound min %.3g, max %.3g; worst ratio %.3g; "
          "|device - function| max %.3g" % (seen.sum(), err[seen].max(), err[seen].mean(), bound[seen].min(), bound[seen].max(),
                                             (err[seen] / bound[seen]).max(), dev_err[seen].max()))
    assert seen.sum() > 80 and (err[seen] <= bound[seen]).all()
