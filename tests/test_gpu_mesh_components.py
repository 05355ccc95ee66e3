"""Connected components, the per-component table, selection and clean_mesh on the GPU (csrc/mesh_components.hip through ngp_hip.components /
select_components / clean_mesh) against the serial reference of the contract (tests/mesh_components_reference.py).

THE STANDARD ASSERTION (_check): vertex_component, face_component, n, bad_faces, unused_vertices and every integer column equal the
reference; lo and hi equal it bit for bit; area and volume are within (n + 16) 2^-52 sum m_f of the reference's fsum (the derivation is
the reference's module docstring); rounds is at most max(V, 1), the bound DESIGN.md states."""
import numpy as np
import pytest
import torch

import mesh_components_reference as R
import mesh_sdf_reference as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mesh(v, f, normals=None):
    from ngp_hip import mesh
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return mesh.Mesh(t(np.asarray(v, np.float32).reshape(-1, 3)), t(np.asarray(f, np.int32).reshape(-1, 3)), None if normals is None else t(normals))


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return _np(t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32))


def _check(v, f, strict=True, ref=None, what=""):
    import ngp_hip
    cc = ngp_hip.components(_mesh(v, f), strict=strict)
    lab, tab = ref if ref is not None else (lambda lab: (lab, R.table(v, f, lab)))(R.label(f, len(v)))
    print("%s V %d T %d: C %d, %d rounds" % (what, len(v), len(f), cc.n, cc.rounds))
    assert (cc.n, cc.bad_faces, cc.unused_vertices) == (lab["n"], lab["bad_faces"], lab["unused_vertices"])
    assert cc.vertex_component.dtype == torch.int32 and cc.face_component.dtype == torch.int32
    assert np.array_equal(_np(cc.vertex_component), lab["vertex_component"]) and np.array_equal(_np(cc.face_component), lab["face_component"])
    assert 0 <= cc.rounds <= max(len(v), 1)
    s = cc.stats
    assert s is cc.stats                                                   # computed once
    for name in R.INT_FIELDS:
        got = getattr(s, name)
        assert got.dtype == torch.int32 and np.array_equal(_np(got), tab[name]), name
    assert s.area.dtype == torch.float64 and s.volume.dtype == torch.float64 and s.lo.dtype == torch.float32
    for name in ("area", "volume"):
        err, bound = np.abs(_np(getattr(s, name)) - tab[name]), tab[name + "_bound"]
        if len(err):
            print("  %s: worst |device - fsum| / bound %.3g" % (name, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), name
    assert np.array_equal(_bits(s.lo), tab["lo"].view(np.int32)) and np.array_equal(_bits(s.hi), tab["hi"].view(np.int32))
    return cc


# ---- sizes around every boundary of the implementation: the 64-lane wave, the 512-slot scan chunk, many chunks ------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 20000])
def test_disjoint_triangles(n):
    v, f = R.disjoint_triangles(n, seed=n)
    cc = _check(v, f, what="disjoint")
    assert cc.n == n and cc.rounds == (2 if n else 0)


# ---- the two per-wave counters (bad faces in cc_mark_kernel, unused vertices in cc_assign_vertices_kernel): whole waves, a lone lane, a
# wave with its tail past the end, several blocks; all, half and a seventh of the faces bad; V / 3 unused vertices behind the used ones
@pytest.mark.parametrize("every", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_bad_faces_and_unused_vertices_are_counted_per_wave(n, every):
    v, f = R.disjoint_triangles(n, seed=n)
    v = np.concatenate([v, np.full((len(v) // 3, 3), 0.25, np.float32)])
    f = f.copy()
    bad = np.arange(0, n, every)
    f[bad[0::2], 1] = len(v)                                                   # the first index past the end
    f[bad[1::2], 2] = -1
    lab = R.label(f, len(v))
    assert lab["bad_faces"] == len(bad) and lab["unused_vertices"] == n + 3 * len(bad) and lab["n"] == n - len(bad)
    cc = _check(v, f, strict=False, ref=(lab, R.table(v, f, lab)), what="bad every %d" % every)
    assert cc.rounds == (2 if len(bad) < n else 1)             # a pass that joins every good face, a pass that finds nothing to join


def test_no_vertices_and_no_faces():
    empty_f = np.zeros((0, 3), np.int32)
    cc = _check(np.zeros((0, 3), np.float32), empty_f)
    assert (cc.n, cc.rounds) == (0, 0) and cc.stats.area.shape == (0,) and cc.stats.lo.shape == (0, 3)
    cc = _check(M.cube()[0], empty_f)                                          # V > 0, T = 0
    assert cc.unused_vertices == 8 and _np(cc.vertex_component).tolist() == [-1] * 8
    cc = _check(np.zeros((0, 3), np.float32), M.cube()[1], strict=False)       # V = 0, T > 0: every face is bad
    assert cc.bad_faces == 12 and _np(cc.face_component).tolist() == [-1] * 12


# ---- chains: the worst case for propagation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering", ["ascending", "descending", "random"])
def test_strip(numbering):
    v, f = R.strip(2**16 + 3, numbering, seed=5)
    cc = _check(v, f, what="strip " + numbering)
    assert cc.n == 1 and cc.rounds <= len(v)                                   # the bound DESIGN.md states: V
    assert cc.stats.euler.tolist() == [1] and cc.stats.boundary_edges.tolist() == [2**16 + 5]


@pytest.mark.parametrize("hub", [0, 5000, 10000])
def test_fan_contention(hub):
    v, f = R.fan(10**4, hub)
    cc = _check(v, f, what="fan hub %d" % hub)
    assert cc.n == 1 and cc.stats.euler.tolist() == [1] and cc.stats.boundary_edges.tolist() == [10**4]


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.NAMED))
def test_named_shapes(name):
    v, f, lab, tab = R.case(name)
    cc = _check(v, f, ref=(lab, tab), what=name)
    want = {"two_apart": 2, "two_sharing": 1, "three_on_edge": 1, "needle": 1, "soup500": 500, "open_quad": 1}.get(name)
    assert want is None or cc.n == want
    if name == "three_on_edge":
        assert cc.stats.nonmanifold_edges.tolist() == [1]
    if name == "two_sharing":
        assert cc.stats.euler.tolist() == [3]


# ---- a real extraction -----------------------------------------------------------------------------------------------------------------------
def _extract(cut):
    from ngp_hip import mesh
    values = torch.from_numpy(R.spheres_field(32, cut=cut)).to(DEV)
    return mesh.marching_tetrahedra(values, 0.0, sign=-1, lo=(0.0, 0.0, 0.0), h=(1 / 32,) * 3)


def test_extracted_spheres():
    import ngp_hip
    m = _extract(cut=False)
    v, f = _np(m.vertices), _np(m.faces)
    cc = _check(v, f, what="5 spheres at 33^3")
    assert cc.n == 5 and cc.stats.euler.tolist() == [2] * 5 and cc.stats.boundary_edges.tolist() == [0] * 5
    radius = sorted(r for _, r in R.SPHERES)
    volume = np.sort(_np(cc.stats.volume))
    assert np.allclose(volume, [4 / 3 * np.pi * r**3 for r in radius], rtol=0.15)          # outward: positive, about a sphere's at 3 - 4 cells
    m6 = _extract(cut=True)
    cc6 = ngp_hip.components(m6)
    assert cc6.n == 6 and sorted(cc6.stats.euler.tolist()) == [1, 2, 2, 2, 2, 2]
    cleaned, report = ngp_hip.clean_mesh(m6, closed_only=True)
    open_one = int(np.flatnonzero(_np(cc6.stats.boundary_edges) > 0)[0])
    assert report["components_dropped"] == 1 and report["kept"] == [c for c in range(6) if c != open_one]
    assert float(_np(cc6.stats.lo)[open_one, 2]) == 0.0                                     # it is the sphere the grid boundary cuts
    again = ngp_hip.components(cleaned)
    assert again.n == 5 and again.stats.boundary_edges.tolist() == [0] * 5 and again.unused_vertices == 0
    assert cleaned.normals is not None and cleaned.normals.shape == cleaned.vertices.shape


# ---- bad input -------------------------------------------------------------------------------------------------------------------------------
def test_bad_faces_and_unused_vertices():
    import ngp_hip
    v, f = R.two_tetrahedra_apart()
    v = np.concatenate([v, np.ones((2, 3), np.float32)])
    clean = _check(v, f)
    assert clean.unused_vertices == 2 and _np(clean.vertex_component).tolist() == [0] * 4 + [1] * 4 + [-1, -1]
    bad = np.array([[0, 1, -1], [2, 10, 3], [4, R.INT_MIN, 5], [2**31 - 1, 6, 7]], np.int32)
    f_bad = np.concatenate([f[:3], bad[:2], f[3:], bad[2:]]).astype(np.int32)
    with pytest.raises(ValueError, match="4 of the 12 faces"):
        ngp_hip.components(_mesh(v, f_bad))
    cc = _check(v, f_bad, strict=False)
    assert cc.bad_faces == 4 and _np(cc.face_component).tolist() == [0] * 3 + [-1, -1] + [0] + [1] * 4 + [-1, -1]
    assert np.array_equal(_np(cc.vertex_component), _np(clean.vertex_component))             # the neighbours' results are unchanged
    for name in R.INT_FIELDS + ("area", "volume", "lo", "hi"):
        assert np.array_equal(_bits(getattr(cc.stats, name)), _bits(getattr(clean.stats, name))), name


def test_non_finite_coordinates_leave_the_integers_alone():
    import ngp_hip
    v, f, lab, tab = R.case("two_apart")
    v = v.copy()
    v[1], v[2, 0] = np.nan, np.inf                                          # both in component 0
    cc = ngp_hip.components(_mesh(v, f))
    assert np.array_equal(_np(cc.vertex_component), lab["vertex_component"]) and np.array_equal(_np(cc.face_component), lab["face_component"])
    for name in R.INT_FIELDS:
        assert np.array_equal(_np(getattr(cc.stats, name)), tab[name]), name
    assert abs(float(cc.stats.area[1]) - tab["area"][1]) <= tab["area_bound"][1]           # the other component's floats are its own
    assert np.array_equal(_bits(cc.stats.lo[1]), tab["lo"][1].view(np.int32))


def test_the_round_cap_raises():
    """The host loop's cap is a condition: with a cap below the rounds a mesh needs (never the case for the default, V) it raises."""
    from ngp_hip import ops
    v, f = R.fan(100)
    faces = _mesh(v, f).faces
    assert ops.mesh_components_label(faces, len(v))[3] == 2
    with pytest.raises(RuntimeError, match="rounds"):
        ops.mesh_components_label(faces, len(v), max_rounds=1)
    assert ops.mesh_components_label(faces, len(v), max_rounds=2)[3] == 2


# ---- invariance and determinism --------------------------------------------------------------------------------------------------------------
def test_face_order_and_vertex_names_do_not_matter():
    import ngp_hip
    (v, f), _ = R.sphere_and_floaters(60)
    base = _check(v, f, what="sphere and floaters")
    rng = np.random.default_rng(9)
    perm = rng.permutation(len(f))
    cc = ngp_hip.components(_mesh(v, f[perm]))
    assert cc.n == base.n and np.array_equal(_np(cc.vertex_component), _np(base.vertex_component))
    assert np.array_equal(_np(cc.face_component), _np(base.face_component)[perm])
    tab = R.table(v, f, R.label(f, len(v)))
    for name in R.INT_FIELDS + ("lo", "hi"):
        assert np.array_equal(_bits(getattr(cc.stats, name)), _bits(getattr(base.stats, name))), name
    for name in ("area", "volume"):
        assert (np.abs(_np(getattr(cc.stats, name)) - tab[name]) <= tab[name + "_bound"]).all()
    names = rng.permutation(len(v))                                                          # vertex i is now called names[i]
    v2, f2 = R.renumber(v, f, names)
    cc2 = _check(v2, f2, what="renamed")
    pairs = np.unique(np.stack([_np(base.vertex_component), _np(cc2.vertex_component)[names]], 1), axis=0)
    assert len(pairs) == base.n and len(np.unique(pairs[:, 0])) == base.n and len(np.unique(pairs[:, 1])) == base.n     # a bijection


def test_two_runs_write_the_same_bytes():
    import ngp_hip
    v, f = R.join(M.extracted_torus(), M.soup(500, 11), R.strip(5000, "random", seed=2))
    m = _mesh(v, f, normals=np.random.default_rng(1).normal(size=v.shape).astype(np.float32))
    runs = []
    for _ in range(2):
        cc = ngp_hip.components(m)
        keep = torch.arange(cc.n) % 3 != 1
        out, vmap, fmap = ngp_hip.select_components(m, cc, keep)
        runs.append([cc.vertex_component, cc.face_component, *cc.stats, out.vertices, out.faces, out.normals, vmap, fmap])
    assert len(runs[0]) == 17
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ---- selection -------------------------------------------------------------------------------------------------------------------------------
def test_selection_equals_the_reference():
    import ngp_hip
    from ngp_hip import mesh
    v, f, lab, tab = R.case("icospheres4")
    normals = np.random.default_rng(4).normal(size=v.shape).astype(np.float32)
    m = _mesh(v, f, normals)
    cc = ngp_hip.components(m)
    for keep in ([True, False, True, False], [False, False, False, True], [True] * 4, [False] * 4):
        for device in ("cpu", DEV):
            out, vmap, fmap = ngp_hip.select_components(m, cc, torch.tensor(keep, device=device))
            want = R.select(v, normals, f, lab, keep)
            assert vmap.dtype == torch.int32 and fmap.dtype == torch.int32 and out.faces.dtype == torch.int32
            assert np.array_equal(_bits(out.vertices), want["vertices"].view(np.int32)) and np.array_equal(_bits(out.normals), want["normals"].view(np.int32))
            assert np.array_equal(_np(out.faces), want["faces"]) and np.array_equal(_np(vmap), want["vertex_map"]) and np.array_equal(_np(fmap), want["face_map"])
            assert out.vertices.shape == (sum(k * n for k, n in zip(keep, tab["vertices"])), 3)
        again = ngp_hip.components(out)
        assert again.n == sum(keep) and again.unused_vertices == 0
        kept = np.array(keep)
        top = mesh.topology(out)
        assert top == {"vertices": int(tab["vertices"][kept].sum()), "faces": int(tab["faces"][kept].sum()),
                       "euler": int(tab["euler"][kept].sum()), "boundary_edges": int(tab["boundary_edges"][kept].sum())}
    all_of_it, _, _ = ngp_hip.select_components(m, cc, torch.ones(4, dtype=torch.bool))
    assert np.array_equal(_bits(all_of_it.vertices), v.view(np.int32)) and np.array_equal(_np(all_of_it.faces), f)
    none, vmap, fmap = ngp_hip.select_components(_mesh(v, f), cc, torch.zeros(4, dtype=torch.bool))
    assert none.vertices.shape == (0, 3) and none.faces.shape == (0, 3) and none.normals is None and (vmap == -1).all() and (fmap == -1).all()
    with pytest.raises(ValueError, match="keep"):
        ngp_hip.select_components(m, cc, torch.ones(3, dtype=torch.bool))


def test_selection_drops_bad_faces_and_unused_vertices():
    import ngp_hip
    v, f = R.two_tetrahedra_apart()
    v = np.concatenate([np.ones((1, 3), np.float32), v])                                     # vertex 0 is unused
    f = np.concatenate([f + 1, [[1, 2, 99]]]).astype(np.int32)
    m = _mesh(v, f)
    cc = ngp_hip.components(m, strict=False)
    out, vmap, fmap = ngp_hip.select_components(m, cc, torch.ones(2, dtype=torch.bool))
    want = R.select(v, None, f, R.label(f, len(v)), [True, True])
    assert np.array_equal(_np(out.faces), want["faces"]) and np.array_equal(_bits(out.vertices), want["vertices"].view(np.int32))
    assert _np(vmap).tolist() == [-1] + list(range(8)) and _np(fmap).tolist() == list(range(8)) + [-1]


# ---- clean_mesh ------------------------------------------------------------------------------------------------------------------------------
def test_clean_mesh_defaults_are_the_identity_on_a_clean_mesh():
    import ngp_hip
    v, f, lab, tab = R.case("torus")
    out, report = ngp_hip.clean_mesh(_mesh(v, f))
    assert np.array_equal(_bits(out.vertices), v.view(np.int32)) and np.array_equal(_np(out.faces), f)
    assert report["components_kept"] == 1 and report["components_dropped"] == 0 and report["faces_kept"] == len(f) and report["faces_dropped"] == 0
    assert report["bad_faces"] == 0 and report["unused_vertices"] == 0 and report["area_dropped"] == 0.0


def test_clean_mesh_keeps_the_sphere():
    import ngp_hip
    (v, f), n_floaters = R.sphere_and_floaters(200)
    assert n_floaters == 200
    lab = R.label(f, len(v))
    tab = R.table(v, f, lab)
    out, report = ngp_hip.clean_mesh(_mesh(v, f), keep_largest=1)
    sphere = int(np.argmax(tab["faces"]))
    assert tab["faces"][sphere] == 320 and report["kept"] == [sphere]
    want = R.select(v, None, f, lab, np.arange(lab["n"]) == sphere)
    assert np.array_equal(_bits(out.vertices), want["vertices"].view(np.int32)) and np.array_equal(_np(out.faces), want["faces"])
    assert report["components_kept"] + report["components_dropped"] == lab["n"] == 201
    assert report["faces_kept"] == 320 and report["faces_dropped"] == 800 and report["faces_kept"] + report["faces_dropped"] == len(f)
    assert abs(report["area_kept"] + report["area_dropped"] - tab["area"].sum()) <= tab["area_bound"].sum() + 1e-15 * tab["area"].sum()
    small, report = ngp_hip.clean_mesh(_mesh(v, f), min_faces=5)
    assert report["kept"] == [sphere] and small.faces.shape[0] == 320
    frac, report = ngp_hip.clean_mesh(_mesh(v, f), min_area_fraction=0.5)
    assert report["kept"] == [sphere]


def test_example_cleans_before_it_writes(tmp_path, capsys):
    """examples/extract_mesh.py --keep_largest 1 --min_component_faces 4 on the small sphere fit of tests/test_gpu_mesh.py: the file
    holds one component, and the report and both topologies are printed."""
    import importlib.util
    import os
    import ngp_hip
    from conftest import ROOT
    from ngp_hip import mesh
    spec = importlib.util.spec_from_file_location("extract_mesh_example", os.path.join(ROOT, "examples", "extract_mesh.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = str(tmp_path / "sphere.ply")
    info = ex.main(["--sdf", "--steps", "300", "--n", "4096", "--log2_T", "14", "--levels", "8", "--max_res", "128", "--resolution", "48",
                    "--out", out, "--keep_largest", "1", "--min_component_faces", "4"])
    clean, printed = info["clean"], capsys.readouterr().out
    assert clean["components_kept"] == 1 and clean["faces_kept"] == info["faces"] and clean["before"]["faces"] == clean["faces_kept"] + clean["faces_dropped"]
    assert "clean_mesh:" in printed and "topology before:" in printed and '"euler"' in printed
    written = mesh.read_ply(out)
    assert written.faces.shape[0] == info["faces"] and written.vertices.shape[0] == info["vertices"]
    assert ngp_hip.components(mesh.Mesh(written.vertices.to(DEV), written.faces.to(DEV), None)).n == 1


@pytest.mark.parametrize("kw", [{"keep_largest": 1, "by": "area"}, {"keep_largest": 1, "by": "volume"}, {"keep_largest": 1, "by": "faces"},
                                {"keep_largest": 2, "by": "faces"}, {"closed_only": True}, {"keep_largest": 0}])
def test_clean_mesh_picks_what_the_reference_picks(kw):
    import ngp_hip
    v, f, lab, tab = R.case("three_rankings")
    out, report = ngp_hip.clean_mesh(_mesh(v, f), **kw)
    keep = R.rule(tab, **kw)
    assert report["kept"] == np.flatnonzero(keep).tolist()
    assert np.array_equal(_np(out.faces), R.select(v, None, f, lab, keep)["faces"])
    assert report["faces_kept"] == int(tab["faces"][keep].sum()) and report["components_dropped"] == int((~keep).sum())
