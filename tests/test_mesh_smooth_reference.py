"""The serial reference of the smoothing contract (tests/mesh_smooth_reference.py) pinned by itself: hand-derived known answers, a
brute-force adjacency, invariances, the displacement bound and the behaviour Taubin's scheme is chosen for.  No GPU."""
import numpy as np

import mesh_smooth_reference as R


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_octahedron_scales_by_three_quarters_per_iteration():
    """lam = 0.5, mu = -0.5, every vertex free: the neighbour mean of +-e_k is 0 (the serial sum a + (-a) + 0 + 0 is exact), so the lam
    pass halves the vertex and the mu pass multiplies it by 1.5.  3^n / 4^n is a float32 for n <= 15: the answer is exact."""
    v, f = R.octahedron()
    for n in (1, 2, 5, 10, 15):
        out = R.smooth(v, f, iterations=n, lam=0.5, mu=-0.5, boundary="free")["vertices"]
        assert np.array_equal(_bits(out), _bits(v * np.float32(0.75 ** n))), n
        assert out.dtype == np.float32 and np.float32(0.75 ** n) == 0.75 ** n
    assert np.array_equal(_bits(R.smooth(v, f, iterations=0)["vertices"]), _bits(v))
    assert R.smooth(v, f, iterations=3, mu=0.0)["passes"] == 3 and R.smooth(v, f, iterations=3)["passes"] == 6


def test_dyadic_patch_is_a_fixed_point():
    """Six neighbours placed symmetrically: their sum is exactly 6 x, the mean exactly x, the update exactly 0.  With the boundary fixed
    no vertex changes a bit, whatever the number of iterations; with a free boundary the corners (and the whole rim) move inwards."""
    v, f = R.dyadic_patch(8)
    adj = R.adjacency(v, f)
    assert adj["counts"] == (2 * (3 * 64 + 16), 0, 0, 32)                          # E = 3 k^2 + 2 k undirected edges, 4 k rim vertices
    for n in (1, 7, 30):
        assert np.array_equal(_bits(R.smooth(v, f, iterations=n, boundary="fixed", adj=adj)["vertices"]), _bits(v))
    free = R.smooth(v, f, iterations=1, mu=0.0, boundary="free", adj=adj)["vertices"]
    corners = [0, 8, 72, 80]
    assert (free[corners] != v[corners]).any(1).all()
    interior = (adj["vertex_flags"] & R.BOUNDARY) == 0
    two_in = np.array([[i, j] for i in range(9) for j in range(9)])
    deep = ((two_in >= 2) & (two_in <= 6)).all(1)                                  # their neighbours did not move in one pass
    assert interior.sum() == 49 and np.array_equal(_bits(free[deep]), _bits(v[deep]))


def test_adjacency_equals_the_brute_force_construction_on_a_messy_mesh():
    v, f = R.messy()
    a, b = R.adjacency(v, f), R.brute_force_adjacency(v, f)
    for k in ("row_start", "neighbours", "multiplicity", "vertex_flags"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert a["counts"] == b["counts"]
    e2, bad_faces, bad_vertices, boundary = a["counts"]
    assert (bad_faces, bad_vertices) == (6, 1) and e2 == len(a["neighbours"]) == a["row_start"][-1]
    flags = a["vertex_flags"]
    assert flags[10] == R.UNUSED and flags[11] & R.BAD and not flags[11] & R.UNUSED
    assert boundary == int(((flags & R.BOUNDARY) != 0).sum()) > 0

    def mult(u, w):
        row = slice(a["row_start"][u], a["row_start"][u + 1])
        return int(a["multiplicity"][row][list(a["neighbours"][row]).index(w)])
    assert mult(0, 1) == mult(1, 0) == 5 and flags[0] & R.NONMANIFOLD             # three copies, (0,1,4) and (1,0,5)
    assert mult(0, 2) == 3 and mult(2, 3) == 2 and mult(1, 3) == 2                 # the duplicates; the face in both orientations
    assert mult(7, 8) == 1 and flags[7] & R.BOUNDARY
    for u in range(len(v)):                                                        # rows: distinct, ascending
        row = a["neighbours"][a["row_start"][u]:a["row_start"][u + 1]]
        assert (np.diff(row) > 0).all()
    sat = R.adjacency(*R.messy(duplicates=300))
    assert sat["multiplicity"].max() == R.MAX_MULTIPLICITY == 255
    assert np.array_equal(sat["multiplicity"], R.brute_force_adjacency(*R.messy(duplicates=300))["multiplicity"])


def test_result_does_not_depend_on_face_order_or_corner_rotation():
    rng = np.random.default_rng(2)
    for name in ("noisy_icosphere", "cylinder"):
        v, f, adj = R.case(name)
        g = np.stack([np.roll(t, k) for t, k in zip(f[rng.permutation(len(f))], rng.integers(0, 3, len(f)))]).astype(np.int32)
        adj2 = R.adjacency(v, g)
        for k in ("row_start", "neighbours", "multiplicity", "vertex_flags"):
            assert np.array_equal(adj[k], adj2[k]), k
        for mode in R.MODES:
            a = R.smooth(v, f, iterations=4, boundary=mode, max_move=0.01)["vertices"]
            b = R.smooth(v, g, iterations=4, boundary=mode, max_move=0.01)["vertices"]
            assert np.array_equal(_bits(a), _bits(b)), (name, mode)


def test_max_move_bounds_the_displacement_from_the_original_exactly():
    v, f = R.noisy_icosphere(3, amplitude=0.01)
    for mm in (0.004, (0.002, 0.004, 0.0)):
        out = R.smooth(v, f, iterations=50, max_move=mm)["vertices"]
        share = R.max_move_holds(out, v, mm)
        print("max_move %r: %.1f %% of the coordinates sit on the bound after 50 iterations" % (mm, 100 * share))
        assert share > 0.02
    assert np.array_equal(_bits(R.smooth(v, f, iterations=50, max_move=(0.002, 0.004, 0.0))["vertices"][:, 2]), _bits(v[:, 2]))
    free = R.smooth(v, f, iterations=50)["vertices"]
    assert np.abs(free - v).max() > 0.004                                          # without the bound the vertices do go farther


def test_taubin_smooths_without_the_shrinkage_of_the_laplacian():
    """Inequalities between runs of the reference on an icosphere (642 vertices, radius 0.35) with radial noise of sigma 0.01, n = 10."""
    centre, radius, n = (0.5, 0.5, 0.5), 0.35, 10
    v, f = R.noisy_icosphere(3, amplitude=0.01)
    rms0, vol0 = R.radial_rms(v, centre, radius), R.volume(v, f)
    taubin = R.smooth(v, f, iterations=n)["vertices"]
    rms_t, vol_t = R.radial_rms(taubin, centre, radius), R.volume(taubin, f)
    vols = [R.volume(R.smooth(v, f, iterations=k, mu=0.0)["vertices"], f) for k in range(1, 2 * n + 1)]
    print("rms radial deviation %.5f -> %.5f (Taubin, %d iterations); volume %.6f -> %.6f (Taubin) / %.6f (%d Laplacian passes)"
          % (rms0, rms_t, n, vol0, vol_t, vols[-1], 2 * n))
    assert rms_t < 0.5 * rms0
    assert abs(vol_t - vol0) < 0.25 * abs(vols[-1] - vol0)
    assert all(b < a for a, b in zip([vol0] + vols, vols))
    assert abs(R.taubin_mu(0.5) - 1.0 / (0.1 - 2.0)) < 1e-15 and R.taubin_mu(0.5) < -0.5


def ring_measures(vertices, n_around=48, n_along=12):
    """Per boundary ring (first, last): mean z, the spread of z, the spread of the distance from the axis."""
    out = []
    for r in (0, n_along):
        ring = np.asarray(vertices, np.float64)[r * n_around:(r + 1) * n_around]
        out.append((ring[:, 2].mean(), ring[:, 2].std(), np.hypot(ring[:, 0], ring[:, 1]).std()))
    return out


def test_curve_mode_smooths_a_boundary_along_itself():
    """An open cylinder with noise on every coordinate.  In "curve" mode a boundary vertex sees its two boundary neighbours only, and
    the mean of a closed ring is invariant under such a pass in exact arithmetic; every pass rounds every coordinate to float32, by
    half a spacing of the ring's z at most.  So the rings' mean z moves by no more than passes x spacing(length) / 2 -- that is the
    tolerance, from the arithmetic of the run and nothing else -- while their z and radius noise shrinks.  "free" slides them inwards."""
    v, f, _ = R.open_cylinder()
    n = 10
    curve = R.smooth(v, f, iterations=n, boundary="curve")
    tol = curve["passes"] * 0.5 * float(np.spacing(np.float32(1.0)))
    before, after = ring_measures(v), ring_measures(curve["vertices"])
    free = ring_measures(R.smooth(v, f, iterations=n, mu=0.0, boundary="free")["vertices"])
    fixed = R.smooth(v, f, iterations=n, boundary="fixed")["vertices"]
    for (z0, sz0, sr0), (z1, sz1, sr1), (zf, _, _) in zip(before, after, free):
        print("ring: mean z %.6f -> %.6f (tolerance %.2g; free: %.6f), z spread %.5f -> %.5f, radius spread %.5f -> %.5f"
              % (z0, z1, tol, zf, sz0, sz1, sr0, sr1))
        assert abs(z1 - z0) <= tol
        assert sz1 < 0.75 * sz0 and sr1 < 0.75 * sr0               # white noise on 48 points: Taubin keeps its low frequencies
        assert abs(zf - z0) > 100 * tol
    rim = (curve["adjacency"]["vertex_flags"] & R.BOUNDARY) != 0
    assert rim.sum() == 96 and np.array_equal(_bits(fixed[rim]), _bits(v[rim])) and (curve["vertices"][rim] != v[rim]).any()


def test_bad_vertices_stay_and_are_left_out():
    v, f = R.noisy_icosphere(2)
    v = v.copy()
    v[5, 1], v[40, 0] = np.nan, np.inf
    adj = R.adjacency(v, f)
    assert adj["counts"][2] == 2
    out = R.smooth(v, f, iterations=3, adj=adj)["vertices"]
    assert np.array_equal(_bits(out[[5, 40]]), _bits(v[[5, 40]]))
    good = np.isfinite(v).all(1)
    assert np.isfinite(out[good]).all() and (out[good] != v[good]).any()
    pinned = np.zeros(len(v), np.uint8)
    pinned[:20] = 1
    out = R.smooth(v, f, iterations=3, fixed=pinned, adj=adj)["vertices"]
    assert np.array_equal(_bits(out[:20]), _bits(v[:20]))


def test_vertex_normals():
    """Outward unit normals on a sphere (area weights: within the facet angle of the radial direction), exact zeros where the area
    vectors cancel, where a face has a vertex that is not finite, and on an unused vertex; the bound is a few float32 roundings."""
    v, f = R.case("icosphere")[:2]
    n, bound = R.vertex_normals(v, f)
    radial = v.astype(np.float64) - 0.5
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert n.dtype == np.float32 and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 2e-7
    assert (np.einsum("ij,ij->i", n, radial) > 0.999).all() and bound.max() < 4 * 2.0**-24
    n, _ = R.vertex_normals(*R.cancelling())
    assert np.array_equal(n[0], np.zeros(3, np.float32)) and np.abs(n[3] - [0, 0, 1]).max() == 0
    v, f = R.messy()
    n, _ = R.vertex_normals(v, f)
    assert not n[10].any() and not n[11].any() and not n[5].any() and np.isfinite(n).all() and n[7].any()
    g = np.roll(f, 1, axis=1)                                                      # a rotation keeps the area vector up to rounding
    assert np.abs(R.vertex_normals(v, g)[0] - n).max() <= 2.0**-22
