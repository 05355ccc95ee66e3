"""The numpy reference of the vertex-colour contract (tests/mesh_color_reference.py) against closed forms, and the condition on the named
sets that the GPU tests use: at most MAX_UNDECIDED of their (vertex, camera) pairs are undecided.  No GPU, no package."""
import numpy as np
import pytest

import mesh_color_reference as R

F32, F64 = np.float32, np.float64


def _axis_camera(width=8, height=8, focal=16.0):
    """A camera at the origin looking along +z, right = +x, down = +y: u = focal x / z + W / 2."""
    c2w = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]], F32)
    return R.intrinsics(width, height, focal), c2w


def _towards_origin(v):
    v = np.asarray(v, F64)
    return (-v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


@pytest.mark.parametrize("T", [F32, F64])
def test_constant_images_give_the_cos2_weighted_mean(T):
    """Every view a constant colour c_n: the result is sum cos^2 c_n / sum cos^2 over the views that count -- bit for bit in the float32
    restatement (dyadic colours: the bilinear mean of a constant is exact there), to the rounding of f64 in the float64 contract."""
    case = R.case("convex")
    consts = np.array([[0.25, 0.5, 0.75], [1.0, 0.125, 0.5], [0.5, 0.5, 0.5], [0.75, 0.25, 1.0], [0.0, 1.0, 0.25], [0.375, 0.625, 0.875]], F32)
    images = np.broadcast_to(consts[:, None, None, :], (6, 32, 32, 3)).copy()
    out = R.bake(case.vertices, case.faces, case.normals, images, case.K, case.c2w, case.eps, T=T)
    cos, counts = out["project"]["cos"], out["counts"]
    assert counts.any(0).sum() > 100 and (counts.sum(0) >= 2).sum() > 50
    num, den = np.zeros((len(case.vertices), 3)), np.zeros(len(case.vertices))
    for j in range(6):                                                           # the same serial order
        w = np.where(counts[j], (cos[j] * cos[j]).astype(F64), 0.0)
        num += w[:, None] * consts[j].astype(F64)
        den += w
    seen = den > 0
    want = num[seen] / den[seen, None]
    assert np.array_equal(out["views"], counts.sum(0)) and np.array_equal(seen, out["views"] > 0)
    if T is F32:
        assert np.array_equal(out["colors"][seen], want.astype(F32)) and np.array_equal(out["weight"][seen], den[seen].astype(F32))
    else:
        assert np.allclose(out["colors"][seen], want, rtol=1e-14, atol=0) and np.array_equal(out["weight"][seen], den[seen])
    assert not out["colors"][~seen].any() and (out["filled"][~seen] == R.UNCOLOURED).all() and not out["filled"][seen].any()


def test_best_picks_the_view_with_the_largest_cos():
    for name in ("best", "tie"):
        case = R.case(name)
        r = case.ref()["r64"]
        cos = np.where(r["counts"], r["project"]["cos"], -np.inf)
        seen = r["counts"].any(0)
        assert seen.sum() >= 6 and np.array_equal(r["winner"][seen], cos.argmax(0)[seen]) and (r["winner"][~seen] == -1).all()   # argmax: the first
        assert (r["views"][seen] == 1).all()
        w = np.take_along_axis(r["project"]["weight"], np.maximum(r["winner"], 0)[None], 0)[0]
        assert np.array_equal(r["weight"][seen], w[seen])
    # the tie: the middle column sees both cameras under the same cos, bit for bit, in both arithmetics, and camera 0 stays
    case = R.case("tie")
    for key in ("r32", "r64"):
        r = case.ref()[key]
        cos = r["project"]["cos"]
        middle = np.flatnonzero(case.vertices[:, 0] == 0.5)
        assert len(middle) == 3 and r["counts"][:, middle].all() and np.array_equal(cos[0, middle], cos[1, middle])
        assert (r["winner"][middle] == 0).all()
        left = case.vertices[:, 0] < 0.5
        assert (r["winner"][left] == 0).all() and (r["winner"][case.vertices[:, 0] > 0.5] == 1).all()


@pytest.mark.parametrize("T", [F32, F64])
def test_behind_outside_and_on_the_border(T):
    """W = H = 8, focal 16, the camera at the origin along +z: a = 16 x / z + 3.5.  x = -3.5, z = 16 is the centre of column 0 exactly
    (the border, inside), x = 3.5 that of column 7; a hair beyond either is outside; z < 0 is behind whatever the rest says."""
    K, c2w = _axis_camera()
    v = np.array([[-3.5, 0, 16], [3.5, 0, 16], [0, -3.5, 16], [0, 3.5, 16],            # on the four borders
                  [-3.5009766, 0, 16], [3.5009766, 0, 16], [0, -3.5009766, 16], [0, 3.5009766, 16],      # just outside
                  [0.5, 0.25, -16], [0, 0, 16], [1, 1, 16]], F32)                       # behind; the centre; inside
    n = _towards_origin(v)
    images = R.smooth_images(1, 8, 8)
    p = R.project(v, n, K, c2w, (8, 8), 1e-3, T=T)
    assert p["cos_ok"].all() and np.array_equal(p["depth_ok"][0], v[:, 2] > 0)
    assert np.array_equal(p["frame_ok"][0], [1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1])          # the mirror image of a point behind lies in the frame
    assert np.array_equal(p["accept"][0], [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1])
    assert np.array_equal(p["a"][0, :4], [0, 7, 3.5, 3.5]) and np.array_equal(p["b"][0, :4], [3.5, 3.5, 0, 7])
    out = R.bake(v, np.zeros((0, 3), np.int32), n, images, K, c2w, 1e-3, T=T)
    assert np.array_equal(out["views"], p["accept"][0].astype(np.int32))
    img = images[0].astype(F64)
    want = [0.5 * (img[3, 0] + img[4, 0]), 0.5 * (img[3, 7] + img[4, 7]), 0.5 * (img[0, 3] + img[0, 4]), 0.5 * (img[7, 3] + img[7, 4])]
    assert np.allclose(out["colors"][:4], want, rtol=1e-7 if T is F32 else 4e-15, atol=0)      # the border texel itself, its neighbour clamped
    assert np.allclose(out["colors"][9], 0.25 * (img[3, 3] + img[3, 4] + img[4, 3] + img[4, 4]), rtol=1e-7, atol=0)
    # a normal turned away fails the cos test alone; two_sided turns it back
    away = R.project(v[9:], -n[9:], K, c2w, (8, 8), 1e-3, T=T)
    assert not away["cos_ok"].any() and away["depth_ok"].all() and away["frame_ok"].all() and not away["weight"].any()
    back = R.project(v[9:], -n[9:], K, c2w, (8, 8), 1e-3, two_sided=True, T=T)
    front = R.project(v[9:], n[9:], K, c2w, (8, 8), 1e-3, T=T)
    assert back["accept"].all() and all(np.array_equal(back[k], front[k]) for k in ("cos", "a", "b", "weight", "o", "d"))
    # a vertex or a normal that is not finite rejects its pairs and nobody else's
    bad_v, bad_n = v.copy(), n.copy()
    bad_v[9, 1], bad_n[10, 0] = np.nan, np.inf
    q = R.project(bad_v, bad_n, K, c2w, (8, 8), 1e-3, T=T)
    assert np.array_equal(q["accept"][0], [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]) and np.array_equal(q["a"][0, :9], p["a"][0, :9])
    assert np.isfinite(q["o"]).all() and np.isfinite(q["d"]).all()


def test_occluder_views():
    """The far square's four vertices behind the near one are seen by camera B alone, its other five by both."""
    case = R.case("occluder")
    r = case.ref()["r64"]
    far = case.vertices[:9]
    covered = (far[:, 0] >= 0.5) & (far[:, 1] >= 0.5)
    assert covered.sum() == 4 and r["project"]["accept"][:, :9].all()
    assert np.array_equal(r["occluded"][0, :9], covered) and not r["occluded"][1, :9].any()
    assert np.array_equal(r["views"][:9], np.where(covered, 1, 2))
    assert np.array_equal(case.ref()["r32"]["views"], r["views"])


def test_fill_goes_ring_by_ring():
    """A strip of 6 columns, the first column coloured: round r colours column r with the mean of what column r - 1 and, within the
    column, nobody yet holds; after 3 rounds columns 4 and 5 still have the default."""
    cols = 6
    v = np.array([[i, j, 0] for i in range(cols) for j in range(2)], F32)
    f = np.array([t for i in range(cols - 1) for t in ((2 * i, 2 * i + 2, 2 * i + 3), (2 * i, 2 * i + 3, 2 * i + 1))], np.int32)
    assert R.neighbours(f, len(v))[0] == [1, 2, 3] and R.neighbours(f, len(v))[3] == [0, 1, 2, 5]
    colors = np.zeros((len(v), 3), F32)
    colors[0], colors[1] = (0.25, 0.5, 1.0), (0.75, 0.5, 0.0)
    filled = np.full(len(v), R.UNCOLOURED, np.uint8)
    filled[:2] = 0
    out, state = R.fill(colors, filled, f, 3)
    assert state.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 255, 255, 255, 255]
    assert np.array_equal(out[2], colors[0]) and np.array_equal(out[3], np.array([0.5, 0.5, 0.5], F32))      # 2 sees 0 only; 3 sees 0 and 1
    assert np.array_equal(out[4], out[2]) and np.array_equal(out[5], ((out[2].astype(F64) + out[3]) / 2).astype(F32))
    assert np.array_equal(out[8:], np.full((4, 3), 0.5, F32)) and np.array_equal(out[:2], colors[:2])
    none, state0 = R.fill(colors, filled, f, 0, default=(0.1, 0.2, 0.3))
    assert state0.tolist() == filled.tolist() and np.array_equal(none[2:], np.tile(np.array([0.1, 0.2, 0.3], F32), (10, 1)))
    full, state_all = R.fill(colors, filled, f, 8)
    assert state_all.max() == 5 and np.array_equal(full[:8], out[:8])
    # a face with a repeated or a wild index joins nothing
    assert R.neighbours(np.array([[0, 0, 1], [0, 1, 99], [-1, 0, 1]]), 3) == [[], [], []]


@pytest.mark.parametrize("name", R.SETS)
def test_named_sets_stay_decided(name):
    """The condition on the sets of tests/test_gpu_mesh_color.py: the float64 contract and the float32 restatement disagree on at most
    MAX_UNDECIDED of the pairs (the project's cap, as tests/test_gpu_sdf_trace.py), and the set exercises what its name says."""
    case = R.case(name)
    ref = case.ref()
    share = case.undecided_fraction()
    views = ref["r64"]["views"]
    print("%s: %d pairs, %.2f %% undecided, %d of %d vertices decided, %d with a view; E32 colour %.3g, weight %.3g"
          % (name, ref["decided_pairs"].size, 100 * share, int(ref["decided"].sum()), len(views), int((views > 0).sum()), ref["e32_c"], ref["e32_w"]))
    assert share <= R.MAX_UNDECIDED
    assert ref["e32_c"] < 1e-4 and ref["e32_w"] < 1e-4                           # a float32 restatement, not another computation
    if name == "flipped_one_sided":
        assert not views.any()
    elif name == "cap":
        assert 10 <= (views == 0).sum() <= len(views) - 50
    elif name == "v1":
        assert len(views) == 1 and case.faces.shape == (0, 3)
    else:
        assert (views > 0).sum() >= min(len(views), 9) // 2
    if name == "flipped":
        assert np.array_equal(ref["r64"]["colors"], R.case("convex").ref()["r64"]["colors"])


def test_closed_loop_images_show_the_function():
    """The closed loop's images: a hit pixel holds linear_colour at a point of the mesh (inside the sphere's shell), a miss the background."""
    case = R.case("closed_loop")
    images, masks = R.closed_loop_images(case.vertices, case.faces, case.K, case.c2w[:1], R.WH, background=-1.0)
    assert 0.3 < masks.mean() < 0.8 and (images[~masks] == -1.0).all() and (images[masks] > 0).all() and (images[masks] < 1.1).all()
    assert masks[0, 16, 16] and not masks[0, 0, 0]
