"""Float64 model of the two ray-gradient reductions of csrc/ray_grad.hip, their serial float32 evaluation, a float32 evaluation in
the kernels' own order, and the inputs both test files use (tests/test_ray_grad_reference.py on the CPU, tests/test_gpu_ray_grad.py on
the GPU).  numpy only: no GPU, no oracle.

The contracts:

    march:  row m of rays_a = (ray, start, N);  d_o[ray] = sum_{j<N} dx[start+j];  d_d[ray] = sum_{j<N} ((t[start+j] dx[start+j]) + dd[start+j])
    poses:  d_poses[i][r][c] = sum_{k: img(k)=i} g_d[k][r] dir[pix(k)][c] (c < 3);  d_poses[i][r][3] = sum_{k: img(k)=i} g_o[k][r]

Each has three evaluations: float64 (*_64, which also returns S, the same sum over the absolute values of its terms), a serial float32
one in sample / ray order (*_serial32: every rounding is one numpy float32 operation, multiply and add separate, as the library is built
with -ffp-contract=off) and the kernel's order (*_wave32: per-lane strided partial sums, then the xor butterfly; for the poses 256
thread-strided partials, a butterfly per wave and (w0 + w1) + (w2 + w3)).

The yardstick is the project's (tests/composite_reference.py): E32 = max |serial32 - f64| / S over the elements of one input, and a
result passes element by element when |got - f64| <= K E32 S + TINY."""
import numpy as np

F = np.float32
K = 4
TINY = 1e-30
WAVE = 64
POSE_THREADS = 256
SENTINEL = -7.0
EDGE_N = (0, 1, 2, 63, 64, 65, 127, 128, 129, 500, 1024)


# ------------------------------------------------------------------------------------------------------------------ inputs
def ray_input(seed=7, permute=False):
    """The ray batch of the GPU test: one ray of every EDGE_N length plus 150 rays with N in [1, 400), packed in ray order behind a
    64-sample sentinel gap; d_xyzs ~ N(0,1), d_dirs ~ 0.1 N(0,1), ts ascending in [0.05, 1.7] along each ray.  permute: the rays_a rows
    in a seeded random order (results are indexed by ray_idx, so they do not change)."""
    rng = np.random.default_rng(seed)
    N = np.concatenate([np.asarray(EDGE_N, np.int64), rng.integers(1, 400, 150)])
    order = rng.permutation(len(N))                      # which ray_idx each packed range belongs to
    start = 64 + np.concatenate([[0], np.cumsum(N)[:-1]])
    S = int(64 + N.sum() + 64)
    rays_a = np.stack([order, start, N], 1).astype(np.int32)
    ts = np.full(S, np.nan, F)
    for s, n in zip(start, N):
        ts[s:s + n] = np.sort(rng.uniform(0.05, 1.7, n)).astype(F)
    d_xyzs = rng.standard_normal((S, 3)).astype(F)
    d_dirs = (0.1 * rng.standard_normal((S, 3))).astype(F)
    if permute:
        rays_a = rays_a[np.random.default_rng(seed + 1).permutation(len(N))]
    return dict(rays_a=np.ascontiguousarray(rays_a), ts=ts, d_xyzs=d_xyzs, d_dirs=d_dirs, n=len(N), S=S)


def pose_input(n, n_img, seed=11, hw=4096):
    """n rays over n_img images (with n_img == 3 image 1 receives none), pixels into hw directions of a pinhole camera, N(0,1) ray
    gradients."""
    rng = np.random.default_rng(seed + 1000 * n + n_img)
    img = rng.integers(0, n_img, n).astype(np.int64)
    if n_img == 3:
        img[img == 1] = 2 * rng.integers(0, 2, int((img == 1).sum()))
    pix = rng.integers(0, hw, n).astype(np.int64)
    u = rng.uniform(-0.36, 0.36, (max(hw, n), 2))
    directions = np.concatenate([u, np.ones((len(u), 1))], 1).astype(F)
    return dict(directions=directions, img=img, pix=pix, g_o=rng.standard_normal((n, 3)).astype(F),
                g_d=rng.standard_normal((n, 3)).astype(F), n=n, n_img=n_img)


# ------------------------------------------------------------------------------------------------------------------ march
def _padded(inp, dtype):
    """Per rays_a row: [m, L, .] arrays of its samples (zeros behind N), L = max N."""
    ra = inp["rays_a"].astype(np.int64)
    L = int(max(ra[:, 2].max(initial=0), 1))
    j = np.arange(L)[None, :]
    valid = j < ra[:, 2:3]
    idx = np.where(valid, ra[:, 1:2] + j, 0)
    dx = inp["d_xyzs"] if inp.get("d_xyzs") is not None else np.zeros((inp["S"], 3), F)
    dd = inp["d_dirs"] if inp.get("d_dirs") is not None else np.zeros((inp["S"], 3), F)
    t = np.where(valid, np.nan_to_num(inp["ts"][idx]), 0).astype(dtype)
    return ra, valid, t, np.where(valid[..., None], dx[idx], 0).astype(dtype), np.where(valid[..., None], dd[idx], 0).astype(dtype)


def _by_ray(ra, n, *rows):
    out = []
    for r in rows:
        o = np.zeros((n, 3), r.dtype)
        o[ra[:, 0]] = r
        out.append(o)
    return out


def march_bwd_64(inp):
    """-> d_rays_o, d_rays_d, S_o, S_d: [n,3] float64, indexed by ray_idx."""
    ra, _, t, dx, dd = _padded(inp, np.float64)
    term = t[..., None] * dx + dd
    return _by_ray(ra, inp["n"], dx.sum(1), term.sum(1), np.abs(dx).sum(1), (np.abs(t[..., None] * dx) + np.abs(dd)).sum(1))


def march_bwd_serial32(inp):
    ra, valid, t, dx, dd = _padded(inp, F)
    o, d = np.zeros((len(ra), 3), F), np.zeros((len(ra), 3), F)
    for j in range(valid.shape[1]):
        v = valid[:, j, None]
        o = np.where(v, o + dx[:, j], o)
        term = (t[:, j, None] * dx[:, j]) + dd[:, j]
        d = np.where(v, d + term, d)
    return _by_ray(ra, inp["n"], o, d)


def _butterfly(v):
    """v [..., 64] float32 -> [...]: v += shfl_xor(v, d) for d = 32, 16, ..., 1 (every lane ends with the same sum)."""
    v = np.asarray(v, F)
    lanes = np.arange(WAVE)
    d = WAVE // 2
    while d >= 1:
        v = v + v[..., lanes ^ d]
        d //= 2
    return v[..., 0]


def march_bwd_wave32(inp):
    """float32 in march_train_bwd_kernel's order: lane l adds samples l, l + 64, ... serially, then the butterfly."""
    ra, valid, t, dx, dd = _padded(inp, F)
    m, L = valid.shape
    Lp = -(-L // WAVE) * WAVE
    pad = lambda a: np.concatenate([a, np.zeros((m, Lp - L) + a.shape[2:], a.dtype)], 1)
    t, dx, dd = pad(t), pad(dx), pad(dd)
    o, d = np.zeros((m, WAVE, 3), F), np.zeros((m, WAVE, 3), F)
    for b in range(0, Lp, WAVE):                       # (padding adds +0.0: exact)
        x = dx[:, b:b + WAVE]
        o = o + x
        d = d + ((t[:, b:b + WAVE, None] * x) + dd[:, b:b + WAVE])
    return _by_ray(ra, inp["n"], _butterfly(np.moveaxis(o, 1, -1)), _butterfly(np.moveaxis(d, 1, -1)))


# ------------------------------------------------------------------------------------------------------------------ poses
def _pose_terms(inp, dtype, img_null=None, pix_null=False):
    """[n, 3, 4] terms of every ray (the rounded products in `dtype`) and the image of every ray."""
    n = inp["n"]
    img = inp["img"] if img_null is None else np.full(n, img_null, np.int64)
    pix = np.arange(n) if pix_null else inp["pix"]
    dirs = inp["directions"][pix].astype(dtype)
    g_d = inp["g_d"].astype(dtype) if inp.get("g_d") is not None else np.zeros((n, 3), dtype)
    g_o = inp["g_o"].astype(dtype) if inp.get("g_o") is not None else np.zeros((n, 3), dtype)
    return np.concatenate([g_d[:, :, None] * dirs[:, None, :], g_o[:, :, None]], 2), img


def pose_bwd_64(inp, img_null=None, pix_null=False):
    """-> d_poses, S: [n_img,3,4] float64."""
    terms, img = _pose_terms(inp, np.float64, img_null, pix_null)
    out, S = np.zeros((inp["n_img"], 3, 4)), np.zeros((inp["n_img"], 3, 4))
    ok = (img >= 0) & (img < inp["n_img"])
    np.add.at(out, img[ok], terms[ok])
    np.add.at(S, img[ok], np.abs(terms[ok]))
    return out, S


def pose_bwd_serial32(inp, img_null=None, pix_null=False):
    """Each image's rays in ray order, one float32 add per term."""
    terms, img = _pose_terms(inp, F, img_null, pix_null)
    out = np.zeros((inp["n_img"], 3, 4), F)
    for i in range(inp["n_img"]):
        mine = terms[img == i]
        acc = np.zeros((3, 4), F)
        for row in mine:
            acc = acc + row
        out[i] = acc
    return out


def pose_bwd_wave32(inp, img_null=None, pix_null=False):
    """float32 in sample_rays_bwd_kernel's order: thread t of the image's block visits k = t, t + 256, ... of all rays."""
    terms, img = _pose_terms(inp, F, img_null, pix_null)
    n = inp["n"]
    npad = -(-max(n, 1) // POSE_THREADS) * POSE_THREADS
    out = np.zeros((inp["n_img"], 3, 4), F)
    for i in range(inp["n_img"]):
        mine = np.zeros((npad, 3, 4), F)
        mine[:n] = np.where((img == i)[:, None, None], terms, F(0))
        acc = np.zeros((POSE_THREADS, 3, 4), F)
        for b in range(0, npad, POSE_THREADS):          # (a ray of another image is skipped; adding its +0.0 is the same)
            acc = acc + mine[b:b + POSE_THREADS]
        w = _butterfly(np.moveaxis(acc.reshape(POSE_THREADS // WAVE, WAVE, 3, 4), 1, -1))          # [4 waves, 3, 4]
        out[i] = (w[0] + w[1]) + (w[2] + w[3])
    return out


# ------------------------------------------------------------------------------------------------------------------ yardstick
def e32(serial, ref, S):
    m = S > 0
    return float(np.max(np.abs(serial.astype(np.float64) - ref)[m] / S[m])) if m.any() else 0.0


def worst_ratio(got, ref, S, E32):
    """max |got - f64| / (E32 S) over the elements with S > 0; the elements with S == 0 must hold exact zeros."""
    got = np.asarray(got, np.float64)
    m = S > 0
    assert np.all(got[~m] == 0), "an element without terms is not exactly zero"
    return float(np.max(np.abs(got - ref)[m] / (E32 * S[m]))) if m.any() and E32 > 0 else 0.0


def within(got, ref, S, E32, k=K):
    return bool(np.all(np.abs(np.asarray(got, np.float64) - ref) <= k * E32 * S + TINY))
