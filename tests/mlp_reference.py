"""numpy float64 model of the fused MLP's numerical contract (csrc/mlp.hip: tile_forward_frags, mlp_bwd_kernel), with a running
per-element error bound for the backward, the "dyadic" cases for which the forward is exact in every summation order, and the compare
functions tests/test_gpu_mlp_exact.py (on the kernels) and tests/test_mlp_reference.py (on mutated copies of this model) both call.

Rounding points (round=True; round=False turns every one of them off and leaves the plain float64 graph of modules/networks.py):

forward   enc -> fp16, W_k -> fp16 (the packer).  Every Linear is an exact sum (fp32 accumulation in the kernel) followed by one
          f32 -> fp16 rounding; ReLU acts on the fp16 value.  h = fp16(L2).  sigma = exp(h0), unclamped, in f32 (kept in float64
          here: the comparison allows the f32 rounding).  Directions: d/|d|, (. + 1)/2, the sixteen SH expressions (deploy_reference.sh16,
          the same ones as sh16 in ngp_device.h) in float64, each rounded to fp16.  rgb = fp16(sigmoid(fp16(L5))).
backward  dz5 = fp16(drgb (1 - y) y), y the fp16 rgb.  dz4, dz3, dz1 = fp16(mask * W^T dz), the mask `act > 0` on the forward's fp16
          activation.  dz2 = fp16(W3h^T dz3), then dz2[0] = fp16(dz2[0] + fp16(dsigma exp(clamp(h0, -15, 15)))).  d_enc = W1^T dz1 and
          dW_k = dz_k^T x_k are f32 sums of fp16 operands, not rounded again.  dW is the flat 9 408 vector (OFFS).

Error bound E (backward(...).E_denc, .E_dW): how far a correct kernel may be from this model, element by element, propagated next to the
gradients through |W^T| and the masks.  Sources: y one fp16 ulp off (|drgb| |1 - 2y| ulp16(y)); the TruncExp exponential (2^-21
relative); one fp16 rounding (2^-11 relative to the value) at each dz_k; fp32 accumulation, K 2^-24 sum|w||dz| per contraction with
K = 32 or 64, and for dW with K the number of samples that are summed with a non-zero dz_k row (an all-zero row adds exact zeros); one
fp16 ulp on each SH input for the SH columns of dW3.  Second-order terms are dropped: the comparison allows 2 E."""
import numpy as np

from deploy_reference import sh16

OFFS = (0, 2048, 3072, 5120, 9216, 9408)
SHAPES = ((64, 32), (16, 64), (64, 32), (64, 64), (3, 64))
N_W = OFFS[-1]
U16, U32 = 2.0**-11, 2.0**-24


class Bag(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def r16(x, on=True):
    if not on:
        return x
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float16).astype(np.float64)


def ulp16(x):
    """Spacing of fp16 at |x| (of the binade |x| lies in)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.spacing(np.abs(np.asarray(x)).astype(np.float16)).astype(np.float64)


def _mm(a, b, accum):
    """a [m,k] @ b [k,n].  accum='f64': float64.  accum='f32rev': another legitimate accumulation -- binary32, the contraction index
    walked in reversed order."""
    with np.errstate(over="ignore", invalid="ignore"):
        if accum == "f32rev":
            return (a[:, ::-1].astype(np.float32) @ b[::-1].astype(np.float32)).astype(np.float64)
        return a @ b


def to_pairs(enc_nat, n_max, fill=0):
    """[n,32] natural (level-major) -> pair-major planes [8, n_max, 4] (include/ngp_hip.h, enc_pairs): plane p holds
    [level p f0,f1 | level 15-p f0,f1]; rows >= n hold `fill`.  numpy arrays and torch tensors alike."""
    n = enc_nat.shape[0]
    if isinstance(enc_nat, np.ndarray):
        out = np.full((8, n_max, 4), fill, enc_nat.dtype)
    else:
        out = enc_nat.new_full((8, n_max, 4), fill)
    for p in range(8):
        out[p, :n, 0:2] = enc_nat[:, 2 * p:2 * p + 2]
        out[p, :n, 2:4] = enc_nat[:, 2 * (15 - p):2 * (15 - p) + 2]
    return out


def from_pairs(planes, n):
    """The inverse of to_pairs for the first n rows (numpy)."""
    out = np.empty((n, 32), planes.dtype)
    for p in range(8):
        out[:, 2 * p:2 * p + 2] = planes[p, :n, 0:2]
        out[:, 2 * (15 - p):2 * (15 - p) + 2] = planes[p, :n, 2:4]
    return out


def flat_dw(dWs):
    return np.concatenate([np.asarray(w, np.float64).reshape(-1) for w in dWs])


def forward(enc, dirs, W, round=True, color=True, accum="f64", mut=()):
    """enc [n,32], raw dirs [n,3], W = five [out,in] matrices -> Bag of every intermediate (sigma [n], rgb [n,3], ...).
    mut: deliberate faults for the sensitivity tests (('a1_swap', i, j) exchanges two hidden features between layers 1 and 2)."""
    mut = dict((m[0], m[1:]) for m in mut)
    f = Bag(round=round, accum=accum)
    f.e = r16(np.asarray(enc, np.float64), round)
    f.W = [r16(np.asarray(w, np.float64), round) for w in W]
    f.z1 = _mm(f.e, f.W[0].T, accum)
    f.a1 = np.maximum(r16(f.z1, round), 0.0)
    a1 = f.a1
    if "a1_swap" in mut:
        i, j = mut["a1_swap"]
        a1 = a1.copy(); a1[:, [i, j]] = a1[:, [j, i]]
    f.z2 = _mm(a1, f.W[1].T, accum)
    f.h = r16(f.z2, round)
    with np.errstate(over="ignore"):
        f.sigma = np.exp(f.h[:, 0])
    if not color:
        return f
    with np.errstate(divide="ignore", invalid="ignore"):
        f.sh = r16(sh16(dirs, np.float64), round)
    f.in3 = np.concatenate([f.sh, f.h], 1)
    f.z3 = _mm(f.in3, f.W[2].T, accum)
    f.a3 = np.maximum(r16(f.z3, round), 0.0)
    f.z4 = _mm(f.a3, f.W[3].T, accum)
    f.a4 = np.maximum(r16(f.z4, round), 0.0)
    f.z5 = _mm(f.a4, f.W[4].T, accum)
    f.c = r16(f.z5, round)
    if accum == "f32rev":
        c32 = f.c.astype(np.float32)
        f.rgb = r16((np.float32(1) / (np.float32(1) + np.exp(-c32))).astype(np.float64), round)
    else:
        f.rgb = r16(1.0 / (1.0 + np.exp(-f.c)), round)
    return f


def backward(f, dsigma, drgb, mut=()):
    """f = forward(...) with colour; dsigma [n] f32, drgb [n,3] (fp16 values) -> Bag(d_enc [n,32], dW [9408], E_denc, E_dW, dz1..dz5).
    mut: ('mask_ge',) takes the ReLU mask as act >= 0, ('no_clamp',) drops TruncExp's clamp."""
    mut = dict((m[0], m[1:]) for m in mut)
    rnd, accum = f.round, f.accum
    W1, W2, W3, W4, W5 = f.W
    W3h = W3[:, 16:]
    A = np.abs
    active = (lambda a: a >= 0) if "mask_ge" in mut else (lambda a: a > 0)
    m4, m3, m1 = active(f.a4), active(f.a3), active(f.a1)
    dsigma, drgb = np.asarray(dsigma, np.float64), np.asarray(drgb, np.float64)
    b = Bag()
    with np.errstate(over="ignore", invalid="ignore"):
        y = f.rgb
        b.dz5 = r16(drgb * ((1.0 - y) * y), rnd)
        b.dz4 = r16(np.where(m4, _mm(b.dz5, W5, accum), 0.0), rnd)
        b.dz3 = r16(np.where(m3, _mm(b.dz4, W4, accum), 0.0), rnd)
        dz2p = r16(_mm(b.dz3, W3h, accum), rnd)
        h0 = f.h[:, 0]
        gsv = dsigma * np.exp(h0 if "no_clamp" in mut else np.clip(h0, -15.0, 15.0))
        gs = r16(gsv, rnd)
        b.dz2 = dz2p.copy()
        b.dz2[:, 0] = r16(dz2p[:, 0] + gs, rnd)
        b.dz1 = r16(np.where(m1, _mm(b.dz2, W2, accum), 0.0), rnd)
        b.d_enc = _mm(b.dz1, W1, accum)
        dzs, xs = [b.dz1, b.dz2, b.dz3, b.dz4, b.dz5], [f.e, f.a1, f.in3, f.a3, f.a4]
        b.dWs = [_mm(dz.T, x, accum) for dz, x in zip(dzs, xs)]
        b.dW = flat_dw(b.dWs)
        if not rnd:
            return b
        # ---- the running bound ----
        e5 = A(drgb) * A(1.0 - 2.0 * y) * ulp16(y) + U16 * A(b.dz5)
        e4 = m4 * (e5 @ A(W5) + 32 * U32 * (A(b.dz5) @ A(W5))) + U16 * A(b.dz4)
        e3 = m3 * (e4 @ A(W4) + 64 * U32 * (A(b.dz4) @ A(W4))) + U16 * A(b.dz3)
        e2 = e3 @ A(W3h) + 64 * U32 * (A(b.dz3) @ A(W3h)) + U16 * A(dz2p)
        e2[:, 0] += 2.0**-21 * A(gsv) + U16 * A(gs) + U32 * (A(dz2p[:, 0]) + A(gs)) + U16 * A(b.dz2[:, 0])
        e1 = m1 * (e2 @ A(W2) + 32 * U32 * (A(b.dz2) @ A(W2))) + U16 * A(b.dz1)
        b.E_denc = e1 @ A(W1) + 64 * U32 * (A(b.dz1) @ A(W1))
        E = []
        for k, (ek, dz, x) in enumerate(zip([e1, e2, e3, e4, e5], dzs, xs)):
            K = int(np.count_nonzero(np.any(dz != 0, axis=1)))
            Ek = ek.T @ A(x) + K * U32 * (A(dz).T @ A(x))
            if k == 2:
                Ek[:, :16] += A(dz).T @ ulp16(f.sh)
            E.append(Ek)
        b.E_dWs = E
        b.E_dW = flat_dw(E)
        # a non-finite gradient has no bound: inf - inf below would make it NaN where the gradient itself is +-inf
        b.E_denc = np.where(np.isfinite(b.d_enc), b.E_denc, np.inf)
        b.E_dW = np.where(np.isfinite(b.dW), b.E_dW, np.inf)
    return b


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
N_CASES = 8          # 64 inputs / 8 non-zeros per row: after 8 rotations every weight position has been non-zero
# (out, in, non-zeros per row, magnitudes): W1, W2, the h columns of W3, W4, W5
_SPARSE = ((64, 32, 8, (1.0,)), (16, 64, 8, (0.5, 0.25)), (64, 16, 4, (1.0, 0.5)), (64, 64, 8, (0.5,)), (3, 64, 8, (0.125,)))


def dyadic_weights(case):
    """Sparse rows of +-2^-k.  Row r of a layer keeps one fixed random order of its columns; case c takes the c-th run of m of them
    (cyclically), so N_CASES cases cover every position.  W2's row 0 (h0, the log density) is +-1/8 so that sigma and the loss-scaled
    dsigma exp(h0) stay inside fp16; W3's h0 column is +-1 (h0 lies on a finer grid than the other h).  W3[:, :16] (SH) is zero."""
    order = np.random.default_rng(977)
    rng = np.random.default_rng(100 + case)
    out = []
    for o, k, m, mags in _SPARSE:
        w = np.zeros((o, k))
        for r in range(o):
            cols = np.roll(order.permutation(k), -m * case)[:m]
            w[r, cols] = rng.choice(mags, m) * rng.choice([-1.0, 1.0], m)
        out.append(w)
    out[1][0] = np.sign(out[1][0]) * 0.125
    h0col = out[2][:, 0]
    out[2][:, 0] = np.sign(h0col)
    out[2] = np.concatenate([np.zeros((64, 16)), out[2]], 1)
    return [w.astype(np.float32) for w in out]


def dyadic_inputs(case, n):
    rng = np.random.default_rng(5000 + case)
    enc = rng.integers(-1, 5, (n, 32)).astype(np.float32) * np.float32(0.5)           # {-1/2, 0, ..., 2}: signed, mean 3/4
    dirs = rng.standard_normal((n, 3)).astype(np.float32)
    return enc, dirs


def assert_exact(enc, dirs, W):
    """The claim the per-element forward checks rest on: with these inputs every pre-activation of every layer is an fp16 number, so
    the rounded and the unrounded model -- and every summation order -- agree bit for bit.  (The SH values themselves are inexact;
    they may not reach a pre-activation: W3[:, :16] == 0, or a probe of its own.)"""
    fr = forward(enc, dirs, W, round=True)
    if np.any(np.asarray(W[2])[:, :16] != 0):           # an SH probe: one-hot rows, exact given the fp16 SH values
        return fr
    fu = forward(np.asarray(enc, np.float16), dirs, [np.asarray(w, np.float16) for w in W], round=False)
    for name in ("z1", "z2", "z3", "z4", "z5"):
        assert np.array_equal(fr[name], fu[name]), "layer %s is not exact for this case" % name
        assert np.array_equal(r16(fr[name]), fr[name]), "layer %s is not an fp16 number" % name
    return fr


def dyadic_case(case, n):
    """-> (enc, dirs, W, forward Bag), exactness asserted."""
    W = dyadic_weights(case)
    enc, dirs = dyadic_inputs(case, n)
    return enc, dirs, W, assert_exact(enc, dirs, W)


def gradients(case, n, keep=1.0):
    """Loss-scaled dsigma (f32) and drgb (fp16 values), like GradScaler's.  About one row in eight is all zero (never the first or the last); keep < 1 zeroes all but
    that share of the rows (the first and last 40 stay), so that a large n still sums few enough samples per weight for one sample to
    count.  The signs lean one way (7 : 1): a sum over samples with balanced signs cancels to the size of its own rounding noise."""
    rng = np.random.default_rng(9000 + case)
    sgn = lambda shape: np.where(rng.random(shape) < 0.125, -1.0, 1.0)
    dsig = (np.abs(rng.standard_normal(n)) * sgn(n) * 64).astype(np.float32)
    drgb = (np.abs(rng.standard_normal((n, 3))) * sgn((n, 3)) * 64).astype(np.float16)
    live = rng.random(n) < 0.875 * keep
    if keep < 1.0:
        live[:40] = True; live[-40:] = True
    live[0] = live[-1] = True                   # the first sample and the tail lane always count
    dsig[~live] = 0; drgb[~live] = 0
    # sample 0 takes a four-sigma dsigma: alone (n = 1) its d_enc is then led by the density path, whose error is two roundings; led
    # by the colour path, whose error passes four sparse mixed-sign layers, E would be no small fraction of so few values
    dsig[0] = np.float32(256.0) * np.sign(dsig[0])
    return dsig, drgb


def live_list(case, n_max, n_live):
    """A shuffled strict subset of range(n_max), padded to n_max entries with valid rows the call does not own."""
    rng = np.random.default_rng(7000 + case)
    perm = rng.permutation(n_max).astype(np.int32)
    return perm, perm[:n_live]


def clamp_case():
    """h0 = enc[:, 5] through two units relu(x), relu(-x) subtracted; every other weight zero.  h0 in {-16, -15, 0, 15, 16} and
    halfway values."""
    W = [np.zeros(s, np.float32) for s in SHAPES]
    W[0][0, 5], W[0][1, 5] = 1.0, -1.0
    W[1][0, 0], W[1][0, 1] = 1.0, -1.0
    h0 = np.array([-16, -15, 0, 15, 16, -15.5, 15.5, 1, -1, 16, -16, 0, 15, -15, 3, -3, 16, 15, -16], np.float32)
    enc = np.zeros((len(h0), 32), np.float32)
    enc[:, 5] = h0
    dirs = np.tile(np.array([[0.3, -0.5, 0.8]], np.float32), (len(h0), 1))
    dsig = np.full(len(h0), 2.0**-8, np.float32) * np.where(np.arange(len(h0)) % 2, -1, 1).astype(np.float32)
    drgb = np.zeros((len(h0), 3), np.float16)
    return enc, dirs, W, dsig, drgb


SH_SEEDS = 11        # 3 outputs per seed: 33 >= the 32 (coefficient, sign) pairs


def sh_case(seed, n=96):
    """Hidden unit u of layer 3 takes SH coefficient u % 16 with weight +1 (u < 16) or -1 (16 <= u < 32); W4 passes the units
    through, W5's output o picks unit (3 seed + o) % 32.  The xyz path is zeroed.  Directions: random, plus the axes and diagonals."""
    W = [np.zeros(s, np.float32) for s in SHAPES]
    for u in range(32):
        W[2][u, u % 16] = 1.0 if u < 16 else -1.0
        W[3][u, u] = 1.0
    units = [(3 * seed + o) % 32 for o in range(3)]
    for o, u in enumerate(units):
        W[4][o, u] = 1.0
    rng = np.random.default_rng(300 + seed)
    dirs = rng.standard_normal((n, 3)).astype(np.float32) * np.float32(3.0)
    fixed = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1], [-1, -1, -1], [1, -1, 0],
                      [0, 2, -2]], np.float32)
    dirs[:len(fixed)] = fixed
    enc = rng.integers(-2, 4, (n, 32)).astype(np.float32) * np.float32(0.5)
    return enc, dirs, W, units


# ---------------------------------------------------------------- comparisons ----------------------------------------------------------------
def ulps16_apart(a, b):
    """Distance in fp16 steps between two arrays of fp16 values (adjacent representable numbers are 1 apart; NaN vs NaN is 0, NaN
    vs a number is a large count)."""
    def key(x):
        bits = np.asarray(x, np.float16).view(np.uint16).astype(np.int64)
        return np.where(bits & 0x8000, -(bits & 0x7fff), bits)
    a16, b16 = np.asarray(a, np.float16), np.asarray(b, np.float16)
    d = np.abs(key(a16) - key(b16))
    nan_a, nan_b = np.isnan(a16), np.isnan(b16)
    return np.where(nan_a | nan_b, np.where(nan_a & nan_b, 0, 1 << 20), d)


def compare_forward(sigma, rgb, ref, rgb_ulps=1, rows=None):
    """sigma f32 [n] and rgb fp16 [n,3] of a kernel against ref = forward(...): sigma within 2^-22 relative of exp(h0) (expf is
    documented at 1 ulp; the second is the model's own rounding to f32), rgb within rgb_ulps fp16 steps.  rows: the model's rows the
    outputs correspond to.  rgb=None: density only.  -> dict(sigma_rel, rgb_ulps, rgb_off_share); raises AssertionError."""
    rs = ref.sigma if rows is None else ref.sigma[rows]
    sigma = np.asarray(sigma, np.float64)
    assert sigma.shape == rs.shape
    rel = np.abs(sigma - rs) / rs
    worst = float(rel.max()) if rel.size else 0.0
    assert np.all(rel <= 2.0**-22), "sigma: worst relative error %.3e (2^-22 = %.3e) at row %d" % (worst, 2.0**-22, int(rel.argmax()))
    out = dict(sigma_rel=worst, rgb_ulps=0, rgb_off_share=0.0)
    if rgb is None:
        return out
    rr = ref.rgb if rows is None else ref.rgb[rows]
    assert rgb.shape == rr.shape
    d = ulps16_apart(rgb, rr)
    out["rgb_ulps"] = int(d.max()) if d.size else 0
    out["rgb_off_share"] = float(np.mean(d != 0)) if d.size else 0.0
    assert np.all(d <= rgb_ulps), "rgb: %d elements more than %d fp16 ulp off, worst %d at %s" % (
        int(np.sum(d > rgb_ulps)), rgb_ulps, out["rgb_ulps"], np.unravel_index(int(d.argmax()), d.shape))
    return out


def _within(got, ref, E, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), "%s: finite where the model is not, or the reverse" % what
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(np.where(fin, got - ref, 0.0))
        bad = err > 2.0 * np.where(fin, E, 0.0)
        ratio = np.where(err > 0, err / np.where(fin, E, 1.0), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert not bad.any(), "%s: %d of %d elements beyond 2 E; worst |err|/E = %.3g at %s (got %r, model %r, E %.3g)" % (
        what, int(bad.sum()), bad.size, worst, np.unravel_index(int(ratio.argmax()), ratio.shape), got.flat[int(ratio.argmax())],
        ref.flat[int(ratio.argmax())], E.flat[int(ratio.argmax())])
    return worst


def compare_backward(d_enc, dW, ref):
    """d_enc [n,32] (row j = position j of the model's inputs) and the flat dW [9408] of a kernel against ref = backward(...):
    |got - model| <= 2 E element by element.  -> dict of the worst |err|/E per tensor; raises AssertionError."""
    out = dict(d_enc=_within(d_enc, ref.d_enc, ref.E_denc, "d_enc"))
    dW = np.asarray(dW, np.float64)
    assert dW.shape == (N_W,)
    for k in range(5):
        lo, hi = OFFS[k], OFFS[k + 1]
        out["dW%d" % (k + 1)] = _within(dW[lo:hi], ref.dW[lo:hi], ref.E_dW[lo:hi], "dW%d" % (k + 1))
    return out


def assert_bound_not_vacuous(ref):
    """2 E below 2^-6 of the tensor's largest magnitude for at least 99 % of the elements of d_enc and of each dW_k."""
    shares = {}
    for name, g, E in [("d_enc", ref.d_enc, ref.E_denc)] + [("dW%d" % (k + 1), ref.dWs[k], ref.E_dWs[k]) for k in range(5)]:
        top = np.abs(g).max()
        assert top > 0, name
        shares[name] = float(np.mean(2.0 * E < 2.0**-6 * top))
        assert shares[name] >= 0.99, "%s: the bound is vacuous: 2 E < 2^-6 max|.| for only %.2f %% of the elements" % (
            name, 100 * shares[name])
    return shares
