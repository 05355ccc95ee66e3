"""The fused MLP kernels (csrc/mlp.hip) against the float64 model of their numerical contract (tests/mlp_reference.py), element by
element: forward and backward in every entry point and layout -- natural, pair-major, n_dev below n_max, live lists, dW by atomics and
by slabs -- at one trip / round of the persistent loops and at more than one.  The inputs are the model's dyadic cases, for which the
forward is exact in any summation order, so sigma is held to the accuracy of expf, rgb to one fp16 ulp and the gradients to twice the
model's running error bound.  Every test prints the figures it measured (pytest -s): profiles/PARITY_NOTES.md records them."""
import functools

import numpy as np
import pytest
import torch

import mlp_reference as R

pytestmark = pytest.mark.gpu

# mlp.hip, mlp_grid(): the persistent forward grid is at most 768 blocks x 4 waves, and a wave takes 32 samples per trip -- the second
# trip starts at 768 * 4 * 32 samples.  Five more full trips' worth of waves and an odd tail of 13.
FWD_ONE_TRIP = 768 * 4 * 32
FWD_N = [1, 15, 16, 17, 33, FWD_ONE_TRIP + 5 * 32 + 13]
# mlp.hip, mlp_bwd_launch(): at most 256 blocks, a round of a block is 6 groups x 32 = 192 samples -- the second round starts at
# 256 * 192 samples.  Two more full rounds' worth of blocks and an odd tail of 47.
BWD_ONE_ROUND = 256 * 192
BWD_N = [1, 47, 193, BWD_ONE_ROUND + 2 * 192 + 47]
SPARE = 45                     # rows of a buffer beyond n_dev / outside the list
SIG_SENT, RGB_SENT, ENC_SENT, SLAB_SENT, FLAG_SENT = -7777.0, -7.0, -5555.0, 12345.0, 5
BIG_CASES = (3, 6)             # the cases the sizes beyond one trip / round use (all N_CASES run at the small sizes)


def _n_id(n):
    if n > FWD_ONE_TRIP:
        return "n%d_second_trip" % n
    if n > BWD_ONE_ROUND:
        return "n%d_second_round" % n
    return "n%d" % n


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cases(n, k):
    return [BIG_CASES[k % len(BIG_CASES)]] if n > 1000 else list(range(R.N_CASES))


@functools.lru_cache(maxsize=None)
def _fwd_ref(case, n):
    return R.dyadic_case(case, n)


@functools.lru_cache(maxsize=None)
def _bwd_ref(case, n):
    enc, dirs, W, f = _fwd_ref(case, n)
    dsig, drgb = R.gradients(case, n, keep=1.0 if n < 1000 else 1.0 / 16)
    b = R.backward(f, dsig, drgb)
    R.assert_bound_not_vacuous(b)                       # on the CPU, before anything is compared
    return enc, dirs, W, f, dsig, drgb, b


def _pack(L, W, pairs):
    from ngp_hip.ops import _ptr, _stream, check
    ws = [_gpu(w) for w in W]
    wpack = torch.empty(L.ngp_mlp_wpack_halfs(), device="cuda", dtype=torch.float16)
    check(L.ngp_mlp_pack(*[_ptr(w) for w in ws], pairs, _ptr(wpack), _stream()), "ngp_mlp_pack")
    torch.cuda.synchronize()
    return wpack


def _spread(rows, n_max, where, filler):
    """A buffer of n_max rows with rows[j] at row where[j] and `filler` everywhere else."""
    out = np.empty((n_max,) + rows.shape[1:], rows.dtype)
    out[...] = filler
    out[where] = rows
    return out


# ------------------------------------------------------------ 3a. forward ------------------------------------------------------------
FWD_VARIANTS = ["fwd", "ex_natural", "ex_pairs", "ex_ndev_natural", "ex_ndev_pairs", "list_natural", "list_pairs",
                "density_natural", "density_ndev_pairs"]


def _run_forward(L, variant, enc, dirs, W, case):
    """-> (sigma [n_max], rgb [n_max,3] or None, rows: the buffer row of each of the case's n samples)."""
    from ngp_hip.ops import _ptr, _stream, check
    n = enc.shape[0]
    pairs = 1 if variant.endswith("pairs") else 0
    spare = variant.startswith("list") or "ndev" in variant
    n_max = n + SPARE if spare else n
    if variant.startswith("list"):
        perm, rows = R.live_list(case, n_max, n)
    else:
        perm, rows = None, np.arange(n)
    # rows the call does not own hold values that would show: a large enc, a direction of their own
    enc_b = _spread(enc, n_max, rows, np.float32(64.0))
    dirs_b = _spread(dirs, n_max, rows, np.float32(1.0))
    enc_d = _gpu(R.to_pairs(enc_b, n_max)) if pairs else _gpu(enc_b)
    dirs_d = _gpu(dirs_b)
    wpack = _pack(L, W, pairs)
    sig = torch.full((n_max,), SIG_SENT, device="cuda")
    rgb = torch.full((n_max, 3), RGB_SENT, device="cuda", dtype=torch.float16)
    n_dev = torch.tensor([n], device="cuda", dtype=torch.int32) if spare else None
    if variant == "fwd":
        check(L.ngp_mlp_fwd(_ptr(enc_d), _ptr(dirs_d), _ptr(wpack), n, _ptr(sig), _ptr(rgb), _stream()), variant)
    elif variant.startswith("ex"):
        check(L.ngp_mlp_fwd_ex(_ptr(enc_d), _ptr(dirs_d), _ptr(wpack), n_max, _ptr(n_dev), pairs, _ptr(sig), _ptr(rgb), _stream()), variant)
    elif variant.startswith("list"):
        lst = _gpu(perm)
        check(L.ngp_mlp_fwd_list(_ptr(enc_d), _ptr(dirs_d), _ptr(wpack), n_max, _ptr(n_dev), _ptr(lst), pairs, _ptr(sig), _ptr(rgb),
                                 _stream()), variant)
    else:
        check(L.ngp_mlp_fwd_ex(_ptr(enc_d), _ptr(None), _ptr(wpack), n_max, _ptr(n_dev), pairs, _ptr(sig), _ptr(None), _stream()), variant)
        torch.cuda.synchronize()
        return sig.cpu().numpy(), None, rows
    torch.cuda.synchronize()
    return sig.cpu().numpy(), rgb.cpu().numpy(), rows


def _check_forward(sig, rgb, rows, ref, rgb_ulps=1):
    stats = R.compare_forward(sig[rows], None if rgb is None else rgb[rows], ref, rgb_ulps=rgb_ulps)
    other = np.ones(sig.shape[0], bool)
    other[rows] = False
    assert np.all(sig[other] == np.float32(SIG_SENT)), "sigma written outside the rows the call owns"
    if rgb is not None:
        assert np.all(rgb[other] == np.float16(RGB_SENT)), "rgb written outside the rows the call owns"
    return stats


@pytest.mark.parametrize("n", FWD_N, ids=_n_id)
@pytest.mark.parametrize("variant", FWD_VARIANTS)
def test_forward_per_element(hip_lib, variant, n):
    worst = dict(sigma_rel=0.0, rgb_ulps=0, rgb_off_share=0.0)
    for case in _cases(n, FWD_VARIANTS.index(variant)):
        enc, dirs, W, f = _fwd_ref(case, n)
        sig, rgb, rows = _run_forward(hip_lib, variant, enc, dirs, W, case)
        stats = _check_forward(sig, rgb, rows, f)
        worst = {k: max(worst[k], stats[k]) for k in worst}
    print("\nMLPEXACT fwd %s n=%d sigma_rel=%.3e (2^-22=%.3e) rgb_ulps=%d rgb_off_share=%.5f" % (
        variant, n, worst["sigma_rel"], 2.0**-22, worst["rgb_ulps"], worst["rgb_off_share"]))


# ------------------------------------------------------------ 3b. backward ------------------------------------------------------------
BWD_VARIANTS = ["%s_%s_%s" % (lay, lst, out) for lay in ("natural", "pairs") for lst in ("all", "list_ndev")
                for out in ("atomics", "slabs")]


def _run_backward(L, variant, enc, dirs, W, dsig, drgb, case, flag=FLAG_SENT):
    """-> (d_enc [n,32] in position order, dW [9408], flag after the call).  Asserts the sentinels on the way."""
    from ngp_hip.ops import _ptr, _stream, check
    n = enc.shape[0]
    pairs = 1 if variant.startswith("pairs") else 0
    listed = "list_ndev" in variant
    n_max = n + SPARE if listed else n
    if listed:
        perm, rows = R.live_list(case, n_max, n)
    else:
        perm, rows = None, np.arange(n)
    enc_b = _spread(enc, n_max, rows, np.float32(64.0))
    enc_d = _gpu(R.to_pairs(enc_b, n_max)) if pairs else _gpu(enc_b)
    dirs_d = _gpu(_spread(dirs, n_max, rows, np.float32(1.0)))
    dsig_d = _gpu(_spread(dsig, n_max, rows, np.float32(1000.0)))
    drgb_d = _gpu(_spread(drgb, n_max, rows, np.float16(1000.0)))
    wpack = _pack(L, W, pairs)
    d_enc = torch.full((8, n_max, 4) if pairs else (n_max, 32), ENC_SENT, device="cuda")
    found = torch.tensor([flag], device="cuda", dtype=torch.int32)
    n_dev = torch.tensor([n], device="cuda", dtype=torch.int32) if listed else None
    idx = _gpu(perm) if listed else None
    dW = torch.zeros(R.N_W, device="cuda")
    if variant.endswith("atomics"):
        check(L.ngp_mlp_bwd_live(_ptr(enc_d), _ptr(dirs_d), _ptr(wpack), _ptr(dsig_d), _ptr(drgb_d), n_max, _ptr(n_dev), _ptr(idx),
                                 pairs, _ptr(d_enc), _ptr(dW), _ptr(found), _stream()), variant)
    else:
        parts_max = L.ngp_mlp_dw_parts_max()
        parts = torch.full((parts_max * R.N_W,), SLAB_SENT, device="cuda")
        n_parts = L.ngp_mlp_bwd_live_parts(_ptr(enc_d), _ptr(dirs_d), _ptr(wpack), _ptr(dsig_d), _ptr(drgb_d), n_max, _ptr(n_dev),
                                           _ptr(idx), pairs, _ptr(d_enc), _ptr(parts), _ptr(found), _stream())
        assert 1 <= n_parts <= parts_max
        check(L.ngp_mlp_dw_reduce(_ptr(parts), n_parts, _ptr(dW), _stream()), "ngp_mlp_dw_reduce")
        torch.cuda.synchronize()
        assert torch.all(parts[n_parts * R.N_W:] == SLAB_SENT), "a slab beyond n_parts was written"
    torch.cuda.synchronize()
    de = d_enc.cpu().numpy()
    if pairs:
        assert np.all(de[:, n:, :] == np.float32(ENC_SENT)), "d_enc written beyond n_dev"
        de = R.from_pairs(de, n)
    else:
        assert np.all(de[n:] == np.float32(ENC_SENT)), "d_enc written beyond n_dev"
        de = de[:n]
    return de, dW.cpu().numpy(), int(found[0])


@pytest.mark.parametrize("n", BWD_N, ids=_n_id)
@pytest.mark.parametrize("variant", BWD_VARIANTS)
def test_backward_per_element(hip_lib, variant, n):
    worst = {}
    for case in _cases(n, BWD_VARIANTS.index(variant)):
        enc, dirs, W, f, dsig, drgb, b = _bwd_ref(case, n)
        de, dW, flag = _run_backward(hip_lib, variant, enc, dirs, W, dsig, drgb, case)
        stats = R.compare_backward(de, dW, b)
        assert flag == FLAG_SENT, "found_inf was written by a run whose gradients are all finite"
        worst = {k: max(worst.get(k, 0.0), v) for k, v in stats.items()}
    print("\nMLPEXACT bwd %s n=%d worst |err|/E: %s" % (variant, n, " ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))


# ------------------------------------------------------------ 3c. SH columns ------------------------------------------------------------
def test_sh_columns_reach_rgb_within_two_ulp(hip_lib):
    """Each of the 16 SH coefficients, with either sign, alone in front of an output: an order or sign error in sh_quad shows at
    once.  2 fp16 ulp: the SH input contributes one through a slope of at most 1/4, the final rounding one."""
    seen, worst, off = set(), 0, []
    for seed in range(R.SH_SEEDS):
        enc, dirs, W, units = R.sh_case(seed)
        f = R.assert_exact(enc, dirs, W)
        seen.update((u % 16, u < 16) for u in units)
        for variant in ("fwd", "ex_pairs"):
            sig, rgb, rows = _run_forward(hip_lib, variant, enc, dirs, W, seed)
            stats = _check_forward(sig, rgb, rows, f, rgb_ulps=2)
            worst = max(worst, stats["rgb_ulps"]); off.append(stats["rgb_off_share"])
    assert len(seen) == 32, "not every (coefficient, sign) pair reached an output"
    print("\nMLPEXACT sh rgb_ulps=%d rgb_off_share=%.5f" % (worst, float(np.mean(off))))


# ------------------------------------------------------------ 3d. edges ------------------------------------------------------------
@pytest.mark.parametrize("variant", ["natural_all_atomics", "pairs_list_ndev_slabs"])
def test_truncexp_clamp(hip_lib, variant):
    """h0 in {-16, -15, 0, 15, 16}: the forward's sigma is the unclamped exp(h0), the backward's d_enc follows exp(clamp(h0, -15, 15))."""
    enc, dirs, W, dsig, drgb = R.clamp_case()
    f = R.assert_exact(enc, dirs, W)
    assert set(f.h[:, 0]) >= {-16.0, -15.0, 0.0, 15.0, 16.0}
    b = R.backward(f, dsig, drgb)
    assert np.isfinite(b.d_enc).all() and np.abs(b.d_enc[:, 5]).max() > 1e4
    sig, rgb, rows = _run_forward(hip_lib, "ex_pairs" if variant.startswith("pairs") else "fwd", enc, dirs, W, 0)
    _check_forward(sig, rgb, rows, f)
    de, dW, flag = _run_backward(hip_lib, variant, enc, dirs, W, dsig, drgb, 0)
    stats = R.compare_backward(de, dW, b)
    assert flag == FLAG_SENT
    print("\nMLPEXACT clamp %s worst |err|/E: %s" % (variant, " ".join("%s=%.3f" % kv for kv in sorted(stats.items()))))


def _inf_cases(n):
    """(name, dsigma, drgb) on dyadic case 2: gradients that must, or must not, raise found_inf."""
    enc, dirs, W, f = _fwd_ref(2, n)
    dsig, drgb = R.gradients(2, n)
    out = [("finite", dsig, drgb)]
    d = dsig.copy(); d[n - 1] = np.inf
    out.append(("dsigma_inf_at_last_position", d, drgb))
    d = dsig.copy(); j = int(np.argmax(f.h[:, 0])); d[j] = np.float32(6.0e4)
    assert f.h[j, 0] >= 1.0 and float(d[j]) * np.exp(f.h[j, 0]) > 65520.0          # finite in f32, beyond fp16
    out.append(("dsigma_times_exp_overflows_fp16", d, drgb))
    c = drgb.copy(); c[n // 2, 1] = np.inf
    out.append(("drgb_inf", dsig, c))
    return enc, dirs, W, f, out


@pytest.mark.parametrize("variant", ["natural_all_atomics", "pairs_list_ndev_slabs", "natural_list_ndev_atomics"])
def test_found_inf_follows_the_reference(hip_lib, variant):
    """found_inf == "the model's d_enc or dW holds a non-finite value"; a clean run leaves a pre-set flag value untouched."""
    enc, dirs, W, f, cases = _inf_cases(47)
    for name, dsig, drgb in cases:
        b = R.backward(f, dsig, drgb)
        expect = not (np.isfinite(b.d_enc).all() and np.isfinite(b.dW).all())
        assert expect == (name != "finite"), name
        for preset in (0, FLAG_SENT):
            de, dW, flag = _run_backward(hip_lib, variant, enc, dirs, W, dsig, drgb, 2, flag=preset)
            assert flag == (1 if expect else preset), (name, preset, flag)
        R.compare_backward(de, dW, b)                   # finite elements still within the bound, non-finite ones non-finite


def test_zero_length_direction(hip_lib):
    """One sample with d = 0 among normal ones: its rgb is NaN (what d/|d| gives in torch), its sigma exact, every other sample as
    without it."""
    enc, dirs, W, f = _fwd_ref(1, 33)
    dirs0 = dirs.copy(); dirs0[7] = 0.0
    f0 = R.forward(enc, dirs0, W)
    assert np.isnan(f0.rgb[7]).all() and np.array_equal(np.delete(f0.rgb, 7, 0), np.delete(f.rgb, 7, 0))
    for variant in ("fwd", "ex_pairs", "list_natural"):
        sig, rgb, rows = _run_forward(hip_lib, variant, enc, dirs0, W, 1)
        sig1, rgb1, rows1 = _run_forward(hip_lib, variant, enc, dirs, W, 1)
        assert np.isnan(rgb[rows][7]).all(), (variant, rgb[rows][7])
        assert np.array_equal(sig, sig1), variant
        keep = np.delete(rows, 7)
        assert np.array_equal(rgb[keep], rgb1[keep]), variant
        _check_forward(sig, rgb, rows, f0)
