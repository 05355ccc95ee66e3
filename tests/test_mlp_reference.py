"""tests/mlp_reference.py itself (CPU): with the roundings off it is the module's own formulation in double; the dyadic cases
tests/test_gpu_mlp_exact.py uses are exact and cover every weight; the compare functions that file calls reject subtly wrong kernels
(mutated copies of the model) and accept another legitimate accumulation."""
import numpy as np
import pytest
import torch

import mlp_reference as R
import test_gpu_mlp_exact as G


def _random_problem(n=257, seed=0):
    rng = np.random.default_rng(seed)
    W = [rng.standard_normal(s) * 0.35 for s in R.SHAPES]
    W[1][0] *= 4.0                                     # h0 well beyond +-15 for some samples: the clamp matters
    enc = rng.standard_normal((n, 32))
    dirs = rng.standard_normal((n, 3)).astype(np.float32)
    return enc, dirs, W, rng.standard_normal(n), rng.standard_normal((n, 3))


def test_unrounded_model_is_the_modules_formulation_in_double():
    """round=False against torch float64 autograd through the layers of modules/networks.py (MLP, TruncExp; the SH values enter as
    constants, DirEncoder being a GPU operator): forward, d_enc, all five dW, and the clamp."""
    from modules.networks import MLP, TruncExp
    enc, dirs, W, dsig, drgb = _random_problem()
    f = R.forward(enc, dirs, W, round=False)
    b = R.backward(f, dsig, drgb)
    assert np.abs(f.h[:, 0]).max() > 15.5 and np.abs(f.h[:, 0]).min() < 1.0
    xyz = MLP(input_dim=32, output_dim=16, net_depth=1, net_width=64, bias_enabled=False).double()
    rgb = MLP(input_dim=32, output_dim=3, net_depth=2, net_width=64, bias_enabled=False, output_activation=torch.nn.Sigmoid()).double()
    layers = [xyz.hidden_layers[0], xyz.output_layer, rgb.hidden_layers[0], rgb.hidden_layers[1], rgb.output_layer]
    with torch.no_grad():
        for layer, w in zip(layers, W):
            layer.weight.copy_(torch.from_numpy(w))
    e = torch.from_numpy(enc).requires_grad_(True)
    h = xyz(e)
    sigma = TruncExp.apply(h[:, 0])
    c = rgb(torch.cat([torch.from_numpy(R.sh16(dirs, np.float64)), h], 1))
    torch.autograd.backward([sigma, c], [torch.from_numpy(dsig), torch.from_numpy(drgb)])

    def close(a, t, what):
        t = t.detach().numpy()
        assert np.abs(a - t).max() <= 1e-12 * max(1.0, np.abs(t).max()), what
    close(f.sigma, sigma, "sigma"); close(f.rgb, c, "rgb"); close(b.d_enc, e.grad, "d_enc")
    for k, layer in enumerate(layers):
        close(b.dWs[k], layer.weight.grad, "dW%d" % (k + 1))
        assert np.array_equal(b.dW[R.OFFS[k]:R.OFFS[k + 1]].reshape(R.SHAPES[k]), b.dWs[k])
    # without the clamp the same gradients are different: the comparison above does test it
    assert np.abs(R.backward(f, dsig, drgb, mut=[("no_clamp",)]).d_enc - b.d_enc).max() > 1.0


def test_pair_layout_round_trip():
    enc = np.arange(5 * 32, dtype=np.float32).reshape(5, 32)
    planes = R.to_pairs(enc, 9, fill=-1)
    assert planes.shape == (8, 9, 4) and np.all(planes[:, 5:] == -1)
    assert np.array_equal(planes[3, 2], [enc[2, 6], enc[2, 7], enc[2, 24], enc[2, 25]])
    assert np.array_equal(R.from_pairs(planes, 5), enc)
    assert torch.equal(R.to_pairs(torch.from_numpy(enc), 9, fill=-1), torch.from_numpy(planes))


def test_cases_cover_every_weight_and_the_mask_edge():
    """Section 2's conditions: over the cases the GPU file runs at its small sizes (for both packers: the layouts loop over the same
    cases) every weight position is non-zero at least once; about half of the hidden units are inactive and a visible share of the
    pre-activations is exactly 0."""
    for n in G.FWD_N[:-1] + G.BWD_N[:-1]:
        assert G._cases(n, 0) == list(range(R.N_CASES))
    hit = [np.zeros(s, bool) for s in R.SHAPES]
    for case in range(R.N_CASES):
        W = R.dyadic_weights(case)
        assert not W[2][:, :16].any()
        for k in range(5):
            hit[k] |= W[k] != 0
            assert np.array_equal(np.float16(W[k]).astype(np.float32), W[k])
        f = R.dyadic_case(case, 193)[3]
        for a, z in (("a1", "z1"), ("a3", "z3"), ("a4", "z4")):
            assert 0.35 < np.mean(f[a] <= 0) < 0.65, (case, a)
            assert np.mean(f[z] == 0) > 0.002, (case, z)
    hit[2] = hit[2][:, 16:]
    assert all(h.all() for h in hit)
    seen = set()
    for seed in range(R.SH_SEEDS):
        seen.update((u % 16, u < 16) for u in R.sh_case(seed)[3])
    assert len(seen) == 32


@pytest.mark.parametrize("n", sorted(set(G.FWD_N + G.BWD_N)), ids=G._n_id)
def test_every_case_the_gpu_file_uses_is_exact(n):
    """dyadic_case asserts it: rounded and unrounded pre-activations identical; _bwd_ref asserts that the bound is not vacuous."""
    for k in range(len(G.BIG_CASES)):
        for case in G._cases(n, k):
            G._fwd_ref(case, n)
            if n in G.BWD_N:
                G._bwd_ref(case, n)


# ---- the comparison would catch a subtly wrong kernel ----
N_MUT, CASE_MUT = 47, 0


def _truth():
    return G._bwd_ref(CASE_MUT, N_MUT)


def _caught(f_got, b_got, ref_f, ref_b):
    """Do the compare functions of the GPU tests reject this "kernel"?  -> the names of the comparisons that do."""
    out = []
    try:
        R.compare_forward(f_got.sigma.astype(np.float32), f_got.rgb.astype(np.float16), ref_f)
    except AssertionError:
        out.append("forward")
    try:
        R.compare_backward(b_got.d_enc.astype(np.float32), b_got.dW.astype(np.float32), ref_b)
    except AssertionError:
        out.append("backward")
    return out


def _rerun(enc, dirs, W, dsig, drgb, fmut=(), bmut=()):
    f = R.forward(enc, dirs, W, mut=fmut)
    return f, R.backward(f, dsig, drgb, mut=bmut)


def test_the_unmutated_model_passes_its_own_comparison():
    enc, dirs, W, f, dsig, drgb, b = _truth()
    assert _caught(f, b, f, b) == []


def test_mutant_two_w1_columns_swapped():
    enc, dirs, W, f, dsig, drgb, b = _truth()
    W1 = W[0].copy(); W1[:, [3, 4]] = W1[:, [4, 3]]
    assert set(_caught(*_rerun(enc, dirs, [W1] + W[1:], dsig, drgb), f, b)) == {"forward", "backward"}


def test_mutant_pair_planes_exchanged():
    enc, dirs, W, f, dsig, drgb, b = _truth()
    p = 2
    planes = R.to_pairs(enc, N_MUT)
    planes[[p, 7 - p]] = planes[[7 - p, p]]                                # the kernel reads plane 7-p where it wants plane p
    assert "forward" in _caught(*_rerun(R.from_pairs(planes, N_MUT), dirs, W, dsig, drgb), f, b)
    planes = R.to_pairs(enc, N_MUT)
    planes[p] = planes[p][:, [2, 3, 0, 1]]                                 # level p and level 15-p exchanged inside plane p
    assert "forward" in _caught(*_rerun(R.from_pairs(planes, N_MUT), dirs, W, dsig, drgb), f, b)


def test_mutant_hidden_feature_pair_permuted_between_layers():
    enc, dirs, W, f, dsig, drgb, b = _truth()
    assert _caught(*_rerun(enc, dirs, W, dsig, drgb, fmut=[("a1_swap", 20, 36)]), f, b) != []


def test_mutant_mask_taken_as_greater_or_equal():
    enc, dirs, W, f, dsig, drgb, b = _truth()
    assert _caught(*_rerun(enc, dirs, W, dsig, drgb, bmut=[("mask_ge",)]), f, b) == ["backward"]


def test_mutant_clamp_removed():
    enc, dirs, W, dsig, drgb = R.clamp_case()
    f = R.forward(enc, dirs, W)
    b = R.backward(f, dsig, drgb)
    assert _caught(f, b, f, b) == []
    assert _caught(f, R.backward(f, dsig, drgb, mut=[("no_clamp",)]), f, b) == ["backward"]


def _dw_of(rows):
    enc, dirs, W, f, dsig, drgb, b = _truth()
    return _rerun(enc[rows], dirs[rows], W, dsig[rows], drgb[rows])[1].dW


def _with_dw(b, dW):
    got = R.Bag(b)
    got.dW = dW
    return got


def test_mutant_last_sample_dropped_from_dw():
    enc, dirs, W, f, dsig, drgb, b = _truth()
    assert _caught(f, _with_dw(b, _dw_of(np.arange(N_MUT - 1))), f, b) == ["backward"]


def test_mutant_padded_positions_contribute_sample_zero():
    enc, dirs, W, f, dsig, drgb, b = _truth()
    pads = -N_MUT % 32
    assert pads > 0
    assert _caught(f, _with_dw(b, b.dW + pads * _dw_of(np.array([0]))), f, b) == ["backward"]


def test_mutant_one_list_entry_processed_twice():
    enc, dirs, W, f, dsig, drgb, b = _truth()
    j = int(np.nonzero(np.any(drgb != 0, axis=1))[0][20])                  # an entry in the middle that carries a gradient
    assert _caught(f, _with_dw(b, b.dW + _dw_of(np.array([j]))), f, b) == ["backward"]


@pytest.mark.parametrize("n", G.BWD_N, ids=G._n_id)
def test_another_accumulation_passes(n):
    """binary32 matmuls with every contraction (the samples of dW included) walked in reversed order, and an f32 sigmoid."""
    for case in G._cases(n, 0):
        enc, dirs, W, f, dsig, drgb, b = G._bwd_ref(case, n)
        f2 = R.forward(enc, dirs, W, accum="f32rev")
        assert _caught(f2, R.backward(f2, dsig, drgb), f, b) == [], case
