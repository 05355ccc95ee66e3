"""Double backward of the hash encoder on the GPU: ngp_hash_bwd2_gather_{f32,bf16} and ngp_hash_bwd2_table_f32 against the float64
reference (tests/hash_input_grad2_reference.py), element by element, to four times the error of a serial float32 evaluation of the
same formulas; the twice-differentiable encoder's autograd wiring; an end-to-end eikonal loss against torch's own double backward of a
plain-torch encoder; NGP.density_normals(create_graph=True); the example.

The yardstick is that of test_gpu_hash_input_grad.py, whose input this file reuses (1000 points, the first eight rows the fixed edge
cases, row 7 the NaN): per (level table, kind) the float64 outputs, their magnitude sums S and the serial float32 outputs are computed
once on the input with row 7 replaced by an ordinary point -- samples are independent, so every other row of the gather reference is
that of the input with the NaN, and the scatter reference has no row to leave out.  E32 = max |ref32 - ref64| / S per output; the
cases n in {1, 63, 64, 65, 1000} are prefixes and share it.  Each kernel must hold |gpu - ref64| <= 4 * E32 * S + tiny: the factor 4
is the first-order test's (a tree reduction and difference sums instead of the serial order; atomics in arrival order)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import hash_input_grad_reference as ref
import hash_input_grad2_reference as ref2
import test_gpu_hash_input_grad as t1
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = 1e-30
NS = t1.NS
CASES = [(shape, kind) for shape, kind in t1.CASES if kind in ("f32", "bf16")]
TABLES = ["default", "deploy", "tiny", "tiny_mod", "f1"]
ORDINARY = [0.25, 0.5, 0.75]                 # what replaces the NaN row
_cache = {}


def _input(shape, kind, constant=False):
    """The first-order test's input plus ddx, and the reference on it: computed once, never modified."""
    key = (shape, kind, constant)
    if key in _cache:
        return _cache[key]
    c1 = t1._input(shape, kind, constant)
    lv, x = c1["lv"], c1["x"]
    g = torch.Generator().manual_seed(1 + sum(map(ord, shape + kind)))
    ddx = torch.randn(t1.N_POINTS, 3, generator=g)
    x2 = x.copy()
    x2[7] = ORDINARY
    args = (x2, c1["table"].float().numpy(), c1["denc"].numpy(), ddx.numpy(), lv)
    d_denc, S_denc, d_x, S_x, _, _ = ref2.bwd2_64(*args)
    d_denc32, d_x32, d_table32 = ref2.bwd2_32(*args)
    assert np.all(S_denc > 0) and np.all(S_x > 0)
    c = dict(lv=lv, x=x, x2=x2, table=c1["table"], denc=c1["denc"], ddx=ddx, rows=c1["rows"], d_denc=d_denc, S_denc=S_denc, d_x=d_x,
             S_x=S_x, d_table32=d_table32, e32_denc=float(np.max(np.abs(d_denc32 - d_denc) / S_denc)),
             e32_x=float(np.max(np.abs(d_x32 - d_x) / S_x)))
    assert np.isfinite(c["e32_denc"]) and np.isfinite(c["e32_x"]) and (constant or c["e32_denc"] > 0) and c["e32_x"] > 0
    _cache[key] = c
    return c


def _gather(kind, x, table, denc, ddx, lv, **kw):
    from ngp_hip import ops
    fn = {"f32": ops.hash_bwd2_gather_f32, "bf16": ops.hash_bwd2_gather_bf16}[kind]
    out = fn(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), table.to(DEV), denc.contiguous().to(DEV), ddx.contiguous().to(DEV), lv, **kw)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gather_figures(shape, kind):
    """E32 of both outputs and the kernel's worst |gpu - ref64| / (E32 S) over the prefixes (the figures the test prints and
    profiles/microbench/hash_input_grad2.py records)."""
    c = _input(shape, kind)
    L_F = c["lv"].n_levels * c["lv"].n_features
    worst = {"d_denc": 0.0, "d_x": 0.0}
    for n in NS:
        d_denc, d_x = _gather(kind, c["x"][:n], c["table"], c["denc"][:n], c["ddx"][:n], c["lv"])
        assert d_denc.shape == (n, L_F) and d_x.shape == (n, 3)
        rows = c["rows"][:n]
        for name, got, want, S, e32 in (("d_denc", d_denc, c["d_denc"], c["S_denc"], c["e32_denc"]),
                                        ("d_x", d_x, c["d_x"], c["S_x"], c["e32_x"])):
            err = np.abs(got.astype(np.float64)[rows] - want[:n][rows])
            worst[name] = max(worst[name], float(np.max((err - TINY) / (e32 * S[:n][rows]))))
    return {"E32_d_denc": c["e32_denc"], "E32_d_x": c["e32_x"], "worst_d_denc_over_E32_S": worst["d_denc"],
            "worst_d_x_over_E32_S": worst["d_x"], "bound": 4.0}


@pytest.mark.parametrize("shape,kind", CASES)
def test_gather_against_float64(hip_lib, shape, kind):
    r = gather_figures(shape, kind)
    print("hash double backward gather %s/%s: E32 = %.3g (d_denc) %.3g (d_x), worst |gpu - ref64| / (E32 S) = %.3f (d_denc) %.3f (d_x), "
          "bound 4" % (shape, kind, r["E32_d_denc"], r["E32_d_x"], r["worst_d_denc_over_E32_S"], r["worst_d_x_over_E32_S"]))
    assert r["worst_d_denc_over_E32_S"] <= 4.0 and r["worst_d_x_over_E32_S"] <= 4.0, r


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_gather_nan_row_leaves_the_others_untouched(hip_lib, kind):
    """Row 7 is (NaN, 0.5, 0.5): no fault, and every other row has the bits it has with an ordinary point in row 7.  Its own d_denc row
    is NaN throughout; of its d_x row the y and z components are (d_x[0] is built from the y and z weights alone: the encoding is linear
    in x, so no mixed derivative with respect to x reads the x fraction)."""
    c = _input("default", kind)
    a = _gather(kind, c["x"], c["table"], c["denc"], c["ddx"], c["lv"])
    b = _gather(kind, c["x2"], c["table"], c["denc"], c["ddx"], c["lv"])
    rows = c["rows"]
    assert int((~rows).sum()) == 1 and not rows[7]
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u[rows]), _bits(v[rows]))
        assert np.all(np.isfinite(u[rows])) and np.all(np.isfinite(v))
    assert np.all(np.isnan(a[0][7])) and np.all(np.isnan(a[1][7, 1:]))


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_gather_twice_null_outputs_and_bf16(hip_lib, kind):
    """Two launches are bit-identical; a null d_denc or d_x leaves the other output's bits unchanged; the bf16 entry equals the f32
    entry on the rounded table bit for bit."""
    c = _input("default", kind)
    args = (c["x2"], c["table"], c["denc"], c["ddx"], c["lv"])
    a = _gather(kind, *args)
    b = _gather(kind, *args)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    only_x = _gather(kind, *args, need_denc=False)
    only_denc = _gather(kind, *args, need_x=False)
    assert only_x[0] is None and only_denc[1] is None
    assert np.array_equal(_bits(only_x[1]), _bits(a[1])) and np.array_equal(_bits(only_denc[0]), _bits(a[0]))
    if kind == "bf16":
        f = _gather("f32", c["x2"], c["table"].float(), c["denc"], c["ddx"], c["lv"])
        assert np.array_equal(_bits(a[0]), _bits(f[0])) and np.array_equal(_bits(a[1]), _bits(f[1]))


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_gather_exact_zeros(hip_lib, kind):
    """A constant table gives d_denc == 0 exactly (every corner difference is 0); ddx = e_k gives d_x[:, k] == 0 exactly."""
    c = _input("default", kind, constant=True)
    d_denc, _ = _gather(kind, c["x"], c["table"], c["denc"], c["ddx"], c["lv"])
    assert np.all(d_denc[c["rows"]] == 0)
    c = _input("default", kind)
    for k in range(3):
        e = torch.zeros(t1.N_POINTS, 3)
        e[:, k] = 1.0
        _, d_x = _gather(kind, c["x2"], c["table"], c["denc"], e, c["lv"])
        assert np.all(d_x[:, k] == 0) and np.any(d_x != 0)


# ------------------------------------------------------------------------------------------------ scatter
def _scatter(x, denc, ddx, lv, fill=0.0):
    from ngp_hip import ops
    dtable = torch.full((lv.total_entries * lv.n_features,), fill, device=DEV)
    out = ops.hash_bwd2_table_f32(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), denc.contiguous().to(DEV), ddx.contiguous().to(DEV), lv,
                                  dtable)
    torch.cuda.synchronize()
    assert out is dtable
    return dtable.cpu().numpy()


def _table_e32(c):
    """E32 of the scatter: the serial float32 accumulation (sample order) of the whole input against float64, over the touched entries."""
    if "e32_table" not in c:
        _, _, _, _, d_table, S_table = ref2.bwd2_64(c["x2"], c["table"].float().numpy(), c["denc"].numpy(), c["ddx"].numpy(), c["lv"])
        touched = S_table > 0
        assert np.all(c["d_table32"][~touched] == 0)
        c["e32_table"] = float(np.max(np.abs(c["d_table32"][touched] - d_table[touched]) / S_table[touched]))
        c["d_table"], c["S_table"] = d_table, S_table
        assert c["e32_table"] > 0
    return c["e32_table"]


def scatter_figures(shape):
    c = _input(shape, "f32")
    e32 = _table_e32(c)
    worst, worst_ones = 0.0, 0.0
    for n in NS:
        if n == t1.N_POINTS:
            d_table, S_table = c["d_table"], c["S_table"]
        else:
            _, _, _, _, d_table, S_table = ref2.bwd2_64(c["x2"][:n], c["table"].float().numpy(), c["denc"][:n].numpy(), c["ddx"][:n].numpy(),
                                                        c["lv"])
        touched = S_table > 0
        idx, _ = ref.corners(c["x2"][:n], c["lv"])
        F = c["lv"].n_features
        named = np.zeros(S_table.size // F, dtype=bool)
        named[idx.reshape(-1).astype(np.int64)] = True
        assert np.all(np.repeat(named, F)[touched])                 # S_table > 0 only on entries some corner of some sample names
        got = _scatter(c["x2"][:n], c["denc"][:n], c["ddx"][:n], c["lv"])
        assert np.all(_bits(got[~touched]) == 0)                    # untouched entries keep their bits
        err = np.abs(got.astype(np.float64)[touched] - d_table[touched])
        worst = max(worst, float(np.max((err - TINY) / (e32 * S_table[touched]))))
        if n == t1.N_POINTS:                                        # accumulation: onto 1.0, within the bound plus one ulp of 1
            ones = _scatter(c["x2"], c["denc"], c["ddx"], c["lv"], fill=1.0)
            assert np.all(_bits(ones[~touched]) == _bits(np.ones(1, np.float32))[0])
            err = np.abs(ones.astype(np.float64)[touched] - (1.0 + d_table[touched]))
            worst_ones = float(np.max((err - TINY - 2.0**-23) / (e32 * S_table[touched])))
    return {"E32_d_table": e32, "worst_over_E32_S": worst, "worst_onto_ones_over_E32_S_after_one_ulp": worst_ones, "bound": 4.0}


@pytest.mark.parametrize("shape", TABLES)
def test_scatter_against_float64(hip_lib, shape):
    r = scatter_figures(shape)
    print("hash double backward scatter %s: E32 = %.3g, worst |gpu - ref64| / (E32 S) = %.3f onto zeros, %.3f onto ones (after one ulp "
          "of 1), bound 4" % (shape, r["E32_d_table"], r["worst_over_E32_S"], r["worst_onto_ones_over_E32_S_after_one_ulp"]))
    assert r["worst_over_E32_S"] <= 4.0 and r["worst_onto_ones_over_E32_S_after_one_ulp"] <= 4.0, r


@pytest.mark.parametrize("shape", ["default", "deploy"])
def test_scatter_zero_rows_contribute_nothing(hip_lib, shape):
    """Rows whose ddx or whose denc is exactly 0: the entries only they name keep their bits, the others hold the bound."""
    c = _input(shape, "f32")
    e32 = _table_e32(c)
    ddx, denc = c["ddx"].clone(), c["denc"].clone()
    ddx[0::3] = 0.0
    denc[1::3] = 0.0
    _, _, _, _, d_table, S_table = ref2.bwd2_64(c["x2"], c["table"].float().numpy(), denc.numpy(), ddx.numpy(), c["lv"])
    touched = S_table > 0
    assert 0 < int(touched.sum()) < int((c["S_table"] > 0).sum())
    got = _scatter(c["x2"], denc, ddx, c["lv"], fill=1.0)
    assert np.all(_bits(got[~touched]) == _bits(np.ones(1, np.float32))[0])
    err = np.abs(got.astype(np.float64)[touched] - (1.0 + d_table[touched]))
    assert np.all(err <= 4 * e32 * S_table[touched] + TINY + 2.0**-23)


def test_domain_and_empty_input(hip_lib):
    """n == 0, a wrong-size table, F outside the forward's domain and host tensors behave as the first-order operators do."""
    from ngp_hip import ops
    lv = t1._levels("default")
    table = torch.zeros(lv.total_entries * 2, device=DEV)
    z3, z32 = torch.zeros(0, 3, device=DEV), torch.zeros(0, 32, device=DEV)
    d_denc, d_x = ops.hash_bwd2_gather_f32(z3, table, z32, z3, lv)
    assert tuple(d_denc.shape) == (0, 32) and tuple(d_x.shape) == (0, 3)
    ones = torch.ones_like(table)
    assert ops.hash_bwd2_table_f32(z3, z32, z3, lv, ones) is ones and bool((ones == 1).all())
    lv3 = ops.make_levels(2**10, 2, 4, 64, 3)
    x, t3, d3 = torch.rand(4, 3, device=DEV), torch.zeros(lv3.total_entries * 3, device=DEV), torch.zeros(4, 6, device=DEV)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.hash_bwd2_gather_f32(x, t3, d3, x, lv3)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.hash_bwd2_table_f32(x, d3, x, lv3, t3)
    d32 = torch.zeros(4, 32, device=DEV)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.hash_bwd2_gather_bf16(x, torch.zeros(lv3.total_entries * 3, device=DEV, dtype=torch.bfloat16), d3, x, lv3)
    for bad in ((x.cpu(), table, d32, x), (x, table.cpu(), d32, x), (x, table, d32.cpu(), x), (x, table, d32, x.cpu())):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.hash_bwd2_gather_f32(*bad, lv)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.hash_bwd2_table_f32(x, d32, x, lv, table.cpu())
    with pytest.raises(ValueError):
        ops.hash_bwd2_gather_f32(x, table[:-2], d32, x, lv)
    with pytest.raises(ValueError):
        ops.hash_bwd2_table_f32(x, d32, x, lv, table[:-2])
    with pytest.raises(ValueError):
        ops.hash_bwd2_gather_f32(x, table, d32, x[:3], lv)
    with pytest.raises(ValueError):
        ops.hash_bwd2_table_f32(x, d32[:3], x, lv, table)


# ------------------------------------------------------------------------------------------------ modules
def _encoder(kind, twice):
    from modules.hash_encoder import HashEncoder
    torch.manual_seed(3)
    return HashEncoder(table_dtype=torch.bfloat16 if kind == "bf16" else None, twice_differentiable=twice).to(DEV)


def _lattice(lv):
    """The 64 points of test_module_without_position_grad_is_unchanged: distinct cells on every level, no table entry named more than
    twice, so a float-atomic scatter does not depend on arrival order."""
    k = np.arange(4, dtype=np.float32)
    lattice = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3) * np.float32(0.25) + np.float32(0.1)
    xn = (lattice + np.random.default_rng(9).random((64, 3), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    idx, _ = ref.corners(xn, lv)
    assert np.bincount(idx.reshape(-1).astype(np.int64)).max() <= 2
    return xn


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_first_order_is_bit_identical_to_the_default_encoder(hip_lib, kind):
    a, b = _encoder(kind, False), _encoder(kind, True)
    assert torch.equal(a.hash_table, b.hash_table) and b.twice_differentiable and not a.twice_differentiable
    g = torch.randn(64, a.out_dim, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    res = []
    for enc in (a, b):
        x = torch.from_numpy(_lattice(enc.levels_struct)).to(DEV).requires_grad_()
        out = enc(x)
        out.backward(g)
        res.append((out.detach(), x.grad, enc.hash_table.grad))
    for u, v in zip(*res):
        assert u is not None and torch.equal(u, v) and bool(u.abs().sum() > 0)
    # without a position gradient: the table gradient alone, same bits again
    x = torch.from_numpy(_lattice(b.levels_struct)).to(DEV)
    b.hash_table.grad = None
    b(x).backward(g)
    assert torch.equal(b.hash_table.grad, res[0][2])
    # 1000 random points: out and x.grad do not depend on any summation order
    x1 = torch.rand(1000, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    g1 = torch.randn(1000, a.out_dim, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    grads = []
    for enc in (a, b):
        x = x1.clone().requires_grad_()
        out = enc(x)
        out.backward(g1)
        grads.append((out.detach(), x.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_double_backward_is_the_operators(hip_lib, kind):
    from ngp_hip import ops
    enc = _encoder(kind, True)
    lv = enc.levels_struct
    x = torch.from_numpy(_lattice(lv)).to(DEV).requires_grad_()
    g = torch.randn(64, enc.out_dim, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    (gx,) = torch.autograd.grad((enc(x) * g).sum(), x, create_graph=True)
    assert gx.requires_grad
    (gx ** 2).sum().backward()
    ddx = (2 * gx).detach()
    want_table = ops.hash_bwd2_table_f32(x.detach(), g, ddx, lv, torch.zeros_like(enc.hash_table))
    if kind == "bf16":
        _, want_x = ops.hash_bwd2_gather_bf16(x.detach(), enc.table_bf16(), g, ddx, lv, need_denc=False)
    else:
        _, want_x = ops.hash_bwd2_gather_f32(x.detach(), enc.hash_table.detach(), g, ddx, lv, need_denc=False)
    assert torch.equal(enc.hash_table.grad, want_table) and bool(want_table.abs().sum() > 0)
    assert torch.equal(x.grad, want_x) and bool(want_x.abs().sum() > 0)


def test_table_gradient_is_not_differentiable_and_default_is_once(hip_lib):
    enc = _encoder("f32", True)
    x = torch.rand(16, 3, device=DEV).requires_grad_()
    (gt,) = torch.autograd.grad((enc(x) ** 2).sum(), enc.hash_table, create_graph=True)
    assert not gt.requires_grad and bool(gt.abs().sum() > 0)
    enc0 = _encoder("f32", False)
    (gx,) = torch.autograd.grad((enc0(x) ** 2).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ------------------------------------------------------------------------------------------------ end to end
def _eikonal_grads(encode, table, w1, w2, x):
    """hash_table.grad and the two weight grads of ((|grad_x f| - 1)^2).mean() + (f^2).mean(), f = tanh(enc(x) w1^T) w2^T."""
    x = x.clone().requires_grad_()
    f = (torch.tanh(encode(x) @ w1.t()) @ w2.t()).squeeze(1)
    (gx,) = torch.autograd.grad(f.sum(), x, create_graph=True)
    loss = ((torch.linalg.norm(gx, dim=1) - 1) ** 2).mean() + (f ** 2).mean()
    return torch.autograd.grad(loss, (table, w1, w2))


def e2e_figures(shape):
    """Per tensor: |gpu - ref64|_inf, |TorchEncoder(float32) - ref64|_inf and their ratio (the test's bound is 4)."""
    from modules.hash_encoder import HashEncoder
    torch.manual_seed(5)
    enc = HashEncoder(*t1.SHAPES[shape][:4], feature_per_level=t1.SHAPES[shape][4], twice_differentiable=True).to(DEV)
    lv = enc.levels_struct
    gen = torch.Generator().manual_seed(6)
    x = torch.rand(256, 3, generator=gen)
    w1 = torch.randn(16, enc.out_dim, generator=gen) * (0.5 / enc.out_dim ** 0.5)
    w2 = torch.randn(1, 16, generator=gen) * 0.25
    table = enc.hash_table.detach().cpu()
    res = {}
    for name, dtype in (("ref64", torch.float64), ("ref32", torch.float32)):
        t_, a_, b_ = (v.to(dtype).requires_grad_() for v in (table, w1, w2))
        E = ref2.TorchEncoder(lv, dtype)
        res[name] = [v.double() for v in _eikonal_grads(lambda p: E(p, t_), t_, a_, b_, x.to(dtype))]
    a_, b_ = w1.to(DEV).requires_grad_(), w2.to(DEV).requires_grad_()
    res["gpu"] = [v.double().cpu() for v in _eikonal_grads(enc, enc.hash_table, a_, b_, x.to(DEV))]
    out = {}
    for i, name in enumerate(("hash_table", "w1", "w2")):
        e_gpu = float((res["gpu"][i].view(-1) - res["ref64"][i].view(-1)).abs().max())
        e_32 = float((res["ref32"][i].view(-1) - res["ref64"][i].view(-1)).abs().max())
        out[name] = {"gpu_error_inf": e_gpu, "float32_torch_error_inf": e_32, "ratio": e_gpu / e_32,
                     "ref64_inf": float(res["ref64"][i].abs().max()), "bound": 4.0}
    return out


@pytest.mark.parametrize("shape", ["tiny", "default"])
def test_end_to_end_eikonal_loss(hip_lib, shape):
    r = e2e_figures(shape)
    for name, v in r.items():
        print("eikonal end to end %s %s: |gpu - ref64| = %.3g, |float32 torch - ref64| = %.3g, ratio %.3f (bound 4), |ref64| = %.3g"
              % (shape, name, v["gpu_error_inf"], v["float32_torch_error_inf"], v["ratio"], v["ref64_inf"]))
    for name, v in r.items():
        assert v["ref64_inf"] > 0 and v["float32_torch_error_inf"] > 0
        assert v["gpu_error_inf"] <= 4 * v["float32_torch_error_inf"], (name, v)


# ------------------------------------------------------------------------------------------------ NGP.density_normals
@pytest.mark.parametrize("config", ["f32", "bf16", "f32_autocast"])
def test_density_normals_create_graph(hip_lib, config):
    from modules.networks import NGP
    torch.manual_seed(4)
    kind, _, ac = config.partition("_")
    model = NGP(scale=0.5, table_dtype=torch.bfloat16 if kind == "bf16" else None, twice_differentiable=True).to(DEV)
    x = torch.rand(500, 3, device=DEV) - 0.5
    with torch.autocast("cuda", dtype=torch.float16, enabled=bool(ac)):
        sigmas, normals, grad = model.density_normals(x, create_graph=True)
        assert sigmas.requires_grad and normals.requires_grad and grad.requires_grad
        ((normals ** 2).sum() + grad.sum()).backward()
    params = [model.pos_encoder.hash_table] + list(model.xyz_encoder.parameters())
    for p in params:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0)
    assert bool(torch.isfinite(sigmas).all()) and bool(torch.isfinite(normals).all()) and bool(torch.isfinite(grad).all())
    # on x itself where x requires grad: the loss reaches it
    xg = x.clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16, enabled=bool(ac)):
        _, _, grad = model.density_normals(xg, create_graph=True)
        (grad ** 2).sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.abs().sum() > 0)
    # the default call is unchanged: no graph
    s0, n0, g0 = model.density_normals(x)
    assert not (s0.requires_grad or n0.requires_grad or g0.requires_grad)


def test_density_normals_create_graph_needs_the_flag(hip_lib):
    from modules.networks import NGP
    x = torch.rand(8, 3, device=DEV) - 0.5
    with pytest.raises(ValueError, match="twice"):
        NGP(scale=0.5).to(DEV).density_normals(x, create_graph=True)
    with pytest.raises(ValueError, match="twice_differentiable"):
        NGP(scale=0.5, half_opt=True, twice_differentiable=True)
    with pytest.raises(ValueError, match="twice_differentiable"):
        NGP(scale=0.5, pos_encoder_type="triplane", max_res=64, twice_differentiable=True)


def test_example_fits_with_the_eikonal_term(hip_lib):
    spec = importlib.util.spec_from_file_location("fit_sdf_eikonal", os.path.join(ROOT, "examples", "fit_sdf_eikonal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    info = mod.main(["--steps", "50", "--n", "2048", "--log2_T", "14", "--levels", "8", "--max_res", "256", "--sdf_weight", "0"])
    for key in ("sdf_loss_first", "sdf_loss_last", "eikonal_error_first", "eikonal_error_last", "loss_first", "loss_last"):
        assert np.isfinite(info[key]), (key, info)
    assert info["table_grad_nonzero"]
    assert info["eikonal_error_last"] < info["eikonal_error_first"], info
