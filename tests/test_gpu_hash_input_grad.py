"""Position gradient of the hash encoder on the GPU: ngp_hash_bwd_input_{f32,bf16,f16} against the float64 reference
(tests/hash_input_grad_reference.py), element by element, to four times the error of a serial float32 evaluation of the same formula;
the encoders' autograd wiring; NGP.density_normals; the example.

The yardstick.  For every (level table, entry) one input of 1000 points is drawn once; dx64, the magnitude sum S and the serial float32
dx32 are computed on it once, and E32 = max over its elements of |dx32 - dx64| / S.  The cases n in {1, 63, 64, 65, 1000} are prefixes of
that input (its first rows are the fixed edge cases), so they share the reference and the same E32 -- the error the reference's own
float32 evaluation makes on this input, not something read off the kernel.  The kernel must hold |gpu - dx64| <= 4 * E32 * S + tiny:
the factor 4 because its level reduction is a tree and its per-axis sums are differences of corner pairs, not the serial order."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import hash_input_grad_reference as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = 1e-30
N_POINTS = 1000
NS = (1, 63, 64, 65, 1000)          # wave tails, and sample groups on both sides of a wave boundary
SHAPES = {
    "default": (2**19, 16, 16, 2048, 2),
    "deploy": (2**21, 4, 32, 128, 4),
    "tiny": (2**10, 2, 4, 64, 2),          # level 0 dense (conditional subtract; real modulo for the outside point), level 1 hashed (mask)
    "tiny_mod": (1000, 2, 4, 64, 2),       # a hashed level whose size is no power of two: the real modulo
    "f1": (2**14, 5, 8, 300, 1),
}
CASES = [("default", "f32"), ("default", "bf16"), ("default", "f16"), ("deploy", "f32"), ("tiny", "f32"), ("tiny", "bf16"),
         ("tiny", "f16"), ("tiny_mod", "f32"), ("f1", "f32")]
_cache = {}


def _levels(shape):
    from ngp_hip import ops
    return ops.make_levels(*SHAPES[shape])


def _points(lv, seed):
    """[N_POINTS, 3] float32 in [0, 1); the first rows are the fixed edge cases (row 7 carries the NaN)."""
    x = np.random.default_rng(seed).random((N_POINTS, 3), dtype=np.float32)
    top = np.float32(lv.scale[lv.n_levels - 1])
    grid = np.float32((np.floor(top / 2) - np.float32(0.5)) / top)            # pos = x * scale + 0.5 lands on a grid point of the top level
    x[:8] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [grid, grid, grid], [1e-7, 1e-7, 1e-7], [0.999999, 0.999999, 0.999999],
             [1.25, -0.25, 3.0], [np.nan, 0.5, 0.5]]
    return x


def _input(shape, kind, constant=False):
    """The shared input and reference of one (level table, entry): computed once, never modified."""
    key = (shape, kind, constant)
    if key in _cache:
        return _cache[key]
    lv = _levels(shape)
    g = torch.Generator().manual_seed(sum(map(ord, shape + kind)))
    n_table = lv.total_entries * lv.n_features
    table = torch.full((n_table,), 0.75) if constant else torch.randn(n_table, generator=g)
    denc = torch.randn(N_POINTS, lv.n_levels * lv.n_features, generator=g)
    if kind == "bf16":
        table = table.bfloat16()
    elif kind == "f16":
        table, denc = table.half().reshape(-1, 2), denc.half().reshape(N_POINTS, lv.n_levels, 2)
    x = _points(lv, 5)
    args = (x, table.float().numpy(), denc.float().numpy(), lv)
    dx64, S = ref.grad64(*args, half=kind == "f16")
    dx32 = ref.grad32(*args, half=kind == "f16")
    rows = ~np.isnan(x).any(1)
    e32 = float(np.max(np.abs(dx32[rows] - dx64[rows]) / S[rows]))
    assert np.all(S[rows] > 0) and np.isfinite(e32)
    _cache[key] = dict(lv=lv, x=x, table=table, denc=denc, dx64=dx64, S=S, e32=e32, rows=rows)
    return _cache[key]


def _run(kind, x, table, denc, lv):
    from ngp_hip import ops
    fn = {"f32": ops.hash_bwd_input_f32, "bf16": ops.hash_bwd_input_bf16, "f16": ops.hash_bwd_input_f16}[kind]
    return fn(torch.from_numpy(x).to(DEV), table.to(DEV), denc.contiguous().to(DEV), lv)


@pytest.mark.parametrize("shape,kind", CASES)
def test_kernel_against_float64(hip_lib, shape, kind):
    c = _input(shape, kind)
    worst = 0.0
    for n in NS:
        got = _run(kind, c["x"][:n], c["table"], c["denc"][:n], c["lv"])
        torch.cuda.synchronize()
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == (n, 3)
        rows = c["rows"][:n]
        err = np.abs(got[rows] - c["dx64"][:n][rows])
        tol = 4 * c["e32"] * c["S"][:n][rows] + TINY
        worst = max(worst, float(np.max(err / (c["e32"] * c["S"][:n][rows]))))
        assert np.all(err <= tol), (n, float(np.max(err / tol)))
    print("hash input grad %s/%s: E32 = %.3g, worst |gpu - dx64| / (E32 S) = %.3f (bound 4)" % (shape, kind, c["e32"], worst))


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_nan_row_leaves_the_others_untouched(hip_lib, kind):
    """Row 7 is NaN: no fault, and every other row has the bits it has when the NaN row is replaced by an ordinary point."""
    c = _input("default", kind)
    x2 = c["x"].copy()
    x2[7] = [0.25, 0.5, 0.75]
    a = _run(kind, c["x"], c["table"], c["denc"], c["lv"]).cpu().numpy()
    b = _run(kind, x2, c["table"], c["denc"], c["lv"]).cpu().numpy()
    rows = c["rows"]
    assert np.array_equal(a[rows].view(np.uint32), b[rows].view(np.uint32))
    assert np.all(np.isfinite(a[rows])) and np.all(np.isfinite(b))


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_constant_table_cancels(hip_lib, kind):
    c = _input("default", kind, constant=True)
    got = _run(kind, c["x"], c["table"], c["denc"], c["lv"]).cpu().numpy().astype(np.float64)
    rows = c["rows"]
    assert np.all(np.abs(got[rows]) <= 4 * c["e32"] * c["S"][rows] + TINY), (c["e32"], float(np.max(np.abs(got[rows]) / c["S"][rows])))


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_two_launches_are_bit_identical(hip_lib, kind):
    c = _input("default", kind)
    a = _run(kind, c["x"], c["table"], c["denc"], c["lv"]).cpu().numpy()
    b = _run(kind, c["x"], c["table"], c["denc"], c["lv"]).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bf16_entry_equals_f32_entry_on_the_rounded_table(hip_lib):
    c = _input("default", "bf16")
    a = _run("bf16", c["x"], c["table"], c["denc"], c["lv"]).cpu().numpy()
    b = _run("f32", c["x"], c["table"].float(), c["denc"], c["lv"]).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_domain_and_empty_input(hip_lib):
    """n == 0 returns an empty [0,3] tensor; F outside the forward's domain is the forward's error; CPU tensors are refused."""
    from ngp_hip import ops
    lv = _levels("default")
    table = torch.zeros(lv.total_entries * 2, device=DEV)
    assert tuple(ops.hash_bwd_input_f32(torch.zeros(0, 3, device=DEV), table, torch.zeros(0, 32, device=DEV), lv).shape) == (0, 3)
    lv3 = ops.make_levels(2**10, 2, 4, 64, 3)
    x, t3, d3 = torch.rand(4, 3, device=DEV), torch.zeros(lv3.total_entries * 3, device=DEV), torch.zeros(4, 6, device=DEV)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.hash_fwd_f32(x, t3, lv3)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.hash_bwd_input_f32(x, t3, d3, lv3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.hash_bwd_input_f32(torch.zeros(4, 3), table, torch.zeros(4, 32, device=DEV), lv)
    with pytest.raises(ValueError):
        ops.hash_bwd_input_f32(torch.rand(4, 3, device=DEV), table[:-2], torch.zeros(4, 32, device=DEV), lv)


# ------------------------------------------------------------------------------------------------ modules
def _encoder(kind):
    torch.manual_seed(3)
    if kind == "half":
        from modules.hash_encoder_half import HashEncoder
        return HashEncoder().to(DEV)
    from modules.hash_encoder import HashEncoder
    return HashEncoder(table_dtype=torch.bfloat16 if kind == "bf16" else None).to(DEV)


@pytest.mark.parametrize("kind", ["f32", "bf16", "half"])
def test_module_position_gradient_is_the_operator(hip_lib, kind):
    from ngp_hip import ops
    enc = _encoder(kind)
    x = torch.rand(1000, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1)).requires_grad_()
    out = enc(x)
    g = torch.randn(out.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(2)).to(out.dtype)
    out.backward(g)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    lv = enc.levels_struct
    if kind == "f32":
        want = ops.hash_bwd_input_f32(x.detach(), enc.hash_table.detach(), g, lv)
    elif kind == "bf16":
        want = ops.hash_bwd_input_bf16(x.detach(), enc.table_bf16(), g, lv)
    else:
        want = ops.hash_bwd_input_f16(x.detach(), enc.hash_table.detach().half(), g, lv)
    assert torch.equal(x.grad, want) and bool(x.grad.abs().sum() > 0)
    assert enc.hash_table.grad is not None and bool(enc.hash_table.grad.abs().sum() > 0)     # the table still gets its gradient


@pytest.mark.parametrize("kind", ["f32", "bf16", "half"])
def test_module_without_position_grad_is_unchanged(hip_lib, kind, monkeypatch):
    """Positions that do not require grad: the new operators are never called, and output and hash_table.grad have the bits of the
    forward and scatter-add operators called directly.  The 64 points sit in distinct cells of every level and no table entry
    receives more than two contributions (checked below), so the float-atomic scatter-add does not depend on arrival order."""
    from ngp_hip import ops
    enc = _encoder(kind)
    lv = enc.levels_struct
    k = np.arange(4, dtype=np.float32)
    lattice = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3) * np.float32(0.25) + np.float32(0.1)
    xn = (lattice + np.random.default_rng(9).random((64, 3), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    idx, _ = ref.corners(xn, lv, half=kind == "half")
    assert np.bincount(idx.reshape(-1).astype(np.int64)).max() <= 2
    x = torch.from_numpy(xn).to(DEV)

    def forbidden(*a, **kw):
        raise AssertionError("the position-gradient operator ran although the positions do not require grad")
    for name in ("hash_bwd_input_f32", "hash_bwd_input_bf16", "hash_bwd_input_f16"):
        monkeypatch.setattr(ops, name, forbidden)
    out = enc(x)
    g = torch.randn(out.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(2)).to(out.dtype)
    out.backward(g)
    assert x.grad is None
    if kind == "half":
        table_h = enc.hash_table.detach().half().contiguous()
        out_d = ops.hash_fwd_f16(x, table_h, lv).view(64, -1)
        grad_d = ops.hash_bwd_f16(x, g.contiguous(), lv, torch.zeros_like(table_h)).float()
    else:
        out_d = ops.hash_fwd_bf16(x, enc.table_bf16(), lv) if kind == "bf16" else ops.hash_fwd_f32(x, enc.hash_table.detach(), lv)
        grad_d = ops.hash_bwd_f32(x, g.contiguous(), lv, torch.zeros_like(enc.hash_table))
    assert torch.equal(out, out_d)
    assert torch.equal(enc.hash_table.grad, grad_d.view_as(enc.hash_table.grad))


def test_backward_is_once_differentiable(hip_lib):
    enc = _encoder("f32")
    x = torch.rand(16, 3, device=DEV).requires_grad_()
    (gx,) = torch.autograd.grad((enc(x) ** 2).sum(), x, create_graph=True)      # the incoming gradient 2 * enc carries a graph
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


@pytest.mark.parametrize("config", ["f32", "f32_autocast", "bf16_autocast", "half_autocast"])
def test_density_normals(hip_lib, config):
    from modules.networks import NGP
    torch.manual_seed(4)
    kind, _, ac = config.partition("_")
    model = NGP(scale=0.5, half_opt=kind == "half", table_dtype=torch.bfloat16 if kind == "bf16" else None).to(DEV)
    x = torch.rand(500, 3, device=DEV) - 0.5
    eps = 1e-20
    with torch.autocast("cuda", dtype=torch.float16, enabled=bool(ac)):
        with torch.no_grad():                                      # evaluation code calls it like this
            sigmas, normals, grad = model.density_normals(x, eps=eps)
        xg = x.clone().requires_grad_()
        s_manual = model.density(xg)
        (g_manual,) = torch.autograd.grad(s_manual.sum(), xg)
    assert all(p.grad is None for p in model.parameters())
    assert not (sigmas.requires_grad or normals.requires_grad or grad.requires_grad)
    assert sigmas.shape == (500,) and normals.shape == grad.shape == (500, 3)
    assert torch.equal(grad, g_manual) and torch.equal(sigmas, s_manual.detach())
    assert bool(torch.isfinite(normals).all()) and bool(torch.isfinite(grad).all())
    norm = torch.linalg.norm(grad.double(), dim=1)
    has = norm > eps
    assert int(has.sum()) > 400                                   # a fresh model has a gradient almost everywhere
    # unit length to float32 rounding of a 3-term norm and a division (a few 2^-24)
    assert bool(((torch.linalg.norm(normals.double(), dim=1) - 1).abs()[has] <= 1e-6).all())
    assert torch.equal(normals, -grad / torch.linalg.norm(grad, dim=1, keepdim=True).clamp_min(eps))


def test_density_normals_refuses_models_without_a_position_gradient(hip_lib):
    from modules.networks import NGP, VoxelGrid
    x = torch.rand(8, 3, device=DEV) - 0.5
    with pytest.raises(NotImplementedError, match="position gradient"):
        NGP(scale=0.5, pos_encoder_type="triplane", max_res=64).to(DEV).density_normals(x)
    with pytest.raises(NotImplementedError, match="position gradient"):
        VoxelGrid(scale=0.5, grid_size=16).to(DEV).density_normals(x)


@pytest.mark.parametrize("train_steps", [0, 16])
def test_example_renders_a_normal_map(hip_lib, tmp_path, train_steps):
    spec = importlib.util.spec_from_file_location("render_normals", os.path.join(ROOT, "examples", "render_normals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / "normals")
    info = mod.main(["--wh", "32", "--train_steps", str(train_steps), "--train_views", "4", "--train_wh", "32", "--out", out])
    img = np.load(out + ".npy")
    assert img.shape == (32, 32, 3) and img.dtype == np.float32 and np.isfinite(img).all()
    assert info["samples"] > 0 and info["finite"] and float(img.max()) > 0
    assert np.all(img >= 0) and np.all(img <= 1 + 1e-5)
    for path in info["out"]:
        assert os.path.getsize(path) > 0
