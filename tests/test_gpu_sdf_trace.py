"""csrc/sdf_trace.hip (ngp_sdf_eval, ngp_sdf_trace) and its Python surface against the numpy reference of the contract
(tests/sdf_trace_reference.py): the embedding bit for bit against ops.hash_fwd_f32, f within 4 x the error of a serial float32
evaluation against float64, the trace exact in status and n_eval on every decided ray of the named sets and within 4 x E32 in t, xyz
and f_last, the invariants on every ray."""
import ctypes

import numpy as np
import pytest

import sdf_trace_reference as R

pytestmark = pytest.mark.gpu
G = 32
NAMES = ["threshold_shell_n1", "threshold_shell_n63", "threshold_shell_n64", "threshold_shell_n65", "threshold_shell_n1153", "threshold_ones",
         "crossing_refine0", "crossing_refine1", "crossing_refine8", "defaults_ones", "all_zeros", "inside_ones", "inside_shell",
         "abandoned_max3", "miss_slab", "miss_past_surface", "zero_component", "grazing", "mixed_signs"]
KEYS = ("status", "t", "xyz", "n_eval", "f_last")


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    return torch


class Field:
    """A reference model on the device: level table, table, pack."""

    def __init__(self, torch, lv, model):
        dev = torch.device("cuda")
        self.lv, self.model = lv, model
        self.table = torch.from_numpy(model.table.reshape(-1)).to(dev)
        self.wpack = torch.from_numpy(model.pack()).to(dev)
        self.bits = {}

    def grid(self, torch, grid):
        from ngp_hip import ops
        key = id(grid)
        if key not in self.bits:
            b = torch.from_numpy(grid.bits).cuda()
            self.bits[key] = (b, ops.coarse_bitfield(b, grid.casc, grid.G))
        return self.bits[key]


def run(torch, fld, case, o=None, d=None, out=None, coarse=True):
    from ngp_hip import ops
    m = case.model
    bits, cz = fld.grid(torch, case.grid)
    o = torch.from_numpy(case.o if o is None else o).cuda()
    d = torch.from_numpy(case.d if d is None else d).cuda()
    res = ops.sdf_trace(o, d, bits, cz if coarse else None, fld.table, fld.lv, fld.wpack, m.width, m.depth, case.grid.casc, m.scale,
                        case.grid.G, out=out, **case.params)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(KEYS, res)}


@pytest.fixture(scope="module")
def small(torch_mod):
    from ngp_hip import ops
    lv = ops.make_levels(2**12, 4, 8, 64, 2)
    levels = ops.levels_to_numpy(lv)
    model = R.make_model(levels, lv.begin_fast_hash_level, lv.total_entries, 16, 1, 0.5, seed=3)
    return Field(torch_mod, lv, model), {c.name: c for c in R.case_table(model, G)}


@pytest.fixture(scope="module")
def wide(torch_mod):
    from ngp_hip import ops
    lv = ops.make_levels(2**12, 4, 8, 64, 2)
    model = R.make_model(ops.levels_to_numpy(lv), lv.begin_fast_hash_level, lv.total_entries, 16, 1, 1.0, seed=3)
    return Field(torch_mod, lv, model), {c.name: c for c in R.case_table(model, G)}


@pytest.fixture(scope="module")
def default_arch(torch_mod):
    from ngp_hip import ops
    lv = ops.make_levels(2**19, 16, 16, 2048, 2)
    case = R.default_arch_case(ops.levels_to_numpy(lv), lv.begin_fast_hash_level, lv.total_entries, G)
    return Field(torch_mod, lv, case.model), case


def check_eval(torch, fld, x):
    """the embedding bit for bit, f within 4 x E32 of float64 (E32: the serial float32 field's largest error on these points, at
    least one float32 ulp of the largest |f|)"""
    from ngp_hip import ops
    m = fld.model
    xt = torch.from_numpy(x).cuda()
    f, enc = ops.sdf_eval(xt, fld.table, fld.lv, fld.wpack, m.width, m.depth, m.scale, return_enc=True)
    lo, hi = torch.full((1, 3), -m.scale, device="cuda"), torch.full((1, 3), m.scale, device="cuda")
    want_enc = ops.hash_fwd_f32(((xt - lo) / (hi - lo)).contiguous(), fld.table, fld.lv)
    assert torch.equal(enc.view(torch.int32), want_enc.view(torch.int32)), "the embedding differs from hash_fwd_f32 in some bit"
    assert torch.equal(f, ops.sdf_eval(xt, fld.table, fld.lv, fld.wpack, m.width, m.depth, m.scale))
    f64, f32 = R.field(m, x, np.float64), R.field(m, x, np.float32)
    e32 = max(float(np.abs(f32 - f64).max()), float(R.ulp32(np.abs(f64).max())))
    err = float(np.abs(f.cpu().numpy().astype(np.float64) - f64).max())
    print("sdf_eval n=%d: err %.3g = %.2f x E32" % (len(x), err, err / e32))
    assert err <= 4 * e32, "f off by %.3g = %.2f x E32 (bound 4)" % (err, err / e32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1153])
def test_eval_small_model(torch_mod, small, n):
    check_eval(torch_mod, small[0], R.eval_points(np.random.default_rng(100 + n), n, 0.5))


def test_eval_wide_and_default_models(torch_mod, wide, default_arch):
    check_eval(torch_mod, wide[0], R.eval_points(np.random.default_rng(7), 130, 1.0))
    check_eval(torch_mod, default_arch[0], R.eval_points(np.random.default_rng(8), 65, 0.5))


def check_case(torch, fld, case):
    got = run(torch, fld, case)
    R.invariants(case, got)
    if not case.only_invariants:
        assert case.undecided_fraction() <= R.MAX_UNDECIDED
        fig = R.judge(case, got)
        print(case.name, " ".join("%s %.2f" % kv for kv in fig.items()))
    return got


@pytest.mark.parametrize("name", NAMES)
def test_trace_small_model(torch_mod, small, name):
    fld, cases = small
    got = check_case(torch_mod, fld, cases[name])
    if name == "all_zeros":
        assert (got["status"] == R.MISS).all() and (got["n_eval"] == 0).all()


@pytest.mark.parametrize("name", ["threshold_shell_n65", "crossing_refine8"])
def test_trace_two_cascades(torch_mod, wide, name):
    fld, cases = wide
    assert cases[name].grid.casc == 2
    check_case(torch_mod, fld, cases[name])


def test_trace_default_architecture(torch_mod, default_arch):
    fld, case = default_arch
    got = check_case(torch_mod, fld, case)
    assert (got["status"] == R.HIT).sum() > 10


def test_plane_by_hand(torch_mod, small):
    """f = z - 0.25 exactly (zero table, Softplus the identity); the ray of tests/test_sdf_trace_reference.py: the threshold path is
    the geometric recurrence, bit for bit; the crossing path returns the root of the linear interpolation."""
    from test_sdf_trace_reference import PLANE_D, PLANE_O, plane_model
    from ngp_hip import ops
    lv = small[0].lv
    fld = Field(torch_mod, lv, plane_model(ops.levels_to_numpy(lv), lv.begin_fast_hash_level, lv.total_entries))
    grid = R.Grid(np.full(G**3 // 8, 255, np.uint8), 0.5, G)
    c = R.Case("plane_threshold", fld.model, grid, PLANE_O, PLANE_D, eps=1e-3, min_step=0.0)
    got = run(torch_mod, fld, c)
    assert got["status"][0] == R.HIT and got["n_eval"][0] == 9
    assert got["t"][0] == np.float32(1.0 + 0.5 * (1.0 - 2.0**-8)) and got["f_last"][0] == np.float32(2.0**-10)
    for nr in (0, 1, 8):
        c = R.Case("plane_crossing", fld.model, grid, PLANE_O, PLANE_D, eps=0.0, n_refine=nr)
        got = run(torch_mod, fld, c)
        assert got["status"][0] == R.HIT and got["n_eval"][0] == 11 + nr and abs(float(got["t"][0]) - 1.5) <= 4 * 2.0**-24 * 1.5


def test_launches_are_bit_identical_and_follow_a_permutation(torch_mod, small):
    fld, cases = small
    for name in ("threshold_shell_n1153", "mixed_signs"):
        case = cases[name]
        a, b, nc = run(torch_mod, fld, case), run(torch_mod, fld, case), run(torch_mod, fld, case, coarse=False)
        perm = np.random.default_rng(5).permutation(len(case.o))
        p = run(torch_mod, fld, case, o=np.ascontiguousarray(case.o[perm]), d=np.ascontiguousarray(case.d[perm]))
        for k in KEYS:
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
            assert np.array_equal(a[k].view(np.int32), nc[k].view(np.int32)), "%s depends on the coarse table" % k
            assert np.array_equal(a[k][perm].view(np.int32), p[k].view(np.int32)), "%s depends on the batch order" % k


def test_rows_past_n_rays_stay_untouched(torch_mod, small):
    torch = torch_mod
    fld, cases = small
    case = cases["threshold_shell_n65"]
    n, pad = 65, 64
    full = (torch.full((n + pad,), -7, device="cuda", dtype=torch.int32), torch.full((n + pad,), float("nan"), device="cuda"),
            torch.full((n + pad, 3), float("nan"), device="cuda"), torch.full((n + pad,), -7, device="cuda", dtype=torch.int32),
            torch.full((n + pad,), float("nan"), device="cuda"))
    got = run(torch, fld, case, out=tuple(t[:n] for t in full))
    want = run(torch, fld, case)
    for k, t in zip(KEYS, full):
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32))
        tail = t[n:].cpu().numpy()
        assert (tail == -7).all() if tail.dtype == np.int32 else np.isnan(tail).all(), "%s: a row past n_rays was written" % k


def test_bad_arguments_launch_nothing(torch_mod, small):
    torch = torch_mod
    from ngp_hip import lib, ops
    L = lib.load()
    fld, cases = small
    case = cases["threshold_shell_n65"]
    bits, cz = fld.grid(torch, case.grid)
    o, d = torch.from_numpy(case.o).cuda(), torch.from_numpy(case.d).cuda()
    n = 65
    outs = (torch.full((n,), -7, device="cuda", dtype=torch.int32), torch.full((n,), -7.0, device="cuda"), torch.full((n, 3), -7.0, device="cuda"),
            torch.full((n,), -7, device="cuda", dtype=torch.int32), torch.full((n,), -7.0, device="cuda"))
    f_out, enc_out = torch.full((n,), -7.0, device="cuda"), torch.full((n, 8), -7.0, device="cuda")
    lv4 = lib.HashLevels()
    ctypes.memmove(ctypes.byref(lv4), ctypes.byref(fld.lv), ctypes.sizeof(lib.HashLevels))
    lv4.n_features = 4
    P = ops._ptr

    def trace(**kw):
        a = dict(o=P(o), d=P(d), bits=P(bits), coarse=P(cz), table=P(fld.table), lv=fld.lv, w=P(fld.wpack), width=16, depth=1, casc=1, scale=0.5,
                 G=G, n=n, eps=1e-4, step=1.0, min_step=0.0, n_refine=8, max_evals=256, status=P(outs[0]))
        a.update(kw)
        return L.ngp_sdf_trace(a["o"], a["d"], a["bits"], a["coarse"], a["table"], ctypes.byref(a["lv"]), a["w"], a["width"], a["depth"], a["casc"],
                               a["scale"], a["G"], a["n"], a["eps"], a["step"], a["min_step"], a["n_refine"], a["max_evals"], a["status"],
                               P(outs[1]), P(outs[2]), P(outs[3]), P(outs[4]), None, ops._stream())

    def evalf(**kw):
        a = dict(x=P(o), table=P(fld.table), lv=fld.lv, w=P(fld.wpack), width=16, depth=1, scale=0.5, n=n, f=P(f_out))
        a.update(kw)
        return L.ngp_sdf_eval(a["x"], a["table"], ctypes.byref(a["lv"]), a["w"], a["width"], a["depth"], a["scale"], a["n"], a["f"], P(enc_out),
                              ops._stream())

    null = ctypes.c_void_p(0)
    bad_trace = [dict(o=null), dict(bits=null), dict(table=null), dict(w=null), dict(status=null), dict(n=-1), dict(width=48), dict(depth=3),
                 dict(depth=0), dict(lv=lv4), dict(casc=9), dict(casc=0), dict(G=2048), dict(G=48), dict(G=512, casc=2), dict(scale=0.0),
                 dict(eps=-1.0), dict(step=0.0), dict(min_step=-1.0), dict(n_refine=-1), dict(max_evals=-1)]
    for kw in bad_trace:
        assert trace(**kw) == -1, kw
    for kw in [dict(x=null), dict(table=null), dict(w=null), dict(f=null), dict(n=-1), dict(width=48), dict(depth=3), dict(lv=lv4), dict(scale=-1.0)]:
        assert evalf(**kw) == -1, kw
    assert trace(n=0) == 0 and evalf(n=0) == 0
    torch.cuda.synchronize()
    for t in outs + (f_out, enc_out):
        assert (t == -7).all(), "a refused call wrote an output"
    with pytest.raises(ValueError):
        ops.sdf_trace(o, d, bits, cz, fld.table, fld.lv, fld.wpack, 48, 1, 1, 0.5, G)
    with pytest.raises(ValueError):
        ops.sdf_eval(o, fld.table, fld.lv, fld.wpack[:-1], 16, 1, 0.5)
    assert trace() == 0                                             # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert (outs[0] >= 0).all()


@pytest.fixture(scope="module")
def sdf_model(torch_mod):
    torch = torch_mod
    from ngp_hip.surface import SDFField
    torch.manual_seed(3)
    model = SDFField(scale=0.5, levels=4, log2_T=12, base_res=8, max_res=64, geo_width=16, geo_depth=1).cuda()
    with torch.no_grad():
        model.pos_encoder.hash_table.uniform_(-0.05, 0.05)
        model.density_bitfield.fill_(255)
    return model


def test_packed_geometry_round_trips(torch_mod, sdf_model):
    torch = torch_mod
    pack = sdf_model.packed_geometry()
    layers = list(sdf_model.geo_layers)
    k = 0
    for lin in layers[:-1]:
        for p in (lin.weight, lin.bias):
            assert torch.equal(pack[k:k + p.numel()].view(torch.int32), p.detach().reshape(-1).view(torch.int32))
            k += p.numel()
    assert torch.equal(pack[k:k + 16], layers[-1].weight.detach()[0]) and torch.equal(pack[k + 16:], layers[-1].bias.detach()[:1])
    assert pack.numel() == k + 17
    before = pack.clone()
    with torch.no_grad():
        layers[0].bias.add_(1.0)
    assert torch.equal(pack, before), "the pack aliases the parameters"
    with torch.no_grad():
        layers[0].bias.sub_(1.0)


def test_public_path(torch_mod, sdf_model):
    torch = torch_mod
    from ngp_hip import ops
    from ngp_hip.surface import render_surface_traced, trace_surface
    model = sdf_model
    rng = np.random.default_rng(9)
    o1, d1 = R.rays_at(rng, 200, 1.7, 0.0, 0.15, mixed=True)
    o2, d2 = R.rays_at(rng, 57, 1.7, 1.5, 2.0, mixed=True)
    o, d3 = torch.from_numpy(np.concatenate([o1, o2])).cuda(), 3.0 * torch.from_numpy(np.concatenate([d1, d2])).cuda()
    d = (d3 / torch.linalg.norm(d3, dim=1, keepdim=True)).contiguous()      # what render_surface_traced traces
    x = torch.from_numpy(R.eval_points(rng, 300, 0.5)).cuda()
    with torch.no_grad():
        want = model.sdf(x)                      # torch's Linear sums in another order; outside the box the extrapolated |f| is large
        assert ((model.sdf_fused(x) - want).abs() <= 1e-5 * (1.0 + want.abs())).all()
    tr = trace_surface(model, o, d)
    enc = model.pos_encoder
    raw = ops.sdf_trace(o, d, model.density_bitfield, None, enc.hash_table.detach(), enc._levels, model.packed_geometry(), 16, 1, model.cascades,
                        model.scale, model.grid_size)
    for k, v in zip(KEYS, raw):
        assert torch.equal(tr[k].view(torch.int32), v.view(torch.int32)), k
    with torch.no_grad():
        out = render_surface_traced(model, o, d3, bg=0.25, chunk=100)       # directions are normalised inside; three launches
    st = tr["status"]
    on = (st == 1) | (st == 2)
    assert on.sum() > 50 and (~on).sum() > 50
    assert torch.equal(out["status"], st) and torch.equal(out["n_eval"], tr["n_eval"])
    assert (out["rgb"][~on] == 0.25).all() and (out["opacity"][~on] == 0).all() and (out["depth"][~on] == 0).all() and (out["normal"][~on] == 0).all()
    assert torch.equal(out["depth"][on], tr["t"][on]) and (out["opacity"][on] == 1).all()
    assert (torch.linalg.norm(out["normal"][on], dim=1) - 1).abs().max() < 1e-5
    assert ((out["rgb"][on] > 0) & (out["rgb"][on] < 1)).all()
    f, _, g = model.sdf_and_grad(tr["xyz"][st == 1])
    assert f.abs().max() < 1e-3                                          # the HIT points lie on the zero level set
