"""The run-merging float-atomic scatters of the hash encoder on an input that HAS runs: ngp_hash_bwd_f32 (hash_bwd_f32x2_kernel, and
the generic hash_bwd_f32_kernel<4>), ngp_hash_bwd2_table_f32 (hash_bwd2_table_f32x2_kernel, and the generic hash_bwd2_table_kernel<1>)
and the half2 form ngp_hash_bwd_f16_live (hash_bwd_f16x2_kernel).

The other scatter tests draw positions at random, so above the coarsest levels consecutive samples almost never share a cell, and the
part these kernels share -- run detection across the 16- (f16: 32-) sample tile, the segmented scan, the tail-only atomic -- hardly
runs.  Here samples 0..39 sit inside a box of side 2^-13 around one interior point: on EVERY level they share one cell, so one run
starts at a tile start, covers a whole tile and ends inside a later one; samples 40..69 are uniform in the unit cube and pairwise in
different cells on the finest level.  Both properties are asserted from the reference's cells, not from the kernels.  Rows 3 and 41
of the gradient are exactly zero.  The prefixes n in NS are the tile edges of both lane distances.

Yardstick (that of test_gpu_hash_input_grad2.py): |gpu - ref64| <= 4 * E32 * S + 1e-30 per table entry, S the sum of the term
magnitudes, E32 the largest error over S of the serial float32 scatter in sample order on the whole 70-sample input; entries with
S == 0 keep their bits, on a table of zeros and on one of ones (which adds one ulp of 1 to the bound; the generic first-order kernel,
one atomic per sample, is held to the kept bits alone there).  Where all samples of a tile share a cell every (entry, feature)
receives exactly one atomic and two launches are bit-identical."""
import ctypes

import numpy as np
import pytest
import torch

import hash_input_grad_reference as ref
import hash_input_grad2_reference as ref2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = 1e-30
N_RUN, N = 40, 70
NS = (1, 15, 16, 17, 32, 33, 40, 70)
ZERO_ROWS = (3, 41)
TABLES = {"default": (2**19, 16, 16, 1024, 2), "f1": (2**14, 5, 8, 300, 1), "f4": (2**14, 5, 8, 300, 4)}
CENTRE = (0.7301, 0.5347, 0.3337)              # at least 0.08 of a cell from every face on every level of every table below
SEED = 11
_cache = {}
f32, f64 = np.float32, np.float64


def _input(shape):
    """The 70 samples, their gradient rows and ddx, the reference's corners, and the structure the test is about: computed once."""
    if shape in _cache:
        return _cache[shape]
    from ngp_hip import ops
    lv = ops.make_levels(*TABLES[shape])
    L, F = lv.n_levels, lv.n_features
    rng = np.random.default_rng(SEED)
    x = np.empty((N, 3), dtype=f32)
    x[:N_RUN] = np.asarray(CENTRE, dtype=f32) + (rng.random((N_RUN, 3), dtype=f32) - f32(0.5)) * f32(2.0**-13)
    x[N_RUN:] = rng.random((N - N_RUN, 3), dtype=f32)
    g = rng.standard_normal((N, L * F)).astype(f32)
    g[list(ZERO_ROWS)] = 0.0
    ddx = rng.standard_normal((N, 3)).astype(f32)
    t = ref.level_table(lv)
    for l in range(L):
        cell, _ = ref.cell_frac(x, t["scale"][l])
        # one run on every level: it starts at sample 0 (a tile start), covers samples 16..31 (a whole tile) and ends at sample 39,
        # inside the third 16-sample tile (the second 32-sample tile)
        assert np.all(cell[:N_RUN] == cell[0]), "level %d: samples 0..39 do not share a cell" % l
        assert np.any(cell[N_RUN] != cell[0]), "level %d: the run does not end at sample 39" % l
    assert len(np.unique(cell[N_RUN:], axis=0)) == N - N_RUN, "finest level: samples 40..69 are not pairwise in different cells"
    idx, w = ref.corners(x, lv)
    c = dict(lv=lv, L=L, F=F, x=x, g=g, ddx=ddx, idx=idx.astype(np.int64), w=w, size=lv.total_entries * F)
    _cache[shape] = c
    return c


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_input_has_the_runs(hip_lib):
    for shape in TABLES:
        c = _input(shape)                                             # asserts the structure
        assert c["idx"].shape == (N, c["L"], 8) and not np.any(c["g"][list(ZERO_ROWS)]) and np.all(np.any(c["g"][[0, 1, 2, 40]] != 0, axis=1))


# ------------------------------------------------------------------------------------------------ first order
def _first_order_ref(c, n):
    """Float64 scatter of the forward's float32 corner weights times the gradient rows, on the entries some corner names:
    (flat entries, sum, magnitude sum S, serial float32 sum in sample order)."""
    F = c["F"]
    wn, gn = c["w"][:n], c["g"][:n].reshape(n, c["L"], 1, F)
    flat = (c["idx"][:n][..., None] * F + np.arange(F)).reshape(-1)
    uniq, inv = np.unique(flat, return_inverse=True)
    term = (wn.astype(f64)[..., None] * gn.astype(f64)).reshape(-1)
    d = np.bincount(inv, weights=term, minlength=uniq.size)
    S = np.bincount(inv, weights=np.abs(term), minlength=uniq.size)
    d32 = np.zeros(uniq.size, dtype=f32)
    np.add.at(d32, inv, (wn[..., None] * gn).astype(f32).reshape(-1))      # unbuffered: one float32 add per term, sample-major order
    return uniq, d, S, d32


def _check_kept(got, entries, S, fill, what):
    """got: the whole table after the launch (device).  Every element but the entries with S > 0 keeps fill's bits."""
    on = S > 0
    keep = torch.ones(got.numel(), dtype=torch.bool, device=DEV)
    keep[_dev(entries[on])] = False
    fill_bits = int(_bits(np.full(1, fill, dtype=f32))[0])
    assert bool((got.view(torch.int32)[keep] == fill_bits).all()), "%s: an entry with S == 0 changed" % what


def _check(got, entries, d, S, e32, fill, what):
    """Entries with S > 0 hold the bound; every other element keeps fill's bits."""
    _check_kept(got, entries, S, fill, what)
    on = S > 0
    err = np.abs(got[_dev(entries[on])].cpu().numpy().astype(f64) - (f64(fill) + d[on]))
    slack = TINY + (2.0**-23 if fill else 0.0)
    worst = float(np.max((err - slack) / (e32 * S[on])))
    print("%s onto %g: worst |gpu - ref64| / (E32 S) = %.3f, bound 4" % (what, fill, worst))
    assert worst <= 4.0, (what, fill, worst)


def _first_order_launch(c, x, g, n, fill):
    from ngp_hip import ops
    got = ops.hash_bwd_f32(x[:n].contiguous(), g[:n].contiguous(), c["lv"], torch.full((c["size"],), fill, device=DEV))
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("shape,fill", [("default", 0.0), ("default", 1.0), ("f4", 0.0)])
def test_first_order_scatter_against_float64(hip_lib, shape, fill):
    """F = 2 (the run-merging kernel) onto zeros and onto ones, F = 4 (hash_bwd_f32_kernel<4>, one atomic per sample) onto zeros.
    F = 4 onto ones is NOT held to the bound (test_generic_first_order_scatter_onto_ones_keeps_the_other_entries has the reason)."""
    c = _input(shape)
    _, d, S, d32 = _first_order_ref(c, N)
    e32 = float(np.max(np.abs(d32[S > 0].astype(f64) - d[S > 0]) / S[S > 0]))
    assert e32 > 0
    print("first-order scatter %s: E32 = %.3g" % (shape, e32))
    x, g = _dev(c["x"]), _dev(c["g"])
    for n in NS:
        entries, d, S, _ = _first_order_ref(c, n)
        _check(_first_order_launch(c, x, g, n, fill), entries, d, S, e32, fill, "ngp_hash_bwd_f32 %s n=%d" % (shape, n))


def test_generic_first_order_scatter_onto_ones_keeps_the_other_entries(hip_lib):
    """F = 4 onto a table of ones: every entry with S == 0 keeps its bits, on every prefix.  The entries with S > 0 are not compared
    here: 4 * E32 * S + one ulp of 1 is not a bound that one float32 atomic PER SAMPLE can keep on this input.  An entry of the run
    takes sixteen (n = 40: forty) roundings at the magnitude of the 1.0 it is added onto, whatever its S; measured, the worst
    |gpu - ref64| / (E32 S) after the ulp is 4.178 at n = 16 or below 4 depending on the order in which the atomics land (before
    the scatter kernels shared any code, and since), and a serial float32 accumulation of the same terms onto ones gives
    2.0 .. 5.4 over the prefixes depending on the order.  An allowance that is sound per entry -- half an ulp of the running sum per
    contribution -- is not the suite's yardstick, so no bound is asserted until one is agreed (profiles/hash_lanes_refactor.md).
    The run-merging F = 2 kernel adds a run's sum once and is held to the bound onto ones above."""
    c = _input("f4")
    x, g = _dev(c["x"]), _dev(c["g"])
    for n in NS:
        entries, _, S, _ = _first_order_ref(c, n)
        _check_kept(_first_order_launch(c, x, g, n, 1.0), entries, S, 1.0, "ngp_hash_bwd_f32 f4 n=%d" % n)


# ------------------------------------------------------------------------------------------------ second order
@pytest.mark.parametrize("fill", [0.0, 1.0])
@pytest.mark.parametrize("shape", ["default", "f1"])
def test_second_order_scatter_against_float64(hip_lib, shape, fill):
    from ngp_hip import ops
    c = _input(shape)
    zeros = np.zeros(c["size"], dtype=f32)                            # the table scatter does not read the table
    if "e32_table" not in c:
        _, _, d_table32 = ref2.bwd2_32(c["x"], zeros, c["g"], c["ddx"], c["lv"])
        _, _, _, _, d_table, S_table = ref2.bwd2_64(c["x"], zeros, c["g"], c["ddx"], c["lv"])
        touched = S_table > 0
        assert np.all(d_table32[~touched] == 0)
        c["e32_table"] = float(np.max(np.abs(d_table32[touched].astype(f64) - d_table[touched]) / S_table[touched]))
        c["ref2"] = {}
        for n in NS[::-1]:                                            # (entries with S > 0, their sums, their S) per prefix, N first
            if n != N:
                _, _, _, _, d_table, S_table = ref2.bwd2_64(c["x"][:n], zeros, c["g"][:n], c["ddx"][:n], c["lv"])
            entries = np.flatnonzero(S_table > 0)
            c["ref2"][n] = (entries, d_table[entries], S_table[entries])
    e32 = c["e32_table"]
    assert e32 > 0
    print("second-order scatter %s: E32 = %.3g" % (shape, e32))
    x, g, ddx = _dev(c["x"]), _dev(c["g"]), _dev(c["ddx"])
    for n in NS:
        got = ops.hash_bwd2_table_f32(x[:n].contiguous(), g[:n].contiguous(), ddx[:n].contiguous(), c["lv"],
                                      torch.full((c["size"],), fill, device=DEV))
        torch.cuda.synchronize()
        _check(got, *c["ref2"][n], e32, fill, "ngp_hash_bwd2_table_f32 %s n=%d" % (shape, n))


# ------------------------------------------------------------------------------------------------ one run, one atomic per entry
def _pair_major(g, n):
    """[n, 16, 2] rows as the fused path's eight pair-major planes [8][n][4] (plane p = levels p and 15 - p)."""
    g = g.reshape(n, 16, 2)
    pm = torch.zeros(8, n, 4, device=g.device)
    for l in range(16):
        pm[l if l < 8 else 15 - l, :, (0 if l < 8 else 2):(2 if l < 8 else 4)] = g[:, l]
    return pm.contiguous()


def single_run_launches():
    """name -> closure that runs the entry once on a zero table and returns the table: n = 16 (f16: 32) samples of the run, i.e. one
    tile whose samples share a cell on every level, so every (entry, feature) receives exactly one atomic."""
    from ngp_hip import lib as L, ops
    from ngp_hip.ops import _ptr, _stream
    lib = L.load()
    c = _input("default")
    lv, LV = c["lv"], ctypes.byref(c["lv"])
    for n in (16, 32):                                                # the eight corners of the cell are eight entries on every level
        assert all(len(set(c["idx"][0, l])) == 8 for l in range(c["L"])) and np.all(c["idx"][:n] == c["idx"][0])
    x, g, ddx = _dev(c["x"]), _dev(c["g"]), _dev(c["ddx"])
    ident = torch.arange(32, device=DEV, dtype=torch.int32)
    null = _ptr(None)

    def run(name, dtype, *args):
        def go():
            table = torch.zeros(c["size"], device=DEV, dtype=dtype)
            a = [_ptr(table) if v is table_slot else v for v in args]
            L.check(getattr(lib, name)(*a, _stream()), name)
            torch.cuda.synchronize()
            return table
        return go

    table_slot = object()
    x16, g16, x32, g32 = x[:16].contiguous(), g[:16].contiguous(), x[:32].contiguous(), g[:32].contiguous()
    pm16, pm32, d16 = _pair_major(g16, 16), _pair_major(g32, 32), ddx[:16].contiguous()
    keep = (x16, g16, x32, g32, pm16, pm32, d16, ident)               # the closures hold raw pointers into these
    return {
        "ngp_hash_bwd_f32": run("ngp_hash_bwd_f32", torch.float32, _ptr(x16), _ptr(g16), LV, 16, table_slot),
        "ngp_hash_bwd_f32_live": run("ngp_hash_bwd_f32_live", torch.float32, _ptr(x16), _ptr(pm16), LV, 16, null, _ptr(ident), 0, 0.0, 1.0, 1,
                                     table_slot, null),
        "ngp_hash_bwd2_table_f32": run("ngp_hash_bwd2_table_f32", torch.float32, _ptr(x16), _ptr(g16), _ptr(d16), LV, 16, table_slot),
        "ngp_hash_bwd_f16_live": run("ngp_hash_bwd_f16_live", torch.float16, _ptr(x32), _ptr(pm32), LV, 32, null, _ptr(ident), 0, 0.0, 1.0, 1,
                                     table_slot, null),
    }, keep


@pytest.mark.parametrize("entry", ["ngp_hash_bwd_f32", "ngp_hash_bwd_f32_live", "ngp_hash_bwd2_table_f32", "ngp_hash_bwd_f16_live"])
def test_single_run_is_bit_reproducible(hip_lib, entry):
    launches, _keep = single_run_launches()
    a, b = launches[entry](), launches[entry]()
    assert bool((a != 0).any()) and torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                                                b.view(torch.int16 if b.dtype == torch.float16 else torch.int32))
    if entry == "ngp_hash_bwd_f32_live":                              # the list and the pair-major layout move no bit either
        assert torch.equal(a, launches["ngp_hash_bwd_f32"]())


# ------------------------------------------------------------------------------------------------ the half2 form
def test_f16_live_matches_the_operator_kernel_on_runs(hip_lib):
    """ngp_hash_bwd_f16_live (runs summed in f32, one packed f16 atomic per run) against ngp_hash_bwd_f16 (one atomic per sample) on the
    run input, with the comparison of test_gpu_half_fused.py::test_bwd_f16_ex_matches_operator_kernel."""
    from ngp_hip import lib as L, ops
    from ngp_hip.ops import _ptr, _stream
    lib = L.load()
    c = _input("default")
    lv = c["lv"]
    x, g = _dev(c["x"]), _dev(c["g"])
    want = torch.zeros(lv.total_entries, 2, device=DEV, dtype=torch.float16)
    ops.hash_bwd_f16(x, g.half().view(N, 16, 2), lv, want)
    got = torch.zeros_like(want)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    L.check(lib.ngp_hash_bwd_f16_live(_ptr(x), _ptr(g), ctypes.byref(lv), N, _ptr(None), _ptr(None), 0, 0.0, 1.0, 0, _ptr(got), _ptr(flag),
                                      _stream()), "ngp_hash_bwd_f16_live")
    torch.cuda.synchronize()
    a, b = got.float(), want.float()
    assert int(flag) == 0
    same, worst, rel = ((a != 0) == (b != 0)).float().mean().item(), (a - b).abs().max().item(), ((a - b).norm() / b.norm()).item()
    print("f16 live vs operator kernel on runs: same touched %.5f, max |a - b| = %.3g of max |b| = %.3g, relative norm %.3g"
          % (same, worst, b.abs().max().item(), rel))
    assert same > 0.999
    assert worst <= 2e-2 * b.abs().max().item()
    assert rel < 2e-3
