"""tests/occupancy_reference.py on the CPU: it reproduces the vectors the reference project's own update_density_grid produced
(tests/golden/ref_update_density_grid.npz) from the recorded draws alone, agrees with the oracle's restatement, its generator keeps
the promised band clear at every size the GPU test uses, merge_sum_bound dominates a float32 emulation of the kernels' summation
tree, every edge rule of the module's docstring holds on a hand-sized case, and every comparison helper rejects a near miss."""
import os

import numpy as np
import pytest

import occupancy_reference as oref
from occupancy_reference import F32, F64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN, INF = F32(np.nan), F32(np.inf)


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


# ------------------------------------------------------------------------------------------------ the reference project's vectors
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_reproduces_reference_fixture(dtype):
    """Warm-up and sampled update of the 2-cascade 16^3 fixture from the recorded jitter, randint draws and densities: positions,
    grids and bitfields bit for bit.  The float64 form differs from the float32 one in the positions (held to POS_BOUND against the
    recorded float32 ones, which cannot be bit-equal to a float64 number) and in the threshold (a float64 mean): its grids and
    bitfields are bit for bit the fixture's all the same."""
    g = np.load(os.path.join(GOLDEN, "ref_update_density_grid.npz"))
    G, C, scale = int(g["grid_size"]), int(g["cascades"]), float(g["scale"])
    cap, decay, G3 = float(g["threshold"]), float(g["decay"]), G**3
    order = g["all_indices"].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(G3))
    jit = []
    for c in range(C):
        j = np.empty((G3, 3), F32)
        j[order] = g["warm_jitter"][c]                       # recorded in grid_coords order; row i of ours is Morton code i
        jit.append(j)
    w = oref.update(g["grid_before"], G, scale, cap, decay, True, jit, list(g["warm_sigma_by_morton"]), dtype=dtype)
    for c in range(C):
        if dtype == F32:
            assert oref.same_bits(w["xyz"][c], g["warm_xyz_by_morton"][c])
        else:
            s, _ = oref.cascade_extent(c, scale, G)
            assert np.abs(w["xyz"][c] - g["warm_xyz_by_morton"][c].astype(F64)).max() <= oref.pos_bound(s)
    assert oref.same_bits(w["grid"], g["warm_grid_after"])
    assert oref.same_bytes(w["bits"], g["warm_bitfield"])
    # the fixture sits in the cap branch -- which is why the GPU tests bring inputs of their own for the other one
    assert w["sum64"] / w["count"] > cap and float(w["thr"]) == float(F32(cap))
    # sampled update: the reference's randint draws as the uniforms that select the same cells
    assert oref.same_bits(w["grid"], g["samp_grid_before"])
    uni = []
    for c in range(C):
        lst, n_occ = oref.compact(g["samp_grid_before"][c], cap)
        assert n_occ == int(g["samp_n_occupied"][c])
        code = oref.morton(g["samp_coords1"][c]).astype(F64)
        uni.append((((code + 0.5) / G3).astype(F32), ((g["samp_rand_idx"][c].astype(F64) + 0.5) / n_occ).astype(F32)))
        idx = oref.sample_indices(uni[c][0], uni[c][1], lst, n_occ, G3 // 4, G)
        assert np.array_equal(idx[:G3 // 4], code.astype(np.int32)) and np.array_equal(idx[G3 // 4:], lst[g["samp_rand_idx"][c]])
    centre = [np.full((G3 // 2, 3), 0.5, F32)] * C
    dens = lambda c, xyz, idx: g["centre_sigma_by_morton"][c][idx]
    s = oref.update(g["samp_grid_before"], G, scale, cap, decay, False, centre, dens, uniforms=uni, dtype=dtype)
    assert oref.same_bits(s["grid"], g["samp_grid_after"])
    assert oref.same_bytes(s["bits"], g["samp_bitfield"])
    assert not oref.same_bits(s["grid"], g["samp_grid_before"])
    d = oref.update(g["samp_grid_before"], G, scale, cap, decay, False, centre, dens, uniforms=uni, det=True, dtype=dtype)
    assert oref.same_bits(d["grid"], g["samp_grid_after"])                 # one density per cell: the max scatter agrees


def test_agrees_with_oracle(oracle):
    """Two restatements side by side: oracle.train_loop's update_density_grid (warm-up form), oracle.packbits and the Morton codes."""
    from oracle.train_loop import OracleTrainer
    G, scale, cap = 16, 2.0, 5.912
    tr = OracleTrainer([np.zeros((2, 2), F32)] * 5, np.zeros(4, F32), scale=scale, grid_size=G)
    C, G3 = tr.cascades, G**3
    assert C == 3
    rng = np.random.default_rng(5)
    for amp in (4.0, 40.0):                                                # mean below and above the cap
        tr.density = lambda xyz, autocast=False: oref.blob(xyz, amp)
        tr.density_grid = np.where(rng.random((C, G3)) < 0.1, -1, rng.random((C, G3)) * amp).astype(F32)
        before = tr.density_grid.copy()
        jit = [rng.random((G3, 3), dtype=F32) for _ in range(C)]
        mean = tr.update_density_grid(cap, jit)
        r32 = oref.update(before, G, scale, cap, 0.95, True, jit, lambda c, xyz, idx: oref.blob(xyz, amp))
        dens = [oref.blob(x, amp) for x in r32["xyz"]]                     # the float64 form: same densities, float64 threshold
        r64 = oref.update(before, G, scale, cap, 0.95, True, jit, dens, dtype=F64)
        for c in range(C):
            assert np.abs(r64["xyz"][c] - r32["xyz"][c]).max() <= oref.pos_bound(oref.cascade_extent(c, scale, G)[0])
        for r in (r32, r64):
            assert oref.same_bits(r["grid"], tr.density_grid)
            assert abs(r["sum64"] / r["count"] - mean) <= 1e-12 * mean and (mean < cap) == (amp == 4.0)
            assert oref.same_bytes(r["bits"], tr.bits)
    grid = tr.density_grid.reshape(-1)
    assert oref.same_bytes(oref.pack(grid, F32(1.25)), oracle.packbits(grid, 1.25))
    codes = np.arange(G3, dtype=np.int32)
    assert np.array_equal(oref.morton_invert(codes), oracle.morton3d_invert(codes))
    coords = rng.integers(0, 128, (500, 3)).astype(np.int32)
    assert np.array_equal(oref.morton(coords), oracle.morton3d(coords))
    assert np.array_equal(oref.morton_invert(oref.morton(coords)), coords)


# ------------------------------------------------------------------------------------------------ generator and bound
def test_merge_depth_formula():
    assert [oref.merge_blocks(n) for n in oref.MERGE_SIZES] == [1, 2, 8, 512, 512, 512]
    assert [oref.merge_depth(n) for n in oref.MERGE_SIZES] == [4 + 1 + 17, 4 + 1 + 17, 4 + 1 + 17, 4 + 2 + 17, 8 + 2 + 17, 68 + 2 + 17]
    assert oref.merge_depth(128**3) == 4 * 4 + 2 + 17
    D = oref.merge_depth(oref.MERGE_SIZES[-1])
    assert oref.merge_sum_bound(oref.MERGE_SIZES[-1]) == D * oref.U / (1 - D * oref.U) + oref.U


@pytest.mark.parametrize("n", oref.MERGE_SIZES)
def test_generator_band_and_branches(n):
    cap = 5.912
    grid, tmp = oref.merge_inputs(n, n % 1000, "mean", cap)
    after, s64, cnt = oref.merge(grid, tmp, 0.95)
    mean = s64 / cnt
    assert mean < cap and oref.band_clear(after, s64, cnt, n)
    assert np.abs(after.astype(F64) - mean).min() > 4 * oref.merge_sum_bound(n) * mean
    # the float32 threshold of the kernels' own summation order selects the same cells as the float64 one
    t32 = oref.threshold32(*oref.merge_sum32(after), cap)
    assert abs(float(t32) - mean) <= oref.merge_sum_bound(n) * (1 + 1e-4) * mean
    assert oref.same_bytes(oref.pack(np.resize(after, n + (-n % 8)), t32), oref.pack(np.resize(after, n + (-n % 8)), mean))
    if n >= 1032:                                                          # every kind of cell is there
        gd = (grid * F32(0.95)).astype(F32)
        vis = grid > 0
        assert (grid == -1).any() and (grid == 0).any() and (tmp[vis] == 0).any() and (tmp[vis] == gd[vis]).any()
        assert (tmp[vis] > gd[vis]).any() and ((tmp[vis] < gd[vis]) & (tmp[vis] > 0)).any() and (tmp[grid == -1] > 0).any()
        assert 0.05 < (grid == -1).mean() < 0.15 and 0.2 < (grid == 0).mean() < 0.4
    grid, tmp = oref.merge_inputs(n, n % 1000, "cap", cap)
    after, s64, cnt = oref.merge(grid, tmp, 0.95)
    assert s64 / cnt > 2 * cap
    grid, tmp = oref.merge_inputs(n, n % 1000, "none", cap)
    after, s64, cnt = oref.merge(grid, tmp, 0.95)
    assert cnt == 0 and s64 == 0 and ((grid == -1).any() or n < 1032)


@pytest.mark.parametrize("n", oref.MERGE_SIZES)
def test_bound_dominates_emulated_summation(n):
    """The float32 emulation of occ_merge_kernel + occ_pack_kernel's summation tree stays within merge_sum_bound(n) of the float64
    sum -- on the generator's inputs and on a grid of equal values, where every rounding of a serial chain has the same sign."""
    worst = 0.0
    for after in (oref.merge(*oref.merge_inputs(n, 3, "mean"), 0.95)[0], oref.merge(*oref.merge_inputs(n, 4, "cap"), 0.95)[0],
                  np.full(n, 0.1, F32), np.full(n, 1.0 + 2.0**-23, F32)):
        _, s64, cnt = oref.merge(after, np.zeros(n, F32), 1.0)
        tot, c32 = oref.merge_sum32(after)
        assert float(c32) == cnt
        ratio = abs(float(tot) - s64) / (oref.merge_sum_bound(n) * s64)
        worst = max(worst, ratio)
        assert ratio <= 1.0
    print("n = %d: D = %d, worst emulated |sum32 - sum64| / (bound sum64) = %.3f" % (n, oref.merge_depth(n), worst))


def test_emulation_sees_every_cell():
    """A positive cell anywhere moves the emulated sum: the vector part, the n & 3 tail, the second grid-stride trip."""
    for n in (1, 3, 5, 1027, 8192, 524296):
        base = np.zeros(n, F32)
        for i in {0, n - 1, n // 2, (n >> 2) * 4 - 1 if n >= 4 else 0}:
            a = base.copy()
            a[i] = 3.0
            tot, cnt = oref.merge_sum32(a)
            assert (float(tot), float(cnt)) == (3.0, 1.0), (n, i)
    ps, pc = oref.merge_partials32(np.ones(1027, F32))
    assert ps.shape == (2,) and float(ps.sum()) == 1027.0 and float(pc.sum()) == 1027.0


# ------------------------------------------------------------------------------------------------ edge rules, hand-sized
def test_compact_rules():
    thr = F32(2.5)
    grid = np.array([thr, up(thr), down(thr), NAN, -1, INF, 0, 3], F32)
    lst, n = oref.compact(grid, 2.5)
    assert lst.dtype == np.int32 and lst.tolist() == [1, 5, 7] and n == 3
    assert oref.compact(np.zeros(5, F32), 0.0)[1] == 0 and oref.compact(np.zeros(5, F32), 0.0)[0].size == 0


def test_sample_rules():
    G, M = 2, 4
    one, last = F32(1.0), F32(1.0 - 2.0**-24)
    lst = np.array([1, 4, 6], np.int32)
    u_cell = np.array([0, last, one, 0.5], F32)
    u_pick = np.array([0, last, one, 0.34], F32)
    jit = np.full((2 * M, 3), 0.5, F32)
    idx, xyz = oref.sample(u_cell, u_pick, jit, lst, 3, M, G, F32(0.5), F32(0.25))
    assert idx.tolist() == [0, 7, 7, 4, 1, 6, 6, 4]                       # both clamps; 0.34 * 3 = 1.02 -> list[1]
    assert np.array_equal(oref.morton_invert(idx)[[1, 3, 4]], [[1, 1, 1], [0, 0, 1], [1, 0, 0]])
    assert np.array_equal(xyz[1], [0.25, 0.25, 0.25]) and np.array_equal(xyz[3], [-0.25, -0.25, 0.25])   # cell centres
    idx0, _ = oref.sample(u_cell, u_pick, jit, lst, 0, M, G, F32(0.5), F32(0.25))
    assert idx0[M:].tolist() == [0, 0, 0, 0]                               # empty list: cell 0 stands in
    # the float32 product, not a wider one, at 2^21 - 1 entries
    n_occ = 2**21 - 1
    big = np.arange(n_occ, dtype=np.int32)
    mid = F32(0.4032384753227234)                                          # mid * n_occ = 845651.97..., float32 ulp there 1/16: 845652.0
    k = oref.sample_indices(np.zeros(3, F32), np.array([last, one, mid], F32), big, n_occ, 3, 128)[3:]
    assert k.tolist() == [n_occ - 1, n_occ - 1, 845652] and int(F64(mid) * n_occ) == 845651   # float64 would pick another cell
    # jitter 0 and 1 reach the cell's faces; float64 and float32 positions agree within the bound
    u = np.random.default_rng(0).random((16**3, 3), dtype=F32)
    a, b = oref.all_cells(u, 16, F32(1.0), F32(1.0 / 16)), oref.all_cells(u, 16, F32(1.0), F32(1.0 / 16), F64)
    assert a.dtype == F32 and b.dtype == F64 and 0 < np.abs(a - b).max() <= oref.pos_bound(1.0)
    assert np.abs(b).max() <= 1.0


def test_scatter_rules():
    den = F32(1e-42)
    idx = np.array([2, 2, 2, 3, 3, 4, 5, 5, 6, 6], np.int32)
    sig = np.array([1.0, 3.0, 2.0, -1.0, 0.0, NAN, den, 0.0, INF, 7.0], F32)
    got = oref.scatter_max(idx, sig, np.zeros(8, F32))
    want = np.array([0, 0, 3.0, 0, 0, den, INF, 0], F32)
    assert oref.same_bits(got, want)
    assert oref.same_bits(oref.scatter_max(idx, sig, got), got)            # idempotent
    assert oref.same_bits(oref.scatter_max(idx[::-1], sig[::-1], np.zeros(8, F32)), want)     # order-free
    assert oref.same_bits(oref.scatter_max(None, sig[:8], np.zeros(8, F32)), np.array([1, 3, 2, 0, 0, 0, den, 0], F32))
    cand = oref.scatter(idx, sig, oref.poison(8))
    for v2, v3, v4 in ((1.0, -1.0, NAN), (3.0, 0.0, NAN), (2.0, -1.0, NAN)):
        held = oref.poison(8)
        held[2:7] = [v2, v3, v4, den, 7.0]
        assert cand.holds(held).all()
    held[2] = 4.0                                                         # not drawn for cell 2
    assert cand.holds(held).tolist() == [True, True, False, True, True, True, True, True]
    held[2], held[0] = 1.0, 0.0                                           # an untouched cell lost its poison
    assert cand.holds(held).tolist() == [False] + [True] * 7
    held[0], held[3] = oref.poison(1)[0], 1.0                             # cell 2's value in cell 3
    assert not cand.holds(held)[3]


def test_merge_rules():
    d = F32(0.95)
    grid = np.array([-1, -1, 0, 0, 2, 2, 2, 2, NAN, NAN, NAN, INF, 2, 2, 0, 2], F32)
    tmp = np.array([5, NAN, 0, 3, 0, 1, F32(2) * d, 4, 3, 0, NAN, 1, NAN, INF, -3, -0.0], F32)
    after, s64, cnt = oref.merge(grid, tmp, 0.95)
    gd = F32(2) * d
    want = np.array([-1, -1, 0, 3, gd, gd, gd, 4, 3, 0, NAN, INF, gd, INF, 0, gd], F32)
    assert oref.same_bits(after, want)
    assert cnt == 10 and s64 == np.inf                                    # NaN never counted; inf counted
    assert float(oref.threshold64(s64, cnt, 5.912)) == float(F32(5.912))  # an infinite mean falls back to the cap
    tot, c32 = oref.merge_sum32(after)
    assert float(c32) == 10 and float(tot) == np.inf and oref.threshold32(tot, c32, 5.912) == F32(5.912)
    bits = oref.pack(after, oref.threshold32(tot, c32, 5.912))
    assert bits.tolist() == [0, 0b00101000]                               # only the two infinities exceed the cap
    # the merge is float32: grid * decay rounds once
    g1 = np.linspace(0.1, 9.0, 1000, dtype=F32)
    m1 = oref.merge(g1, np.zeros(1000, F32), 0.95)[0]
    assert oref.same_bits(m1, g1 * F32(0.95)) and not oref.same_bits(m1, (g1.astype(F64) * 0.95).astype(F32))
    # torch.maximum would have propagated the NaN of tmp; the kernel's fmaxf does not
    assert np.isnan(np.maximum(F32(2) * d, NAN)) and after[12] == gd


def test_threshold_and_pack_rules():
    cap = F32(5.912)
    none = np.array([-1, 0, 0, -1, 0, 0, 0, 0], F32)
    after, s64, cnt = oref.merge(none, np.zeros(8, F32), 0.95)
    tot, c32 = oref.merge_sum32(after)
    assert cnt == 0 and float(c32) == 0 and oref.threshold32(tot, c32, cap) == cap and oref.threshold64(s64, cnt, cap) == float(cap)
    assert oref.pack(after, cap).tolist() == [0]
    grid = np.array([cap, up(cap), down(cap), 100, 100, 100, 100, 100], F32)       # mean above the cap: strict at the cap
    tot, c32 = oref.merge_sum32(grid)
    thr = oref.threshold32(tot, c32, cap)
    assert thr == cap and oref.pack(grid, thr).tolist() == [0b11111010] and oref.pack(grid, float(cap)).tolist() == [0b11111010]
    low = np.array([1, 2, 3, 2, -1, 0, NAN, 2], F32)                               # mean 2 below the cap: strict at the mean
    _, s64, cnt = oref.merge(low, np.zeros(8, F32), 1.0)
    assert oref.threshold64(s64, cnt, cap) == 2.0 and oref.pack(low, 2.0).tolist() == [0b00000100]
    assert oref.pack(low, oref.threshold32(*oref.merge_sum32(low), cap)).tolist() == [0b00000100]


def test_coarsen_rules():
    bits = np.zeros(64 * 64, np.uint8)
    assert oref.coarsen(bits).tolist() == [0, 0]
    bits[0], bits[63], bits[64 * 33 + 5], bits[-1] = 1, 0x80, 0x10, 0x80
    assert oref.coarsen(bits).dtype == np.uint32 and oref.coarsen(bits).tolist() == [1, (1 << 1) | (1 << 31)]
    assert oref.coarsen(np.full(64 * 32, 255, np.uint8)).tolist() == [0xFFFFFFFF]
    with pytest.raises(AssertionError):
        oref.coarsen(np.zeros(64 * 8, np.uint8))


# ------------------------------------------------------------------------------------------------ the helpers reject near misses
def test_helpers_reject_near_misses():
    a = np.array([1.0, 2.0, 0.0, NAN], F32)
    assert oref.same_bits(a, a.copy())
    for i, v in ((1, up(2.0)), (2, F32(-0.0)), (3, oref.poison(1)[0])):
        b = a.copy()
        b[i] = v
        assert not oref.same_bits(a, b)
    assert not oref.same_bits(a, a.astype(F64)) and not oref.same_bits(a, a[:3])
    bits = np.array([3, 0, 255], np.uint8)
    flipped = bits.copy()
    flipped[1] ^= 0x10
    assert oref.same_bytes(bits, bits.copy()) and not oref.same_bytes(bits, flipped) and not oref.same_bytes(bits, bits[:2])
    # band_clear: a cell planted at the mean is in the band
    grid, tmp = oref.merge_inputs(8192, 1, "mean")
    after, s64, cnt = oref.merge(grid, tmp, 0.95)
    assert oref.band_clear(after, s64, cnt, 8192)
    pos = np.flatnonzero(after > 0)[0]
    planted = after.copy()
    planted[pos] = F32(s64 / cnt)
    _, s2, c2 = oref.merge(planted, np.zeros_like(planted), 1.0)
    planted[pos] = F32(s2 / c2)
    _, s2, c2 = oref.merge(planted, np.zeros_like(planted), 1.0)
    assert not oref.band_clear(planted, s2, c2, 8192)
    # the sum bound is tight enough to see one partial of 8 go missing at the fixture's size
    ps, pc = oref.merge_partials32(after)
    short = oref.pack_totals32(ps[:-1], pc[:-1])[0]
    assert abs(float(short) - s64) > oref.merge_sum_bound(8192) * s64
    # Candidates.holds with the merge as transform: a cell one ulp off its candidate is refused
    idx, sig = np.array([1, 1, 3], np.int32), np.array([5.0, 6.0, 0.5], F32)
    before = np.array([1.0, 2.0, -1.0, 4.0], F32)
    cand = oref.scatter(idx, sig, np.zeros(4, F32))
    tr = lambda cells, v: oref.merge(before[cells], v, 0.95)[0]
    ok = np.array([F32(1) * F32(0.95), 6.0, -1.0, F32(4) * F32(0.95)], F32)
    assert cand.holds(ok, tr).all()
    for i in range(4):
        off = ok.copy()
        off[i] = up(off[i])
        assert cand.holds(off, tr).tolist() == [j != i for j in range(4)]
