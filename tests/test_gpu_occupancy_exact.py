"""The occupancy-update kernels -- csrc/occupancy.hip: ngp_occ_compact, ngp_occ_sample, ngp_occ_all_cells, ngp_occ_scatter,
ngp_occ_scatter_max, ngp_occ_merge, ngp_occ_pack; csrc/march.hip: ngp_bitfield_coarsen -- through the C ABI, and
OccupancyUpdater.update through its hooks, against tests/occupancy_reference.py (numpy, float64 contract + float32 restatement in
the kernels' order; tests/test_occupancy_reference.py shows on the CPU that it reproduces the reference project's own vectors).

Every tolerance here is zero, set membership, or one of the two bounds derived in the reference's docstring (merge_sum_bound for the
float32 sum of the positive cells, POS_BOUND for a position against its float64 value).  Outputs start from a poison pattern and
carry a guard behind their last element.  The merge tests print the measured |stats[0] - sum64| / (bound sum64) per size
(pytest -s); profiles/PARITY_NOTES.md records them."""
import numpy as np
import pytest
import torch

import occupancy_reference as oref
from occupancy_reference import F32, F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 16
CAP = 0.01 * 1024 / 3**0.5                 # train.py:180, 5.912...
DECAY = 0.95
NAN, INF = F32(np.nan), F32(np.inf)
LAST = F32(1.0 - 2.0**-24)
_inputs = {}


def _ptr(t):
    from ngp_hip import ops
    return ops._ptr(t)


def _stream():
    from ngp_hip import ops
    return ops._stream()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def fpoison(n):
    return torch.full((n,), oref.POISON_BITS, device=DEV, dtype=torch.int32).view(torch.float32)


def is_poison(a):
    return bool(np.all(oref.bits32(np.ascontiguousarray(a, dtype=F32).reshape(-1)) == oref.POISON_BITS))


def guarded(a):
    """Device copy of a float32 array with GUARD poison elements behind it."""
    t = fpoison(a.size + GUARD)
    t[:a.size] = dev(np.asarray(a, F32).reshape(-1))
    return t


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def inputs(n, branch):
    if (n, branch) not in _inputs:
        grid, tmp = oref.merge_inputs(n, 100 + n % 997, branch, CAP, DECAY)
        _inputs[n, branch] = (grid, tmp) + oref.merge(grid, tmp, DECAY)
    return _inputs[n, branch]


# ---------------------------------------------------------------------------------------------------------------- merge + pack
def run_merge(L, grid, tmp, stats=None, decay=DECAY):
    n = grid.size
    g, t = guarded(grid), dev(np.asarray(tmp, F32).reshape(-1))
    stats = fpoison(L.ngp_occ_stats_floats()) if stats is None else stats
    assert L.ngp_occ_merge(_ptr(g), _ptr(t), decay, n, _ptr(stats), _stream()) == 0
    torch.cuda.synchronize()
    assert is_poison(host(g[n:])), "merge wrote behind the grid"
    return g, stats


def run_pack(L, g, stats, n, cap=CAP):
    bits = torch.full((n // 8 + GUARD,), 0xA5, device=DEV, dtype=torch.uint8)
    assert L.ngp_occ_pack(_ptr(g), _ptr(stats), cap, n // 8, _ptr(bits), _stream()) == 0
    torch.cuda.synchronize()
    assert bool((bits[n // 8:] == 0xA5).all()), "pack wrote behind the bitfield"
    return host(bits[:n // 8])


def judge_merge(n, after, s64, cnt, g, stats):
    """Grid and per-block partials of one merge; returns the partials."""
    B = oref.merge_blocks(n)
    st = host(stats)
    assert oref.same_bits(host(g[:n]), after), "grid after the merge"
    ps, pc = st[2:2 + 2 * B:2], st[3:3 + 2 * B:2]
    assert float(pc.astype(F64).sum()) == cnt, "count partials"
    ps32, pc32 = oref.merge_partials32(after)
    assert oref.same_bits(ps, ps32) and oref.same_bits(pc, pc32), "partials against the float32 restatement"
    if s64 > 0 and np.isfinite(s64):
        assert abs(float(ps.astype(F64).sum()) - s64) <= oref.merge_sum_bound(n) * s64
    return ps, pc


def judge_pack(L, n, after, s64, cnt, g, stats, bits, cap=CAP, band_free=True):
    """Totals, threshold and bitfield of one pack, judged both ways; returns (error of the sum / its bound, cells left out)."""
    st = host(stats)
    tot32, cnt32 = oref.merge_sum32(after)
    assert float(st[1]) == cnt, "stats[1]"
    assert oref.same_bits(st[:2], np.array([tot32, cnt32], F32)), "stats[0..1] against the float32 restatement"
    ratio = 0.0
    if cnt > 0 and np.isfinite(s64):
        ratio = abs(float(st[0]) - s64) / (oref.merge_sum_bound(n) * s64)
        assert ratio <= 1.0, "stats[0] outside merge_sum_bound"
    thr32 = oref.threshold32(st[0], st[1], cap)                            # the kernel's own threshold, one rounded division
    assert oref.same_bytes(bits, oref.pack(after, thr32)), "bitfield at the kernel's threshold"
    thr64 = oref.threshold64(s64, cnt, cap)
    want64 = oref.pack(after, thr64)
    if band_free:
        assert oref.same_bytes(bits, want64), "bitfield at the float64 threshold"
        excluded = 0
    else:                                   # data that no generator cleared: the cells inside the band are the only ones left out
        mean = s64 / cnt if cnt else 0.0
        inband = np.abs(after.reshape(-1).astype(F64) - mean) <= 4.0 * oref.merge_sum_bound(n) * mean
        diff = np.unpackbits(bits ^ want64, bitorder="little").astype(bool)
        assert not (diff & ~inband).any(), "bitfield at the float64 threshold, outside the band"
        excluded = int(inband.sum())
    other = torch.full((n // 8 + GUARD,), 0xA5, device=DEV, dtype=torch.uint8)
    assert L.ngp_packbits(_ptr(g), float(thr32), n // 8, _ptr(other), _stream()) == 0
    torch.cuda.synchronize()
    assert oref.same_bytes(host(other[:n // 8]), bits) and bool((other[n // 8:] == 0xA5).all()), "ngp_packbits at the same threshold"
    return ratio, excluded


@pytest.mark.parametrize("branch", ["mean", "cap", "none"])
@pytest.mark.parametrize("n", oref.MERGE_SIZES)
def test_merge_pack(hip_lib, n, branch):
    L = hip_lib
    grid, tmp, after, s64, cnt = inputs(n, branch)
    if branch == "mean":
        assert s64 / cnt < CAP and oref.band_clear(after, s64, cnt, n)
    elif branch == "cap":
        assert s64 / cnt > CAP
    else:
        assert cnt == 0
    g, stats = run_merge(L, grid, tmp)
    judge_merge(n, after, s64, cnt, g, stats)
    bits = run_pack(L, g, stats, n)
    assert oref.same_bits(host(g[:n]), after), "the pack changed the grid"
    ratio, _ = judge_pack(L, n, after, s64, cnt, g, stats, bits)
    assert is_poison(host(stats)[2 + 2 * oref.merge_blocks(n):]), "partials behind the last block"
    if branch == "none":
        assert not bits.any()
    else:
        assert bits.any() and not (bits == 255).all()
    print("merge+pack n = %d (%s): D = %d, bound = %.3e, |stats[0] - sum64| / (bound sum64) = %.4f"
          % (n, branch, oref.merge_depth(n), oref.merge_sum_bound(n), ratio))


@pytest.mark.parametrize("n", [1, 3, 5, 1027])
def test_merge_tail(hip_lib, n):
    """n & 3 != 0: the scalar tail of block 0, checked on the grid and on the partials summed on the host."""
    rng = np.random.default_rng(n)
    grid = (rng.random(n) * 3 + 0.5).astype(F32)
    tmp = np.where(rng.random(n) < 0.5, grid * F32(2), 0).astype(F32)
    grid[-1], tmp[-1] = 2.0, 7.0                                          # the very last cell is a tail cell and moves
    if n > 1:
        grid[-2] = -1.0
    after, s64, cnt = oref.merge(grid, tmp, DECAY)
    assert after[-1] == 7.0 and cnt == n - (n > 1)
    g, stats = run_merge(hip_lib, grid, tmp)
    ps, pc = judge_merge(n, after, s64, cnt, g, stats)
    assert ps.size == oref.merge_blocks(n) and is_poison(host(stats)[:2])  # the merge leaves the totals to the pack


def test_merge_pack_ignores_stale_partials(hip_lib):
    """A merge at the largest size fills all 512 partials; a merge + pack at 8192 cells on the same stats buffer uses 8 of them."""
    L = hip_lib
    big = oref.MERGE_SIZES[-1]
    grid, tmp, after, s64, cnt = inputs(big, "cap")
    _, stats = run_merge(L, grid, tmp)
    assert not is_poison(host(stats)[2 + 2 * 511:]) and float(host(stats)[2 + 2 * 511]) > 0
    n = 8192
    grid, tmp, after, s64, cnt = inputs(n, "mean")
    g, stats = run_merge(L, grid, tmp, stats)
    judge_merge(n, after, s64, cnt, g, stats)
    bits = run_pack(L, g, stats, n)
    judge_pack(L, n, after, s64, cnt, g, stats, bits)


def test_pack_is_strict_at_the_cap(hip_lib):
    cap32 = F32(CAP)
    n = 8192
    grid, tmp, _, _, _ = inputs(n, "cap")
    grid, tmp = grid.copy(), tmp.copy()
    at = [40, 41, 42, 8191, 8190, 8189]
    grid[at] = 0
    tmp[at] = [cap32, up(cap32), down(cap32)] * 2
    after, s64, cnt = oref.merge(grid, tmp, DECAY)
    assert s64 / cnt > CAP and oref.same_bits(after[at[:3]], np.array([cap32, up(cap32), down(cap32)], F32))
    g, stats = run_merge(hip_lib, grid, tmp)
    bits = run_pack(hip_lib, g, stats, n)
    judge_pack(hip_lib, n, after, s64, cnt, g, stats, bits)
    cells = np.unpackbits(bits, bitorder="little")
    assert cells[at].tolist() == [0, 1, 0, 0, 1, 0]


def test_merge_pack_non_finite(hip_lib):
    """The pinned rules: invisible cells ignore tmp; a NaN tmp loses; a NaN grid cell takes tmp and is never counted as NaN;
    +inf survives, is counted, and sends the threshold to the cap."""
    d = F32(DECAY)
    grid = np.array([-1, -1, 0, 0, 2, 2, 2, 2, NAN, NAN, NAN, INF, 2, 2, 0, 2], F32)
    tmp = np.array([5, NAN, 0, 3, 0, 1, F32(2) * d, 4, 3, 0, NAN, 1, NAN, INF, -3, -1], F32)
    gd = F32(2) * d
    want = np.array([-1, -1, 0, 3, gd, gd, gd, 4, 3, 0, NAN, INF, gd, INF, 0, gd], F32)
    for with_inf in (True, False):
        gr, tm, wa = grid.copy(), tmp.copy(), want.copy()
        if not with_inf:
            gr[11], tm[13], wa[11], wa[13] = 9.0, 9.0, F32(9) * d, 9.0
        after, s64, cnt = oref.merge(gr, tm, DECAY)
        assert oref.same_bits(after, wa) and cnt == 10 and np.isinf(s64) == with_inf
        g, stats = run_merge(hip_lib, gr, tm)
        judge_merge(16, after, s64, cnt, g, stats)
        bits = run_pack(hip_lib, g, stats, 16)
        judge_pack(hip_lib, 16, after, s64, cnt, g, stats, bits, band_free=with_inf)
        if with_inf:
            assert np.isinf(host(stats)[0]) and bits.tolist() == [0, 0b00101000]      # the cap: only the infinities exceed it
        else:
            mean = s64 / cnt
            assert mean < CAP and bits.tolist() == oref.pack(after, mean).tolist() == [0b10000000, 0b00101000]


# ---------------------------------------------------------------------------------------------------------------- compaction
def run_compact(L, grid, thr):
    n = grid.size
    lst = torch.full((n + GUARD,), -1, device=DEV, dtype=torch.int32)
    cnt = torch.full((1,), -7, device=DEV, dtype=torch.int32)
    scratch = torch.full((1024,), -3, device=DEV, dtype=torch.int32)
    g = dev(grid)
    assert L.ngp_occ_compact(_ptr(g), float(thr), n, _ptr(lst), _ptr(cnt), _ptr(scratch), _stream()) == 0
    torch.cuda.synchronize()
    return lst, cnt


@pytest.mark.parametrize("n_cells", [1, 63, 65, 65536, 65537])
def test_compact_sizes_and_planted_cells(hip_lib, n_cells):
    """Sizes around one wave, and around 65536, where the per-wave chunk doubles and half the waves go empty; cells equal to the
    threshold, NaN, -1 and +inf; an empty result; a full one."""
    thr = F32(0.625)
    rng = np.random.default_rng(n_cells)
    grid = rng.random(n_cells, dtype=F32)
    plant = np.array([thr, NAN, -1, INF, up(thr), down(thr)], F32)
    if n_cells >= 63:
        for at in (0, n_cells - 6, n_cells // 2):
            grid[at:at + 6] = plant
    else:
        grid[0] = up(thr)
    for g, t in ((grid, thr), (np.minimum(grid, F32(0.5)), thr), (np.full(n_cells, 1.0, F32), thr), (np.full(n_cells, thr, F32), thr)):
        want, count = oref.compact(g, t)
        lst, cnt = run_compact(hip_lib, g, t)
        assert int(cnt) == count
        assert np.array_equal(host(lst[:count]), want) and bool((lst[count:] == -1).all())
    assert oref.compact(grid, thr)[1] > 0 and oref.compact(np.minimum(grid, F32(0.5)), thr)[1] == 0


# ---------------------------------------------------------------------------------------------------------------- sample
def uniforms_with_edges(rng, m, extra=()):
    u = rng.random(m, dtype=F32)
    edges = [F32(1.0), LAST, F32(0.0)] + list(extra)
    for k, e in enumerate(edges[:m]):
        u[(k * 7919) % m if m > len(edges) else k] = e
    return u


def run_sample(L, u_cell, u_pick, u_jit, lst_dev, cnt_dev, M, G, s, hg):
    idx = torch.full((2 * M + GUARD,), -9, device=DEV, dtype=torch.int32)
    xyz = fpoison(6 * M + GUARD)
    uc, up_, uj = dev(u_cell), dev(u_pick), dev(u_jit)
    assert L.ngp_occ_sample(_ptr(uc), _ptr(up_), _ptr(uj), _ptr(lst_dev), _ptr(cnt_dev), M, G, float(s), float(hg), _ptr(idx), _ptr(xyz),
                            _stream()) == 0
    torch.cuda.synchronize()
    assert bool((idx[2 * M:] == -9).all()) and is_poison(host(xyz[6 * M:]))
    return host(idx[:2 * M]), host(xyz[:6 * M]).reshape(-1, 3)


def judge_positions(got, cells_idx, u_jit, G, s, hg):
    cells = oref.morton_invert(cells_idx)
    assert oref.same_bits(got, oref.positions(cells, u_jit, G, s, hg, F32)), "positions against the float32 restatement"
    assert np.abs(got.astype(F64) - oref.positions(cells, u_jit, G, s, hg, F64)).max() <= oref.pos_bound(s)


@pytest.mark.parametrize("G", [2, 16, 128])
@pytest.mark.parametrize("M", [1, 128, 1000])
def test_sample(hip_lib, M, G):
    """2 M threads = 2, exactly one block, 2000; u = 0, 1 - 2^-24 and exactly 1 in both halves (the clamps); hand-made lists of
    0, 1, 3 and (G = 128) 2^21 - 1 cells and a list chained from ngp_occ_compact."""
    L, G3 = hip_lib, G**3
    rng = np.random.default_rng(1000 * G + M)
    lists = [np.zeros(0, np.int32), np.array([5], np.int32), np.array([1, 4, 6], np.int32)]
    if G == 128:
        lists.append(np.arange(1, 2**21, dtype=np.int32))
    grid = rng.random(G3, dtype=F32)
    lists.append("chained")
    for c, lst in enumerate(lists):
        s, hg = oref.cascade_extent(c % 3, 2.0, G)
        u_cell = uniforms_with_edges(rng, M)
        u_pick = uniforms_with_edges(rng, M, [F32(0.4032384753227234)])   # times 2^21 - 1: float32 and float64 pick different cells
        if M == 1:
            u_cell[0], u_pick[0] = (F32(1.0), F32(1.0)) if c % 2 == 0 else (LAST, LAST)
        u_jit = uniforms_with_edges(rng, 6 * M).reshape(-1, 3)
        if isinstance(lst, str):
            lst_dev, cnt_dev = run_compact(L, grid, 0.7)
            lst, count = oref.compact(grid, 0.7)
            assert count > 0
        else:
            count = lst.size
            lst_dev = torch.full((max(count, 1) + GUARD,), G3 + 5, device=DEV, dtype=torch.int32)
            lst_dev[:count] = dev(lst)
            cnt_dev = dev(np.array([count], np.int32))
        idx, xyz = run_sample(L, u_cell, u_pick, u_jit, lst_dev, cnt_dev, M, G, s, hg)
        want = oref.sample_indices(u_cell, u_pick, lst, count, M, G)
        assert np.array_equal(idx, want), "indices (list of %d)" % count
        assert idx.min() >= 0 and idx.max() < G3
        judge_positions(xyz, idx, u_jit, G, s, hg)
        if count == 0:
            assert not idx[M:].any()


@pytest.mark.parametrize("G,cascades", [(2, 3), (16, 3), (128, 1)])
def test_all_cells(hip_lib, G, cascades):
    G3 = G**3
    rng = np.random.default_rng(G)
    for c in range(cascades):
        s, hg = oref.cascade_extent(c, 2.0, G)
        u_jit = uniforms_with_edges(rng, 3 * G3).reshape(-1, 3)
        xyz = fpoison(3 * G3 + GUARD)
        uj = dev(u_jit)
        assert hip_lib.ngp_occ_all_cells(_ptr(uj), G3, G, float(s), float(hg), _ptr(xyz), _stream()) == 0
        torch.cuda.synchronize()
        assert is_poison(host(xyz[3 * G3:]))
        got = host(xyz[:3 * G3]).reshape(-1, 3)
        judge_positions(got, np.arange(G3), u_jit, G, s, hg)
        assert oref.same_bits(got, oref.all_cells(u_jit, G, s, hg))


# ---------------------------------------------------------------------------------------------------------------- scatter
def densities(rng, n):
    sig = (rng.random(n, dtype=F32) * 10 + F32(0.01)).astype(F32)
    special = np.array([0.0, -1.5, NAN, INF, 1e-42, 3e-39, -0.0, 1e-45], F32)
    for k, v in enumerate(special):
        sig[k * 13 % n::29][:max(1, n // 64)] = v
    if n < 29:
        sig[:] = special[:n] if n > 1 else F32(2.5)
    return sig


def index_patterns(rng, n):
    size = 2 * n + 3
    return {"unique": (rng.permutation(size)[:n].astype(np.int32), size), "seven": (rng.integers(0, 7, n).astype(np.int32) * 3, 24),
            "null": (None, n)}


def run_scatter(L, fn, idx, sig, tmp):
    n = sig.size
    i, sg = None if idx is None else dev(idx), dev(sig)
    assert getattr(L, fn)(_ptr(i), _ptr(sg), n, _ptr(tmp), _stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("pattern", ["unique", "seven", "null"])
@pytest.mark.parametrize("n", [1, 256, 257, 4096])
def test_scatter_max(hip_lib, n, pattern):
    """The deterministic scatter: per cell exactly the largest strictly positive draw (zeros, negatives and NaN dropped, +inf and
    denormals kept), the same bits on a second run, untouched cells and the guard as they were."""
    rng = np.random.default_rng(n)
    idx, size = index_patterns(rng, n)[pattern]
    sig = densities(rng, n)
    neg_poison = np.full(size, 0xFFA5A5A5, np.uint32).view(F32)           # a negative bit pattern: any positive draw beats it
    for init in (np.zeros(size, F32), neg_poison):
        want = oref.scatter_max(idx, sig, init)
        tmp = guarded(init)
        run_scatter(hip_lib, "ngp_occ_scatter_max", idx, sig, tmp)
        first = host(tmp).copy()
        assert oref.same_bits(first[:size], want) and is_poison(first[size:])
        run_scatter(hip_lib, "ngp_occ_scatter_max", idx, sig, tmp)
        assert oref.same_bits(host(tmp), first)
    cells = np.arange(n) if idx is None else idx
    with np.errstate(invalid="ignore"):
        pos = sig > 0
    untouched = np.ones(size, bool)
    untouched[cells[pos]] = False
    assert oref.same_bits(want[untouched], neg_poison[untouched])
    if n >= 256 and pattern != "seven":
        assert untouched[cells].any() and np.isinf(want).any() and (want[~untouched] < 1e-38).any()   # dropped draws, inf, denormals


@pytest.mark.parametrize("pattern", ["unique", "seven", "null"])
@pytest.mark.parametrize("n", [1, 256, 257, 4096])
def test_scatter_plain(hip_lib, n, pattern):
    """The default scatter: every drawn cell ends up holding one of the values drawn for it -- whatever they are, NaN included --
    and every other cell its poison."""
    rng = np.random.default_rng(n + 1)
    idx, size = index_patterns(rng, n)[pattern]
    sig = densities(rng, n)
    cand = oref.scatter(idx, sig, oref.poison(size))
    tmp = fpoison(size + GUARD)
    run_scatter(hip_lib, "ngp_occ_scatter", idx, sig, tmp)
    got = host(tmp)
    assert cand.holds(got[:size]).all() and is_poison(got[size:])
    assert is_poison(got[:size][~cand.touched]) and cand.touched.sum() == (n if idx is None else np.unique(idx).size)


# ---------------------------------------------------------------------------------------------------------------- coarsen
def bit_patterns(C, G, rng):
    n_bytes = C * G**3 // 8
    empty = np.zeros(n_bytes, np.uint8)
    every2 = [empty.copy(), empty.copy()]
    for k, (at, val) in enumerate(((0, 0x01), (63, 0x80))):
        every2[k][at::128] = val                                         # first / last byte of every second 512-cell block
        every2[k][-64 + at] = val                                        # and of the very last block
    sparse = np.packbits(rng.random(n_bytes * 8) < 0.01, bitorder="little")
    return {"empty": empty, "full": np.full(n_bytes, 255, np.uint8), "first": every2[0], "last": every2[1], "sparse": sparse}


@pytest.mark.parametrize("C,G", [(4, 16), (1, 32), (1, 128), (2, 128)])
def test_coarsen(hip_lib, C, G):
    """(4, 16) is one word, written by lane 0 alone; (1, 32) is the first shape in which lane 32 writes the odd word."""
    rng = np.random.default_rng(C * G)
    n_words = C * G**3 // 512 // 32
    for name, bits in bit_patterns(C, G, rng).items():
        want = oref.coarsen(bits)
        assert want.size == n_words
        out = torch.full((n_words + GUARD,), 0x5EADBEEF, device=DEV, dtype=torch.int32)
        b = dev(bits)
        assert hip_lib.ngp_bitfield_coarsen(_ptr(b), C, G, _ptr(out), _stream()) == 0
        torch.cuda.synchronize()
        got = host(out).view(np.uint32)
        assert np.array_equal(got[:n_words], want), name
        assert (got[n_words:] == 0x5EADBEEF).all(), name
    assert oref.coarsen(bit_patterns(C, G, rng)["first"]).any() and not oref.coarsen(bit_patterns(C, G, rng)["empty"]).any()


@pytest.mark.parametrize("C,G", [(1, 16), (3, 8), (0, 128)])
def test_coarsen_rejects(hip_lib, C, G):
    bits = torch.full((max(C, 1) * G**3 // 8,), 255, device=DEV, dtype=torch.uint8)
    out = torch.full((64,), 0x5EADBEEF, device=DEV, dtype=torch.int32)
    assert hip_lib.ngp_bitfield_coarsen(_ptr(bits), C, G, _ptr(out), _stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 0x5EADBEEF).all())


# ---------------------------------------------------------------------------------------------------------------- whole update
class _Grid:
    """What OccupancyUpdater reads of a model, for a grid driven through density_fn alone."""

    def __init__(self, G, C, scale, grid, det):
        self.grid_size, self.cascades, self.scale = G, C, scale
        self.density_grid = dev(grid).clone()
        self.density_bitfield = torch.full((C * G**3 // 8,), 0xA5, dtype=torch.uint8, device=DEV)
        self._ngp_deterministic = det


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "default"])
@pytest.mark.parametrize("G,C,scale,amps", [(128, 1, 0.5, (4.0, 10.0, 10.0, 200.0)), (32, 3, 2.0, (4.0, 30.0, 30.0, 4000.0))])
def test_whole_update(hip_lib, monkeypatch, G, C, scale, amps, det):
    """A warm-up and three sampled updates through OccupancyUpdater.update with all three hooks: the positions handed to density_fn
    are bit-equal to the reference's, the densities are an analytic blob of them, scaled so that the first three updates take the
    mean branch and the last the cap.  Deterministic mode: grid bit-equal, bitfield as in merge + pack (the float64 judgement leaves
    out only cells inside the band, which this data was not cleared of).  Default mode: every cell holds the merge of one of its
    candidates, the bitfield is exact against the device's own grid, and the next update starts from that grid."""
    from ngp_hip.occupancy import OccupancyUpdater
    monkeypatch.delenv("NGP_DETERMINISTIC", raising=False)
    G3, n = G**3, C * G**3
    M = G3 // 4
    rng = np.random.default_rng(G + det)
    grid = np.where(rng.random((C, G3)) < 0.1, -1, 0).astype(F32)
    m = _Grid(G, C, scale, grid, det)
    upd = OccupancyUpdater(m)
    branches = []
    for k, amp in enumerate(amps):
        warm = k == 0
        rows = G3 if warm else 2 * M
        jit = [uniforms_with_edges(rng, 3 * rows).reshape(-1, 3) for _ in range(C)]
        uni = [(uniforms_with_edges(rng, M), uniforms_with_edges(rng, M)) for _ in range(C)]
        ref = oref.update(grid, G, scale, CAP, DECAY, warm, jit, lambda c, xyz, idx: oref.blob(xyz, amp), uniforms=uni, det=det)
        seen = []

        def density_fn(c, xyzs, indices):
            seen.append(oref.same_bits(host(xyzs), ref["xyz"][c]) and (warm or np.array_equal(host(indices), ref["indices"][c])))
            return dev(ref["sigma"][c])
        upd.update(CAP, warmup=warm, decay=DECAY, jitter=lambda c, r: dev(jit[c]), uniforms=lambda c: tuple(dev(u) for u in uni[c]),
                   density_fn=density_fn)
        torch.cuda.synchronize()
        assert seen == [True] * C, "positions / indices handed to density_fn"
        got, bits = host(m.density_grid), host(m.density_bitfield)
        if warm or det:
            after, s64, cnt = ref["grid"], ref["sum64"], ref["count"]
            assert oref.same_bits(got, after), "grid after update %d" % k
        else:
            for c in range(C):
                before_c = grid[c]
                merged = lambda cells, v: oref.merge(before_c[cells], v, DECAY)[0]
                assert ref["cand"][c].holds(got[c], merged).all(), "a cell holds none of its candidates (update %d)" % k
            after = got
            _, s64, cnt = oref.merge(after.reshape(-1), np.zeros(n, F32), 1.0)
        _, excluded = judge_pack(hip_lib, n, after.reshape(-1), s64, cnt, m.density_grid.view(-1), upd.stats, bits, band_free=False)
        assert excluded < 1e-4 * n
        branches.append(s64 / cnt < CAP)
        if not warm:
            assert all(oref.compact(grid[c], CAP)[1] > 0 for c in range(C)) == (k > 1)    # the empty list, then a real one
        grid = got.copy()
    assert branches == [True, True, True, False], branches
    assert 0.05 < (grid < 0).mean() < 0.15 and (grid[grid < 0] == -1).all()
