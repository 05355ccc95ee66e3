"""Independent reference of the occupancy-grid update (csrc/occupancy.hip: ngp_occ_compact, ngp_occ_sample, ngp_occ_all_cells,
ngp_occ_scatter, ngp_occ_scatter_max, ngp_occ_merge, ngp_occ_pack; csrc/march.hip: ngp_bitfield_coarsen; ngp_hip/occupancy.py:
OccupancyUpdater.update) -- the CPU side of tests/test_occupancy_reference.py and tests/test_gpu_occupancy_exact.py.  numpy only; it
imports neither the oracle nor the package under test.

Two layers where the arithmetic is floating point: a float64 contract (dtype=F64) and a float32 restatement with every rounding a
separate numpy float32 operation in the kernel's own order (dtype=F32; the library is built with -ffp-contract=off and without
fast-math, float32 division is correctly rounded, so the restatement is bit for bit what the kernel computes).  Everything that
is integer or a comparison (compaction, Morton codes, scatter, counts, packbits, coarsen) has one exact form.

The update (modules/networks.py:181-209, 255-290), per cascade c of C, G^3 cells each, cell i <-> Morton code i:
    s = min(2^(c-1), scale), half_grid = s / G                                  (the float32 values that cross the C ABI)
    warm-up:  every cell i, position from the jitter row i                     (all_cells)
    sampled:  M = G^3 / 4 uniform cells  idx = min(int(f64(u_cell) G^3), G^3 - 1)
              M cells from the occupied list (cells with grid > cap, in cell order; compact):
                  k = min(int(f32(u_pick) * f32(n_occ)), n_occ - 1) -- ONE float32 product, truncated -- idx = list[k];
                  n_occ == 0: cell 0 stands in (its density is only ever max-merged)                             (sample)
    position: x_k = ((f32(c_k) / f32(G - 1)) * 2 - 1) * (s - half_grid) + (u_jit * 2 - 1) * half_grid, c = Morton inverse of idx
    tmp = 0; tmp[idx] = density   (scatter: any of the values drawn for the cell;  scatter_max, deterministic mode: the largest
                                   strictly positive one; the warm-up writes every cell once)
then over all C G^3 cells:
    grid = where(grid < 0, grid, max(grid * decay, tmp))      in float32, exact per cell                       (merge)
    mean = sum(grid[grid > 0]) / count(grid > 0);  thr = min(mean, cap);  bit i = grid[i] > thr, little-endian    (pack)
    coarse bit j = any bit of bytes 64 j .. 64 j + 63 (one 8^3 block of 512 cells), little-endian in uint32    (coarsen)

Edge rules, as the kernels have them (each is pinned by a test):
  * Every comparison is strict: a cell EQUAL to the threshold is not occupied, neither in the compaction nor in the bitfield.
  * A NaN or non-positive density never reaches the grid.  The max scatter drops it (`s > 0` is false for NaN, 0, -0 and negatives;
    a positive denormal is positive and is kept).  The plain scatter stores whatever it is given, but the merge's fmaxf returns the
    OTHER operand when one is NaN -- unlike torch.maximum, which propagates NaN -- so a NaN in tmp leaves grid * decay, and a
    negative or zero tmp loses against grid * decay >= 0.
  * A NaN grid cell is not `< 0`, so it is merged: fmaxf(NaN * decay, tmp) = tmp.  The cell is replaced by tmp; it is counted as
    positive only if that tmp is > 0 (never as NaN: NaN > 0 is false), and a NaN in both leaves NaN, uncounted, bit clear.
  * +inf survives the merge (inf * decay = inf), is counted, and makes the sum and the mean +inf: the threshold falls back to the cap.
  * No positive cell: the mean is 0 / 0 = NaN, fminf(NaN, cap) = cap (again the non-NaN operand); no cell exceeds it, every bit is clear.
  * Invisible cells (grid < 0, in practice -1) are never changed, counted or set, whatever tmp holds.
  * The max scatter compares bit patterns as signed integers against what tmp holds (0 by contract: bit pattern 0); positive floats
    order like their bit patterns, so this is the float maximum.  It is idempotent and order-free: a second run gives the same bits.
  * grid is assumed to hold no -0 (it starts at 0 or -1 and only ever receives max(.)): the sign of fmaxf(-0, +0) is not pinned.

Bounds the GPU tests use (u = 2^-24, one float32 rounding).

merge_sum_bound(n).  All terms are positive, so a sum formed by any tree of float32 additions in which no term passes through more
than D additions is within gamma_D = D u / (1 - D u) of the exact sum, relatively.  D is read off occ_merge_kernel and
occ_pack_kernel (merge_depth):
    B = min(max(ceil(ceil(n / 256) / 4), 1), 512) blocks of 256 threads;  t = ceil((n >> 2) / (256 B)) grid-stride trips
    a thread adds 4 cells per trip, serially:                       4 t      (the first of them to 0: counted, not exploited)
    the n & 3 tail adds one more cell to a thread of block 0:       1
    wave butterfly (xor 32 .. 1):                                   6
    (ps0 + ps1) + (ps2 + ps3):                                      2
    occ_pack_kernel, thread b adds partials b, b + 256, ...:        ceil(B / 256)
    butterfly, four partials:                                       6 + 2
    D(n) = 4 t + ceil(B / 256) + 17
and merge_sum_bound(n) = gamma_D + u, the extra u being the division total / count (count is an exact integer below 2^24 at every
size used): |thr32 - thr64| <= merge_sum_bound(n) (1 + gamma_D) mean.  The generator keeps every cell 4 merge_sum_bound(n) mean away
from the float64 mean, so the float64 threshold and the device's select the same cells.  The float64 sum itself (numpy's pairwise
sum) is within 1e-15 of the exact sum, 8 orders below u.

POS_BOUND(s) = 8 u s per coordinate.  With a = (c / (G - 1)) 2 - 1 in [-1, 1] and j = u_jit 2 - 1 in [-1, 1]: the quotient is
off by u, doubling is exact, the subtraction rounds to u |a| <= u: |a32 - a| <= 3 u.  (s - half_grid) rounds once, the product once:
|base32 - base| <= (3 + 1 + 1) u (s - half_grid).  u_jit 2 is exact, the subtraction rounds (u), the product by half_grid rounds (u):
2 u half_grid.  The last sum rounds a result of magnitude <= s: u s.  Total <= 5 u (s - hg) + 2 u hg + u s <= 6 u s to first order;
8 u s leaves the second-order terms ample room (they are below 40 u^2 s).
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0**-24
MERGE_MAX_BLOCKS = 512
POISON_BITS = 0x7FA5A5A5          # a NaN with a payload: float poison that no arithmetic here produces


def f32(x):
    return np.asarray(x, dtype=F32)


def bits32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == F32
    return a.view(np.uint32)


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays (NaN payloads and the sign of zero included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == F32 and b.dtype == F32 and a.shape == b.shape and bool(np.array_equal(bits32(a), bits32(b)))


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.dtype.kind in "iu" and a.shape == b.shape and bool(np.array_equal(a, b))


def poison(shape):
    return np.full(shape, POISON_BITS, np.uint32).view(F32)


# ---------------------------------------------------------------------------------------------------------------- Morton codes
def _spread(x):
    x = np.asarray(x, np.uint64) & np.uint64(0x3FF)
    x = (x | (x << np.uint64(16))) & np.uint64(0x030000FF)
    x = (x | (x << np.uint64(8))) & np.uint64(0x0300F00F)
    x = (x | (x << np.uint64(4))) & np.uint64(0x030C30C3)
    x = (x | (x << np.uint64(2))) & np.uint64(0x09249249)
    return x


def morton(coords):
    """[n, 3] cell coordinates (each < 1024) -> Morton code, x in bit 0."""
    c = np.asarray(coords)
    return (_spread(c[:, 0]) | (_spread(c[:, 1]) << np.uint64(1)) | (_spread(c[:, 2]) << np.uint64(2))).astype(np.int32)


def morton_invert(idx):
    """Morton code -> [n, 3] cell coordinates, bit by bit (deliberately not the kernel's magic-number compaction)."""
    i = np.asarray(idx).astype(np.int64)
    out = np.zeros(i.shape + (3,), np.int32)
    for b in range(10):
        for k in range(3):
            out[..., k] |= (((i >> (3 * b + k)) & 1) << b).astype(np.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------- compaction
def compact(grid, thr):
    """(cells with grid > f32(thr), ascending, int32; their count).  NaN, -1 and a cell equal to thr are out; +inf is in."""
    with np.errstate(invalid="ignore"):
        lst = np.flatnonzero(f32(grid) > F32(thr)).astype(np.int32)
    return lst, int(lst.size)


# ---------------------------------------------------------------------------------------------------------------- positions
def positions(cells, u_jit, G, s, half_grid, dtype=F32):
    """cells [n, 3] integer coordinates, u_jit [n, 3] float32 uniforms; s and half_grid are the float32 values that cross the ABI."""
    T = dtype
    s, hg = T(F32(s)), T(F32(half_grid))
    c = np.asarray(cells).astype(T)
    q = c / T(G - 1)
    a = q * T(2) - T(1)
    base = a * T(s - hg)
    j = np.asarray(u_jit, F32).reshape(-1, 3).astype(T) * T(2) - T(1)
    out = base + j * hg
    assert out.dtype == T
    return out


def pos_bound(s):
    return 8.0 * U * float(s)


def all_cells(u_jit, G, s, half_grid, dtype=F32):
    return positions(morton_invert(np.arange(G**3)), u_jit, G, s, half_grid, dtype)


def sample_indices(u_cell, u_pick, lst, count, M, G):
    G3 = G**3
    u_cell, u_pick = f32(u_cell)[:M], f32(u_pick)[:M]
    uni = np.minimum((u_cell.astype(F64) * F64(G3)).astype(np.int64), G3 - 1)
    if count > 0:
        k = np.minimum((u_pick * F32(count)).astype(np.int64), count - 1)            # float32 product, truncated
        occ = np.asarray(lst)[k].astype(np.int64)
    else:
        occ = np.zeros(M, np.int64)
    return np.concatenate([uni, occ]).astype(np.int32)


def sample(u_cell, u_pick, u_jit, lst, count, M, G, s, half_grid, dtype=F32):
    """-> (indices [2M] int32, positions [2M, 3]); the first M rows are the uniform half."""
    idx = sample_indices(u_cell, u_pick, lst, count, M, G)
    return idx, positions(morton_invert(idx), u_jit, G, s, half_grid, dtype)


# ---------------------------------------------------------------------------------------------------------------- scatter
class Candidates:
    """Per cell, the set of float32 bit patterns it may hold after a scatter: the values drawn for it, or, undrawn, what it held."""

    def __init__(self, indices, values, init):
        init = f32(init)
        n = values.shape[0]
        self.cells = np.arange(n, dtype=np.int64) if indices is None else np.asarray(indices).astype(np.int64)
        assert self.cells.shape == (n,) and (n == 0 or (self.cells.min() >= 0 and self.cells.max() < init.size))
        self.values = f32(values)
        self.init = init.copy()
        self.touched = np.zeros(init.size, bool)
        self.touched[self.cells] = True

    def _keys(self, cells, vals):
        return (cells.astype(np.uint64) << np.uint64(32)) | bits32(f32(vals)).astype(np.uint64)

    def holds(self, got, transform=None):
        """Boolean per cell: got[cell] is (bit for bit) one of the cell's candidates.  transform(cells, values) -> values maps
        every candidate first (the merge, when the scattered buffer is only seen after it)."""
        got = f32(got)
        assert got.shape == self.init.shape
        tr = (lambda c, v: v) if transform is None else transform
        allc = np.arange(self.init.size, dtype=np.int64)
        ok = bits32(got) == bits32(f32(tr(allc, self.init)))
        drawn = np.isin(self._keys(allc, got), self._keys(self.cells, f32(tr(self.cells, self.values))))
        return np.where(self.touched, drawn, ok)


def scatter(indices, sigmas, init):
    """tmp[indices] = sigmas with duplicates unresolved (indices None: cell i = draw i, the warm-up form)."""
    return Candidates(indices, f32(sigmas), init)


def scatter_max(indices, sigmas, init):
    """The deterministic scatter, exact: per cell the signed-integer maximum of what it held and the strictly positive draws."""
    sig = f32(sigmas)
    out = np.ascontiguousarray(f32(init)).copy()
    cells = np.arange(sig.size, dtype=np.int64) if indices is None else np.asarray(indices).astype(np.int64)
    with np.errstate(invalid="ignore"):
        keep = sig > F32(0)
    np.maximum.at(out.view(np.int32), cells[keep], np.ascontiguousarray(sig[keep]).view(np.int32))
    return out


# ---------------------------------------------------------------------------------------------------------------- merge + pack
def merge(grid, tmp, decay):
    """-> (grid after, float32 bit-exact per cell; float64 sum of the cells > 0; their exact count)."""
    g, t = f32(grid), f32(tmp)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(g < 0, g, np.fmax(g * F32(decay), t)).astype(F32)                # fmax: a NaN operand loses
        pos = out > 0
    with np.errstate(invalid="ignore"):
        return out, float(out[pos].astype(F64).sum()), int(pos.sum())


def merge_blocks(n):
    return int(min(max(-(-(-(-n // 256)) // 4), 1), MERGE_MAX_BLOCKS))


def merge_depth(n):
    B = merge_blocks(n)
    t = -(-(n >> 2) // (256 * B))
    return 4 * t + -(-B // 256) + 17


def merge_sum_bound(n):
    D = merge_depth(n)
    return D * U / (1.0 - D * U) + U


def _butterfly(v):
    """wave_sum: v += shfl_xor(v, d) for d = 32 .. 1 on rows of 64 lanes; lane 0's value is the one the kernels keep."""
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ d]).astype(F32)
    return v[:, 0]


def _four(p):
    p = p.reshape(-1, 4)
    return ((p[:, 0] + p[:, 1]).astype(F32) + (p[:, 2] + p[:, 3]).astype(F32)).astype(F32)


def merge_partials32(after, n_blocks=None):
    """The per-block (sum, count) partials occ_merge_kernel leaves, in its own float32 order, from the merged grid."""
    g = f32(after).reshape(-1)
    n = g.size
    B = merge_blocks(n) if n_blocks is None else n_blocks
    T, n4 = 256 * B, n >> 2
    s, c = np.zeros(T, F32), np.zeros(T, F32)
    tid = np.arange(T)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(-(-n4 // T) if n4 else 0):
            i = tid + k * T
            live = i < n4
            ii = np.where(live, i, 0)
            for comp in range(4):
                v = g[4 * ii + comp]
                add = live & (v > 0)
                s = np.where(add, (s + v).astype(F32), s)
                c = np.where(add, c + F32(1), c)
        for k in range(n & 3):
            v = g[4 * n4 + k]
            if v > 0:
                s[k] = F32(s[k] + v)
                c[k] += F32(1)
        ps, pc = _butterfly(s.reshape(-1, 64)), _butterfly(c.reshape(-1, 64))
        return _four(ps), _four(pc)


def pack_totals32(psum, pcnt):
    """occ_pack_kernel's fixed-order sum of the partials -> (total, count) as float32."""
    n = psum.size
    s, c = np.zeros(256, F32), np.zeros(256, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(-(-n // 256)):
            seg_s, seg_c = psum[256 * k:256 * (k + 1)], pcnt[256 * k:256 * (k + 1)]
            s[:seg_s.size] = (s[:seg_s.size] + seg_s).astype(F32)
            c[:seg_c.size] = (c[:seg_c.size] + seg_c).astype(F32)
        return _four(_butterfly(s.reshape(4, 64)))[0], _four(_butterfly(c.reshape(4, 64)))[0]


def merge_sum32(after):
    """stats[0], stats[1] as the two kernels compute them."""
    return pack_totals32(*merge_partials32(after))


def threshold32(total, count, cap):
    """fminf(total / count, cap) with one correctly rounded float32 division; NaN (0 / 0) gives the cap."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return F32(np.fmin(F32(total) / F32(count), F32(cap)))


def threshold64(sum64, count, cap):
    """The contract: min(mean, cap) with the cap the float32 value that crosses the ABI; no positive cell, or an infinite sum: the cap."""
    cap = float(F32(cap))
    if count == 0 or not np.isfinite(sum64):
        return cap
    return min(sum64 / count, cap)


def pack(grid, thr):
    """Little-endian bytes of grid > thr (thr a float32 or a float64: the comparison is exact either way)."""
    g = f32(grid).reshape(-1)
    assert g.size % 8 == 0
    with np.errstate(invalid="ignore"):
        cmp = g > thr if isinstance(thr, F32) else g.astype(F64) > F64(thr)
    return np.packbits(cmp, bitorder="little")


def coarsen(bits):
    b = np.asarray(bits, np.uint8).reshape(-1)
    assert b.size % (64 * 32) == 0
    return np.packbits(b.reshape(-1, 64).any(1), bitorder="little").view("<u4").astype(np.uint32)


def band_clear(after, sum64, count, n):
    """No positive cell within 4 merge_sum_bound(n) mean of the float64 mean."""
    mean = sum64 / count
    g = f32(after).astype(F64)
    return not bool(np.any(np.abs(g - mean) <= 4.0 * merge_sum_bound(n) * mean))


# ---------------------------------------------------------------------------------------------------------------- generator
def merge_inputs(n, seed, branch, cap=5.912, decay=0.95, invisible=0.1, zeros=0.3):
    """Inputs for merge + pack: (grid, tmp).  branch 'mean': the mean of the merged positives lies below the cap and no cell is
    within 4 merge_sum_bound(n) mean of it; 'cap': it lies above; 'none': no positive cell after the merge.  A tenth of the
    cells invisible (-1, with a tmp that must be ignored), three tenths zero, the rest positive; tmp is zero, half of
    grid * decay, equal to it, or 1.5 times it, a quarter each (zero cells: zero or a fresh positive density)."""
    rng = np.random.default_rng(seed)
    scale = {"mean": 2.0, "cap": 40.0, "none": 0.0}[branch]
    kind = rng.random(n)
    grid = (rng.random(n) * scale).astype(F32) + F32(scale * 1e-3)
    grid[kind < invisible + zeros] = 0
    grid[kind < invisible] = -1
    gd = (grid * F32(decay)).astype(F32)
    sel = rng.integers(0, 4, n)
    fresh = (rng.random(n) * scale).astype(F32)
    tmp = np.select([sel == 0, sel == 1, sel == 2], [np.zeros(n, F32), gd * F32(0.5), gd], gd * F32(1.5)).astype(F32)
    tmp = np.where(grid == 0, np.where(sel < 2, F32(0), fresh), tmp).astype(F32)
    tmp = np.where(grid < 0, fresh, tmp).astype(F32)
    if branch == "none":
        return grid, np.zeros(n, F32)
    if n >= 8:                                    # one cell of each kind whatever the draw
        grid[:4] = [-1, 0, scale, scale * 0.5]
        tmp[:4] = [scale, scale * 0.25, 0, F32(F32(scale * 0.5) * F32(decay))]
    if branch == "mean":
        for _ in range(64):
            after, s64, cnt = merge(grid, tmp, decay)
            mean = s64 / cnt
            bad = np.abs(after.astype(F64) - mean) <= 4.0 * merge_sum_bound(n) * mean
            if not bad.any():
                break
            grid[bad] = 0                         # out of the band: the cell becomes a fresh density of twice the mean
            tmp[bad] = F32(2.0 * mean)
        else:
            raise AssertionError("band not cleared")
        assert mean < cap
    return grid, tmp


MERGE_SIZES = (8, 1032, 8192, 524288, 524296, 8 * (4096 * 256 + 1))     # what each reaches: tests/test_gpu_occupancy_exact.py


# ---------------------------------------------------------------------------------------------------------------- whole update
def blob(xyz, amp, width=0.35):
    """An analytic density for the whole-update tests: a Gaussian blob, evaluated in float64 from the positions, rounded once."""
    x = np.asarray(xyz).astype(F64)
    return (amp * np.exp(-(x * x).sum(-1) / (2.0 * width * width))).astype(F32)


def cascade_extent(c, scale, G):
    """(s, half_grid) of cascade c as the float32 values the kernels receive."""
    s = min(2.0**(c - 1), float(scale))
    return F32(s), F32(s / G)


def update(grid, G, scale, cap, decay, warmup, jitter, density, uniforms=None, det=False, dtype=F32):
    """One occupancy update over all cascades.  grid [C, G^3] float32; jitter[c] [n, 3] uniforms (warm-up: row i = Morton code i);
    uniforms[c] = (u_cell [M], u_pick [M]); density: per cascade an array [n] of float32 densities in draw order, or a callable
    (c, positions [n, 3], indices or None) -> [n].  dtype chooses the float32 restatement or the float64 contract for the
    positions and for the threshold; the merge is float32 in both (it is exact per cell).  Returns a dict:
    xyz[c], indices[c] (None in the warm-up), sigma[c] (the densities, in draw order), tmp[c] (exact array: warm-up and det) or cand[c] (Candidates: plain sampled scatter),
    and, when every tmp is exact: grid, sum64, count, thr, bits."""
    grid = f32(grid)
    C, G3 = grid.shape[0], G**3
    M = G3 // 4
    out = dict(xyz=[], indices=[], sigma=[], tmp=[], cand=[])
    for c in range(C):
        s, hg = cascade_extent(c, scale, G)
        if warmup:
            idx, xyz = None, all_cells(jitter[c], G, s, hg, dtype)
        else:
            lst, cnt = compact(grid[c], cap)
            idx, xyz = sample(uniforms[c][0], uniforms[c][1], jitter[c], lst, cnt, M, G, s, hg, dtype)
        sig = f32(density(c, xyz, idx) if callable(density) else density[c])
        zero = np.zeros(G3, F32)
        if warmup:
            tmp = zero.copy()
            tmp[:] = sig
            cand = None
        elif det:
            tmp, cand = scatter_max(idx, sig, zero), None
        else:
            cand = scatter(idx, sig, zero)
            pairs = np.unique((idx.astype(np.uint64) << np.uint64(32)) | bits32(sig).astype(np.uint64))
            tmp = None
            if pairs.size == np.unique(idx).size:                                 # every drawn cell has one candidate: exact
                tmp = zero.copy()
                tmp[idx] = sig
        out["xyz"].append(xyz); out["indices"].append(idx); out["sigma"].append(sig); out["tmp"].append(tmp); out["cand"].append(cand)
    if all(t is not None for t in out["tmp"]):
        finish(out, grid, np.stack(out["tmp"]), cap, decay, dtype)
    return out


def finish(out, grid, tmp, cap, decay, dtype=F32):
    """merge + threshold + pack of a whole update from an exact tmp."""
    after, s64, cnt = merge(grid.reshape(-1), tmp.reshape(-1), decay)
    if dtype == F32:
        thr = threshold32(*merge_sum32(after), cap)
    else:
        thr = threshold64(s64, cnt, cap)
    out.update(grid=after.reshape(grid.shape), sum64=s64, count=cnt, thr=thr, bits=pack(after, thr))
    return out
