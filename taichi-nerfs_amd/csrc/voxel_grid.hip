// voxel_grid.hip -- the explicit voxel-grid radiance field (model_name='svox') for gfx950.
//
// Replaces VoxelGrid.forward of the reference's modules/networks.py (:566-575, which cannot run upstream) with the lookup its
// helpers describe: normalize_samples (:521-522), query_grids(use_trilinear=False) (:546-559), out_of_grid (:491-508) and
// sh_utils.eval_sh (:58-113), plus the PlenOctrees activations (sigma = relu(density), rgb = sigmoid(SH)).  DESIGN.md, voxel grid.
//
// Layout: sh = [G, G, G, 3*D] f32 (D = (deg+1)^2, channel-major: R's D coefficients, then G's, then B's), density = [G, G, G] f32,
// index order (x, y, z) 'ij'.  Sample p selects row ((ix * G + iy) * G + iz) with i = rint((p - m) / r) per axis (IEEE divide,
// half-to-even like torch.round); any axis outside [0, G) gives an all-zero row.
// Kernels:
//   voxel_fwd_kernel      one lane per sample: 3*D + 1 gathers of one row, SH basis, relu / sigmoid
//   voxel_density_kernel  one lane per sample: the density only (occupancy update)
//   voxel_bwd_kernel      one wave per 64 consecutive samples.  Every lane writes its W = 3*D + 1 row contributions to the wave's LDS
//                         tile; the row index is recomputed from the position.  Consecutive samples of a ray mostly share a voxel, so
//                         the wave's runs of equal rows are summed before any atomic: lane (slot, channel) adds channel `channel` of
//                         one run over the run's tile rows and issues ONE float atomic for it.  An atomic instruction thus covers
//                         64 / W whole row segments (contiguous addresses), not 64 scattered rows.
//   voxel_tri_fwd_kernel      trilinear: one lane per sample; per corner the density and the three SH dot products (8 row gathers),
//                             then nested lerps a + t (b - a) in z, y, x order.  A group of 8 lanes per sample (a corner each,
//                             exchange-and-lerp by shuffles) measured slower at every degree above 0 (voxel grid)
//   voxel_tri_density_kernel  trilinear density only, one lane per sample: eight 4-byte gathers, the same lerps
//   voxel_tri_bwd_kernel      trilinear backward, one wave per 64 consecutive samples like voxel_bwd_kernel, with the 8 corner weights
//                             beside each lane's row vector in LDS; runs of equal base CELL are summed per (corner, channel) before
//                             any atomic, and the adds of a z-pair of corners form one contiguous 2 x 12 D-byte segment of dsh
//   voxel_occ_*           packbits for the occupancy grid with the mean accumulated in f64 and `>=` (the fresh-field trap)
// Shared by the nearest and the trilinear form, each stated once:
//   vox_row_values        a row's forward value: the raw density and the three dot products sum_k Y[k] sh[c * D + k] (nearest: its one
//                         row; trilinear: each of the eight corners); vox_relu / vox_sigmoid are the two activations
//   vox_trilerp           the lerp tree z, then y, then x over eight corner values (trilinear forward per channel, trilinear density)
//   vox_grad_row          the backward preamble: the sample's four gradients, the all-zero skip, lane's tile row g[c] * Y[k] | gs
//   vox_find_runs         runs of equal keys (row or base cell) among a wave's 64 lanes as two ballots, `starts` (every run) and `heads`
//                         (runs of a key >= 0), then the wave-level ordering of the tile writes before the merge reads them
//   vox_take_heads / vox_run_end   the merge loop's "next PER heads, one per slot" and "[h, next boundary)"
//   vox_cell_key / vox_key_cell    the trilinear run key of base cell b in [-1, G)^3 and its inverse
//   vox_launch / vox_for_degree    the host entries' prologue (n, grid parameters, launch check) and the degree dispatch of the four
//                                  templated kernels; each nearest / trilinear entry pair is one function that picks the kernel
#include <type_traits>
#include "ngp_device.h"

namespace ngp {

constexpr int VOX_BWD_WAVES = 4;
constexpr int VOX_OCC_BLOCKS = 256;

struct VoxParams {
    int G;
    float m, r;           // grid minimum and spacing: i = (p - m) / r
};

// row of p, or -1 when any axis falls outside [0, G) (NaN included)
__device__ __forceinline__ long long vox_row(const VoxParams& vp, const float* __restrict__ xyzs, long i) {
    long long row = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = rintf((xyzs[i * 3 + k] - vp.m) / vp.r);
        if (!(f >= 0.0f && f < (float)vp.G)) return -1;
        row = row * vp.G + (long long)f;
    }
    return row;
}

// eval_sh's basis (sh_utils.py:58-113) at the normalised direction: result = sum_k Y[k] * sh[k]
template <int DEG>
__device__ __forceinline__ void sh_basis(const float* __restrict__ dirs, long i, float Y[(DEG + 1) * (DEG + 1)]) {
    const float dx = dirs[i * 3 + 0], dy = dirs[i * 3 + 1], dz = dirs[i * 3 + 2];
    const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float x = dx / nrm, y = dy / nrm, z = dz / nrm;
    Y[0] = 0.28209479177387814f;
    if (DEG > 0) {
        const float C1 = 0.4886025119029199f;
        Y[1] = -C1 * y; Y[2] = C1 * z; Y[3] = -C1 * x;
    }
    if (DEG > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        Y[4] = 1.0925484305920792f * xy;
        Y[5] = -1.0925484305920792f * yz;
        Y[6] = 0.31539156525252005f * (2.0f * zz - xx - yy);
        Y[7] = -1.0925484305920792f * xz;
        Y[8] = 0.5462742152960396f * (xx - yy);
        if (DEG > 2) {
            Y[9] = -0.5900435899266435f * y * (3.0f * xx - yy);
            Y[10] = 2.890611442640554f * xy * z;
            Y[11] = -0.4570457994644658f * y * (4.0f * zz - xx - yy);
            Y[12] = 0.3731763325901154f * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
            Y[13] = -0.4570457994644658f * x * (4.0f * zz - xx - yy);
            Y[14] = 1.445305721320277f * z * (xx - yy);
            Y[15] = -0.5900435899266435f * x * (xx - 3.0f * yy);
        }
        if (DEG > 3) {
            Y[16] = 2.5033429417967046f * xy * (xx - yy);
            Y[17] = -1.7701307697799304f * yz * (3.0f * xx - yy);
            Y[18] = 0.9461746957575601f * xy * (7.0f * zz - 1.0f);
            Y[19] = -0.6690465435572892f * yz * (7.0f * zz - 3.0f);
            Y[20] = 0.10578554691520431f * (zz * (35.0f * zz - 30.0f) + 3.0f);
            Y[21] = -0.6690465435572892f * xz * (7.0f * zz - 3.0f);
            Y[22] = 0.47308734787878004f * (xx - yy) * (7.0f * zz - 1.0f);
            Y[23] = -1.7701307697799304f * xz * (xx - 3.0f * yy);
            Y[24] = 0.6258357354491761f * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy));
        }
    }
}

__device__ __forceinline__ float vox_relu(float v) { return v > 0.0f ? v : 0.0f; }
__device__ __forceinline__ float vox_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// out[0] = the raw density of `row`, out[1 + c] = sum_k Y[k] * sh[row][c * D + k] in index order; all zero for row < 0
template <int DEG>
__device__ __forceinline__ void vox_row_values(long long row, const float* Y, const float* density, const float* sh, float out[4]) {
    constexpr int D = (DEG + 1) * (DEG + 1);
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    if (row < 0) return;
    out[0] = density[row];
    const float* s = sh + (size_t)row * (3 * D);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < D; ++k) out[1 + c] += Y[k] * s[c * D + k];
}

template <int DEG>
__global__ void __launch_bounds__(256) voxel_fwd_kernel(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                        const float* __restrict__ sh, const float* __restrict__ density, int n,
                                                        VoxParams vp, float* __restrict__ sigmas, float* __restrict__ rgbs) {
    constexpr int D = (DEG + 1) * (DEG + 1);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long row = vox_row(vp, xyzs, i);
    float Y[D], v[4];
    sh_basis<DEG>(dirs, i, Y);
    vox_row_values<DEG>(row, Y, density, sh, v);
    sigmas[i] = vox_relu(v[0]);
#pragma unroll
    for (int c = 0; c < 3; ++c) rgbs[i * 3 + c] = vox_sigmoid(v[1 + c]);
}

__global__ void __launch_bounds__(256) voxel_density_kernel(const float* __restrict__ xyzs, const float* __restrict__ density, int n,
                                                            VoxParams vp, float* __restrict__ sigmas) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long row = vox_row(vp, xyzs, i);
    sigmas[i] = vox_relu(row >= 0 ? density[row] : 0.0f);
}

// ---------------------------------------------------------------------------------------------------- backward, both forms
// d sigma / d density = [density > 0] (= [sigma > 0]); d rgb_c / d sh_{c,k} = rgb_c (1 - rgb_c) Y_k.  Writes sample i's row of the
// wave's tile (column c*D + k the SH contribution, column 3*D the density one) unless all four gradients are zero: false then, the
// sample contributes nothing.
template <int DEG>
__device__ __forceinline__ bool vox_grad_row(const float* __restrict__ dirs, const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                             const float* __restrict__ dsigmas, const float* __restrict__ drgbs, long i, float* trow) {
    constexpr int D = (DEG + 1) * (DEG + 1);
    const float gs = sigmas[i] > 0.0f ? dsigmas[i] : 0.0f;
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float o = rgbs[i * 3 + c];
        g[c] = drgbs[i * 3 + c] * (o * (1.0f - o));
    }
    if (gs == 0.0f && g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f) return false;
    float Y[D];
    sh_basis<DEG>(dirs, i, Y);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < D; ++k) trow[c * D + k] = g[c] * Y[k];
    trow[3 * D] = gs;
    return true;
}

// Runs of equal keys among the wave's lanes: a boundary wherever the key changes.  `starts` has every run's first lane, `heads` those
// of the runs to flush (key >= 0).  Ends with the ordering of the lanes' tile writes before the merge loops read other lanes' rows.
struct VoxRuns {
    unsigned long long starts, heads;
};
__device__ __forceinline__ VoxRuns vox_find_runs(long long key, int lane) {
    const long long prev = __shfl_up(key, 1);
    const bool boundary = lane == 0 || prev != key;
    const VoxRuns r = {__ballot(boundary), __ballot(boundary && key >= 0)};
    wave_sync_lds();
    return r;
}

// the next PER run heads of `heads` (removed from it): slot s gets the s-th, -1 when there is none
template <int PER>
__device__ __forceinline__ int vox_take_heads(unsigned long long& heads, int slot) {
    unsigned long long rest = heads;
    int h = -1;
#pragma unroll
    for (int s = 0; s < PER; ++s) {
        const int hs = rest ? __ffsll((long long)rest) - 1 : -1;
        if (s == slot) h = hs;
        if (rest) rest &= rest - 1ull;
    }
    heads = rest;
    return h;
}

// the run that starts at lane h is [h, next boundary)
__device__ __forceinline__ int vox_run_end(unsigned long long starts, int h) {
    const unsigned long long after = h == 63 ? 0ull : (starts >> (h + 1)) << (h + 1);
    return after ? __ffsll((long long)after) - 1 : NGP_WAVE;
}

// One wave per 64 consecutive samples; runs of equal ROW are summed per channel before any atomic (header).
template <int DEG>
__global__ void __launch_bounds__(64 * VOX_BWD_WAVES) voxel_bwd_kernel(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                                      const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                                                      const float* __restrict__ dsigmas, const float* __restrict__ drgbs,
                                                                      int n, VoxParams vp, float* __restrict__ dsh,
                                                                      float* __restrict__ ddensity) {
    constexpr int D = (DEG + 1) * (DEG + 1), W = 3 * D + 1;
    constexpr int PER = W < NGP_WAVE ? NGP_WAVE / W : 1;              // runs per atomic instruction
    __shared__ float tile[VOX_BWD_WAVES][NGP_WAVE][W];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & (NGP_WAVE - 1);
    float (*T)[W] = tile[wv];
    const long i = ((long)blockIdx.x * VOX_BWD_WAVES + wv) * NGP_WAVE + lane;
    long long row = -1;
    if (i < n) {
        row = vox_row(vp, xyzs, i);
        if (row >= 0 && !vox_grad_row<DEG>(dirs, sigmas, rgbs, dsigmas, drgbs, i, T[lane])) row = -1;
    }
    const VoxRuns runs = vox_find_runs(row, lane);
    const int slot = lane / W, ch = lane % W;                         // (%: ch < W is then known and the column loop folds for W < 64)
    unsigned long long hd = runs.heads;
    while (hd) {
        const int h = vox_take_heads<PER>(hd, slot);
        const long long hrow = __shfl(row, h < 0 ? 0 : h);           // every lane takes part in the shuffle
        if (h < 0) continue;                                         // also the lanes past the last whole row: slot >= PER
        const int end = vox_run_end(runs.starts, h);
        for (int c0 = ch; c0 < W; c0 += (W < NGP_WAVE ? W : NGP_WAVE)) {
            float v = 0.0f;
            for (int s = h; s < end; ++s) v += T[s][c0];
            if (v != 0.0f) {
                if (c0 < 3 * D) unsafeAtomicAdd(dsh + (size_t)hrow * (3 * D) + c0, v);
                else unsafeAtomicAdd(ddensity + hrow, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- trilinear lookup
// Base cell b = floor(u) and fraction f = u - b of u = (p - m) / r per axis; false (and f = 0) when any u is outside [-1, G) or NaN:
// no corner of such a sample is a grid point.  The range test is in float, before the integer conversion.
__device__ __forceinline__ bool vox_cell(const VoxParams& vp, const float* __restrict__ xyzs, long i, int b[3], float f[3]) {
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = (xyzs[i * 3 + k] - vp.m) / vp.r;
        const bool ok = u >= -1.0f && u < (float)vp.G;
        const float fl = ok ? floorf(u) : 0.0f;
        b[k] = (int)fl;
        f[k] = ok ? u - fl : 0.0f;
        in = in && ok;
    }
    return in;
}

// row of corner c (bit 2 = x, bit 1 = y, bit 0 = z) of base cell b, or -1 when it is no grid point (out_of_grid, :489-508)
__device__ __forceinline__ long long vox_corner_row(const VoxParams& vp, const int b[3], int c) {
    const int cx = b[0] + (c >> 2), cy = b[1] + ((c >> 1) & 1), cz = b[2] + (c & 1);
    if ((unsigned)cx >= (unsigned)vp.G || (unsigned)cy >= (unsigned)vp.G || (unsigned)cz >= (unsigned)vp.G) return -1;
    return ((long long)cx * vp.G + cy) * vp.G + cz;
}

// trilinear_interpolation's lerp (:524-533).  This form, not (1 - t) a + t b, returns a constant field exactly.
__device__ __forceinline__ float vox_lerp(float a, float b, float t) { return a + t * (b - a); }

// the nested lerps over the eight corner values: along z, then y, then x
__device__ __forceinline__ float vox_trilerp(const float v[8], const float f[3]) {
    float z[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) z[p] = vox_lerp(v[2 * p], v[2 * p + 1], f[2]);
    return vox_lerp(vox_lerp(z[0], z[1], f[1]), vox_lerp(z[2], z[3], f[1]), f[0]);
}

// the trilinear backward's run key of base cell b, every axis in [-1, G): ((bx + 1) (G + 1) + by + 1) (G + 1) + bz + 1, and back
__device__ __forceinline__ long long vox_cell_key(const VoxParams& vp, const int b[3]) {
    const int G1 = vp.G + 1;
    return ((long long)(b[0] + 1) * G1 + (b[1] + 1)) * G1 + (b[2] + 1);
}
__device__ __forceinline__ void vox_key_cell(const VoxParams& vp, long long key, int b[3]) {
    const int G1 = vp.G + 1;
    b[0] = (int)(key / ((long long)G1 * G1)) - 1;
    b[1] = (int)((key / G1) % G1) - 1;
    b[2] = (int)(key % G1) - 1;
}

// One lane per sample: per corner the density and the three dot products sum_k Y_k sh_{c,k} (eval_sh is linear), then the lerps.
template <int DEG>
__global__ void __launch_bounds__(256) voxel_tri_fwd_kernel(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                                 const float* __restrict__ sh, const float* __restrict__ density, int n,
                                                                 VoxParams vp, float* __restrict__ sigmas, float* __restrict__ rgbs) {
    constexpr int D = (DEG + 1) * (DEG + 1);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int b[3];
    float f[3];
    float v[4][8];                                                       // [density | R, G, B dot product][corner]
    const bool in = vox_cell(vp, xyzs, i, b, f);
    float Y[D];
    sh_basis<DEG>(dirs, i, Y);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float r[4];
        vox_row_values<DEG>(in ? vox_corner_row(vp, b, c) : -1, Y, density, sh, r);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q][c] = r[q];
    }
    sigmas[i] = vox_relu(vox_trilerp(v[0], f));
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgbs[i * 3 + ch] = vox_sigmoid(vox_trilerp(v[1 + ch], f));
}

__global__ void __launch_bounds__(256) voxel_tri_density_kernel(const float* __restrict__ xyzs, const float* __restrict__ density, int n,
                                                                VoxParams vp, float* __restrict__ sigmas) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int b[3];
    float f[3];
    float dv = 0.0f;
    if (vox_cell(vp, xyzs, i, b, f)) {
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const long long row = vox_corner_row(vp, b, c);
            v[c] = row >= 0 ? density[row] : 0.0f;
        }
        dv = vox_trilerp(v, f);
    }
    sigmas[i] = vox_relu(dv);
}

// d out / d row[corner] = w_corner * (d out / d interpolated row), w_corner the product of the per-axis factors (1 - f or f).  Tile
// columns as vox_grad_row writes them; wts[lane][corner] beside them.  A run is a stretch of lanes with the same base cell: all its samples
// add into the same eight rows.  SH: a z-pair of corners (rows r and r + 1) is one segment of SEG = 6 D consecutive floats of dsh; NS
// segments fit one atomic instruction (degree 0: 2 runs x 4 pairs, degree 1: 2 pairs, degree 2: 1; degrees 3, 4: a column loop).
// Density: 8 lanes per run, z on the lowest lane bit, 8 runs per atomic instruction.
template <int DEG>
__global__ void __launch_bounds__(64 * VOX_BWD_WAVES) voxel_tri_bwd_kernel(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                                          const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                                                          const float* __restrict__ dsigmas, const float* __restrict__ drgbs,
                                                                          int n, VoxParams vp, float* __restrict__ dsh,
                                                                          float* __restrict__ ddensity) {
    constexpr int D = (DEG + 1) * (DEG + 1), W = 3 * D + 1, SEG = 6 * D;
    constexpr int LW = SEG < NGP_WAVE ? SEG : NGP_WAVE;                  // lanes per segment
    constexpr int NS = NGP_WAVE / LW;                                    // segments per atomic instruction
    constexpr int PP = NS >= 4 ? 4 : NS;                                 // z-pairs of one run side by side
    constexpr int RP = NS >= 4 ? NS / 4 : 1;                             // runs side by side
    __shared__ float tile[VOX_BWD_WAVES][NGP_WAVE][W];
    __shared__ float wts[VOX_BWD_WAVES][NGP_WAVE][8];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & (NGP_WAVE - 1);
    float (*T)[W] = tile[wv];
    float (*Wt)[8] = wts[wv];
    const long i = ((long)blockIdx.x * VOX_BWD_WAVES + wv) * NGP_WAVE + lane;
    long long cell = -1;                                                 // vox_cell_key of a contributing sample
    if (i < n) {
        int b[3];
        float f[3];
        if (vox_cell(vp, xyzs, i, b, f) && vox_grad_row<DEG>(dirs, sigmas, rgbs, dsigmas, drgbs, i, T[lane])) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                Wt[lane][c] = ((c & 4) ? f[0] : 1.0f - f[0]) * ((c & 2) ? f[1] : 1.0f - f[1]) * ((c & 1) ? f[2] : 1.0f - f[2]);
            cell = vox_cell_key(vp, b);
        }
    }
    const VoxRuns runs = vox_find_runs(cell, lane);
    // ---- SH coefficients
    {
        const int slot = lane / LW, col0 = lane - slot * LW, rslot = slot / PP, pslot = slot - rslot * PP;
        unsigned long long hd = runs.heads;
        while (hd) {
            const int h = vox_take_heads<RP>(hd, rslot);                 // lanes past the last whole segment: rslot >= RP, h = -1
            const long long hcell = __shfl(cell, h < 0 ? 0 : h);         // every lane takes part in the shuffle
            if (h < 0) continue;
            const int end = vox_run_end(runs.starts, h);
            int b[3];
            vox_key_cell(vp, hcell, b);
            for (int p = pslot; p < 4; p += PP)
                for (int col = col0; col < SEG; col += LW) {
                    const int k = col >= 3 * D ? 1 : 0, c0 = col - k * (3 * D), corner = 2 * p + k;
                    const long long row = vox_corner_row(vp, b, corner);
                    if (row < 0) continue;
                    float v = 0.0f;
                    for (int s = h; s < end; ++s) v += Wt[s][corner] * T[s][c0];
                    if (v != 0.0f) unsafeAtomicAdd(dsh + (size_t)row * (3 * D) + c0, v);
                }
        }
    }
    // ---- density
    {
        const int rslot = lane >> 3, corner = lane & 7;
        unsigned long long hd = runs.heads;
        while (hd) {
            const int h = vox_take_heads<8>(hd, rslot);
            const long long hcell = __shfl(cell, h < 0 ? 0 : h);
            if (h < 0) continue;
            const int end = vox_run_end(runs.starts, h);
            int b[3];
            vox_key_cell(vp, hcell, b);
            const long long row = vox_corner_row(vp, b, corner);
            if (row < 0) continue;
            float v = 0.0f;
            for (int s = h; s < end; ++s) v += Wt[s][corner] * T[s][3 * D];
            if (v != 0.0f) unsafeAtomicAdd(ddensity + row, v);
        }
    }
}

// occupancy packbits: f64 sum / count of the positive cells, per block in grid-stride order, then summed in one fixed order by every
// block of the pack kernel
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, NGP_WAVE);
    return v;
}

__device__ __forceinline__ void block_sum2_d(double& s, double& c) {
    __shared__ double ps[4], pc[4];
    s = wave_sum_d(s); c = wave_sum_d(c);
    if ((threadIdx.x & 63) == 0) { ps[threadIdx.x >> 6] = s; pc[threadIdx.x >> 6] = c; }
    __syncthreads();
    s = (ps[0] + ps[1]) + (ps[2] + ps[3]);
    c = (pc[0] + pc[1]) + (pc[2] + pc[3]);
}

__global__ void __launch_bounds__(256) voxel_occ_stats_kernel(const float* __restrict__ grid, long long n, double* __restrict__ partials) {
    double s = 0.0, c = 0.0;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
        const float g = grid[k];
        if (g > 0.0f) { s += (double)g; c += 1.0; }
    }
    block_sum2_d(s, c);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = s; partials[2 * blockIdx.x + 1] = c; }
}

__global__ void __launch_bounds__(256) voxel_occ_pack_kernel(const float* __restrict__ grid, long long n_bytes, const double* __restrict__ partials,
                                                             double thr_max, uint8_t* __restrict__ out) {
    double s = 0.0, c = 0.0;
    for (int b = threadIdx.x; b < VOX_OCC_BLOCKS; b += 256) { s += partials[2 * b]; c += partials[2 * b + 1]; }
    block_sum2_d(s, c);
    // no positive cell: nothing is occupied (NGP's `>` against a NaN mean marks nothing either)
    const float thr = c > 0.0 ? (float)fmin(s / c, thr_max) : INFINITY;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n_bytes; k += (long long)gridDim.x * blockDim.x) {
        const float4 a = reinterpret_cast<const float4*>(grid)[2 * k], b = reinterpret_cast<const float4*>(grid)[2 * k + 1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t bits = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) bits |= (v[j] > 0.0f && v[j] >= thr) ? (1u << j) : 0u;
        out[k] = (uint8_t)bits;
    }
}

// ---------------------------------------------------------------------------------------------------- host entries
// The prologue and epilogue of every per-sample entry: nothing to do for n <= 0, -1 for bad grid parameters or when `launch` (which
// gets the VoxParams and returns whether it launched) refuses, the launch's error otherwise.
template <class Launch>
static int vox_launch(int n, int grid_size, float grid_min, float grid_radius, Launch&& launch) {
    if (n <= 0) return 0;
    if (grid_size < 1 || grid_size > 1024 || !(grid_radius > 0.0f)) return -1;
    if (!launch(VoxParams{grid_size, grid_min, grid_radius})) return -1;
    NGP_LAUNCH_CHECK();
    return 0;
}

// f(std::integral_constant<int, DEG>) for the sh_degree the kernels are instantiated for; false for any other
template <class F>
static bool vox_for_degree(int sh_degree, F&& f) {
    switch (sh_degree) {
        case 0: f(std::integral_constant<int, 0>()); return true;
        case 1: f(std::integral_constant<int, 1>()); return true;
        case 2: f(std::integral_constant<int, 2>()); return true;
        case 3: f(std::integral_constant<int, 3>()); return true;
        case 4: f(std::integral_constant<int, 4>()); return true;
        default: return false;
    }
}

static int vox_fwd(bool trilinear, const float* xyzs, const float* dirs, const float* sh, const float* density, int n, int grid_size,
                   int sh_degree, float grid_min, float grid_radius, float* sigmas, float* rgbs, void* stream) {
    return vox_launch(n, grid_size, grid_min, grid_radius, [&](const VoxParams& vp) {
        return vox_for_degree(sh_degree, [&](auto deg) {
            constexpr int DEG = decltype(deg)::value;
            hipLaunchKernelGGL(trilinear ? voxel_tri_fwd_kernel<DEG> : voxel_fwd_kernel<DEG>, dim3((n + 255) / 256), dim3(256), 0,
                               (hipStream_t)stream, xyzs, dirs, sh, density, n, vp, sigmas, rgbs);
        });
    });
}

static int vox_density(bool trilinear, const float* xyzs, const float* density, int n, int grid_size, float grid_min, float grid_radius,
                       float* sigmas, void* stream) {
    return vox_launch(n, grid_size, grid_min, grid_radius, [&](const VoxParams& vp) {
        hipLaunchKernelGGL(trilinear ? voxel_tri_density_kernel : voxel_density_kernel, dim3((n + 255) / 256), dim3(256), 0,
                           (hipStream_t)stream, xyzs, density, n, vp, sigmas);
        return true;
    });
}

static int vox_bwd(bool trilinear, const float* xyzs, const float* dirs, const float* sigmas, const float* rgbs, const float* dsigmas,
                   const float* drgbs, int n, int grid_size, int sh_degree, float grid_min, float grid_radius, float* dsh, float* ddensity,
                   void* stream) {
    return vox_launch(n, grid_size, grid_min, grid_radius, [&](const VoxParams& vp) {
        return vox_for_degree(sh_degree, [&](auto deg) {
            constexpr int DEG = decltype(deg)::value, per_block = 64 * VOX_BWD_WAVES;
            hipLaunchKernelGGL(trilinear ? voxel_tri_bwd_kernel<DEG> : voxel_bwd_kernel<DEG>, dim3((n + per_block - 1) / per_block),
                               dim3(per_block), 0, (hipStream_t)stream, xyzs, dirs, sigmas, rgbs, dsigmas, drgbs, n, vp, dsh, ddensity);
        });
    });
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_voxel_fwd(const float* xyzs, const float* dirs, const float* sh, const float* density, int n, int grid_size, int sh_degree,
                  float grid_min, float grid_radius, float* sigmas, float* rgbs, void* stream) {
    return vox_fwd(false, xyzs, dirs, sh, density, n, grid_size, sh_degree, grid_min, grid_radius, sigmas, rgbs, stream);
}

int ngp_voxel_trilinear_fwd(const float* xyzs, const float* dirs, const float* sh, const float* density, int n, int grid_size,
                            int sh_degree, float grid_min, float grid_radius, float* sigmas, float* rgbs, void* stream) {
    return vox_fwd(true, xyzs, dirs, sh, density, n, grid_size, sh_degree, grid_min, grid_radius, sigmas, rgbs, stream);
}

int ngp_voxel_density(const float* xyzs, const float* density, int n, int grid_size, float grid_min, float grid_radius, float* sigmas,
                      void* stream) {
    return vox_density(false, xyzs, density, n, grid_size, grid_min, grid_radius, sigmas, stream);
}

int ngp_voxel_trilinear_density(const float* xyzs, const float* density, int n, int grid_size, float grid_min, float grid_radius,
                                float* sigmas, void* stream) {
    return vox_density(true, xyzs, density, n, grid_size, grid_min, grid_radius, sigmas, stream);
}

int ngp_voxel_bwd(const float* xyzs, const float* dirs, const float* sigmas, const float* rgbs, const float* dsigmas, const float* drgbs,
                  int n, int grid_size, int sh_degree, float grid_min, float grid_radius, float* dsh, float* ddensity, void* stream) {
    return vox_bwd(false, xyzs, dirs, sigmas, rgbs, dsigmas, drgbs, n, grid_size, sh_degree, grid_min, grid_radius, dsh, ddensity, stream);
}

int ngp_voxel_trilinear_bwd(const float* xyzs, const float* dirs, const float* sigmas, const float* rgbs, const float* dsigmas,
                            const float* drgbs, int n, int grid_size, int sh_degree, float grid_min, float grid_radius, float* dsh,
                            float* ddensity, void* stream) {
    return vox_bwd(true, xyzs, dirs, sigmas, rgbs, dsigmas, drgbs, n, grid_size, sh_degree, grid_min, grid_radius, dsh, ddensity, stream);
}

int ngp_voxel_occ_scratch_doubles(void) { return 2 * VOX_OCC_BLOCKS; }

int ngp_voxel_occ_pack(const float* density_grid, long long n_bytes, double density_threshold, double* scratch, uint8_t* bitfield,
                       void* stream) {
    if (n_bytes <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(voxel_occ_stats_kernel, dim3(VOX_OCC_BLOCKS), dim3(256), 0, st, density_grid, 8 * n_bytes, scratch);
    NGP_LAUNCH_CHECK();
    long long blocks = (n_bytes + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(voxel_occ_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, density_grid, n_bytes, scratch, density_threshold,
                       bitfield);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
