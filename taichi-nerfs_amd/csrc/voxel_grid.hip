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

template <int DEG>
__global__ void __launch_bounds__(256) voxel_fwd_kernel(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                        const float* __restrict__ sh, const float* __restrict__ density, int n,
                                                        VoxParams vp, float* __restrict__ sigmas, float* __restrict__ rgbs) {
    constexpr int D = (DEG + 1) * (DEG + 1);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long row = vox_row(vp, xyzs, i);
    float Y[D];
    sh_basis<DEG>(dirs, i, Y);
    float sigma = 0.0f, acc[3] = {0.0f, 0.0f, 0.0f};
    if (row >= 0) {
        const float dv = density[row];
        sigma = dv > 0.0f ? dv : 0.0f;
        const float* s = sh + (size_t)row * (3 * D);
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < D; ++k) acc[c] += Y[k] * s[c * D + k];
    }
    sigmas[i] = sigma;
#pragma unroll
    for (int c = 0; c < 3; ++c) rgbs[i * 3 + c] = 1.0f / (1.0f + expf(-acc[c]));
}

__global__ void __launch_bounds__(256) voxel_density_kernel(const float* __restrict__ xyzs, const float* __restrict__ density, int n,
                                                            VoxParams vp, float* __restrict__ sigmas) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long row = vox_row(vp, xyzs, i);
    const float dv = row >= 0 ? density[row] : 0.0f;
    sigmas[i] = dv > 0.0f ? dv : 0.0f;
}

// d sigma / d density = [density > 0] (= [sigma > 0]); d rgb_c / d sh_{c,k} = rgb_c (1 - rgb_c) Y_k.  Tile column c*D + k holds the
// SH contribution, column 3*D the density one.
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
        if (row >= 0) {
            const float gs = sigmas[i] > 0.0f ? dsigmas[i] : 0.0f;
            float g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float o = rgbs[i * 3 + c];
                g[c] = drgbs[i * 3 + c] * (o * (1.0f - o));
            }
            if (gs == 0.0f && g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f) {
                row = -1;                                                  // contributes nothing
            } else {
                float Y[D];
                sh_basis<DEG>(dirs, i, Y);
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < D; ++k) T[lane][c * D + k] = g[c] * Y[k];
                T[lane][3 * D] = gs;
            }
        }
    }
    // runs of equal rows: a boundary wherever the row changes; only runs of a valid row are flushed
    const long long prev = __shfl_up(row, 1);
    const bool boundary = lane == 0 || prev != row;
    const unsigned long long starts = __ballot(boundary);
    unsigned long long heads = __ballot(boundary && row >= 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int slot = lane / W, ch = lane - slot * W;
    while (heads) {
        // the next PER runs: slot s takes the s-th remaining head
        unsigned long long rest = heads;
        int h = -1;
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int hs = rest ? __ffsll((long long)rest) - 1 : -1;
            if (s == slot) h = hs;
            if (rest) rest &= rest - 1ull;
        }
        heads = rest;
        const long long hrow = __shfl(row, h < 0 ? 0 : h);           // every lane takes part in the shuffle
        if (slot < PER && h >= 0) {
            // the run is [h, next boundary)
            const unsigned long long after = h == 63 ? 0ull : (starts >> (h + 1)) << (h + 1);
            const int end = after ? __ffsll((long long)after) - 1 : NGP_WAVE;
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
    float v[8][4];
    const bool in = vox_cell(vp, xyzs, i, b, f);
    float Y[D];
    sh_basis<DEG>(dirs, i, Y);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const long long row = in ? vox_corner_row(vp, b, c) : -1;
        v[c][0] = v[c][1] = v[c][2] = v[c][3] = 0.0f;
        if (row >= 0) {
            v[c][0] = density[row];
            const float* s = sh + (size_t)row * (3 * D);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int k = 0; k < D; ++k) v[c][1 + ch] += Y[k] * s[ch * D + k];
        }
    }
    float o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float z[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) z[p] = vox_lerp(v[2 * p][q], v[2 * p + 1][q], f[2]);
        o[q] = vox_lerp(vox_lerp(z[0], z[1], f[1]), vox_lerp(z[2], z[3], f[1]), f[0]);
    }
    sigmas[i] = o[0] > 0.0f ? o[0] : 0.0f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgbs[i * 3 + ch] = 1.0f / (1.0f + expf(-o[1 + ch]));
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
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = vox_lerp(v[2 * c], v[2 * c + 1], f[2]);
        v[0] = vox_lerp(v[0], v[1], f[1]);
        v[1] = vox_lerp(v[2], v[3], f[1]);
        dv = vox_lerp(v[0], v[1], f[0]);
    }
    sigmas[i] = dv > 0.0f ? dv : 0.0f;
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

// d out / d row[corner] = w_corner * (d out / d interpolated row), w_corner the product of the per-axis factors (1 - f or f).  Tile
// columns as in voxel_bwd_kernel; wts[lane][corner] beside them.  A run is a stretch of lanes with the same base cell: all its samples
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
    const int G1 = vp.G + 1;
    long long cell = -1;                                                 // ((bx + 1) (G + 1) + by + 1) (G + 1) + bz + 1, b in [-1, G)
    if (i < n) {
        int b[3];
        float f[3];
        if (vox_cell(vp, xyzs, i, b, f)) {
            const float gs = sigmas[i] > 0.0f ? dsigmas[i] : 0.0f;
            float g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float o = rgbs[i * 3 + c];
                g[c] = drgbs[i * 3 + c] * (o * (1.0f - o));
            }
            if (!(gs == 0.0f && g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f)) {
                float Y[D];
                sh_basis<DEG>(dirs, i, Y);
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < D; ++k) T[lane][c * D + k] = g[c] * Y[k];
                T[lane][3 * D] = gs;
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    Wt[lane][c] = ((c & 4) ? f[0] : 1.0f - f[0]) * ((c & 2) ? f[1] : 1.0f - f[1]) * ((c & 1) ? f[2] : 1.0f - f[2]);
                cell = ((long long)(b[0] + 1) * G1 + (b[1] + 1)) * G1 + (b[2] + 1);
            }
        }
    }
    const long long prev = __shfl_up(cell, 1);
    const bool boundary = lane == 0 || prev != cell;
    const unsigned long long starts = __ballot(boundary);
    const unsigned long long heads = __ballot(boundary && cell >= 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- SH coefficients
    {
        const int slot = lane / LW, col0 = lane - slot * LW, rslot = slot / PP, pslot = slot - rslot * PP;
        unsigned long long hd = heads;
        while (hd) {
            const int h = vox_take_heads<RP>(hd, rslot);                 // lanes past the last whole segment: rslot >= RP, h = -1
            const long long hcell = __shfl(cell, h < 0 ? 0 : h);         // every lane takes part in the shuffle
            if (h < 0) continue;
            const int end = vox_run_end(starts, h);
            const int b[3] = {(int)(hcell / ((long long)G1 * G1)) - 1, (int)((hcell / G1) % G1) - 1, (int)(hcell % G1) - 1};
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
        unsigned long long hd = heads;
        while (hd) {
            const int h = vox_take_heads<8>(hd, rslot);
            const long long hcell = __shfl(cell, h < 0 ? 0 : h);
            if (h < 0) continue;
            const int end = vox_run_end(starts, h);
            const int b[3] = {(int)(hcell / ((long long)G1 * G1)) - 1, (int)((hcell / G1) % G1) - 1, (int)(hcell % G1) - 1};
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

static bool vox_params(int grid_size, float grid_min, float grid_radius, VoxParams& vp) {
    if (grid_size < 1 || grid_size > 1024 || !(grid_radius > 0.0f)) return false;
    vp = VoxParams{grid_size, grid_min, grid_radius};
    return true;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_voxel_fwd(const float* xyzs, const float* dirs, const float* sh, const float* density, int n, int grid_size, int sh_degree,
                  float grid_min, float grid_radius, float* sigmas, float* rgbs, void* stream) {
    if (n <= 0) return 0;
    VoxParams vp;
    if (!vox_params(grid_size, grid_min, grid_radius, vp)) return -1;
    const dim3 grid((n + 255) / 256), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (sh_degree) {
        case 0: hipLaunchKernelGGL(voxel_fwd_kernel<0>, grid, block, 0, st, xyzs, dirs, sh, density, n, vp, sigmas, rgbs); break;
        case 1: hipLaunchKernelGGL(voxel_fwd_kernel<1>, grid, block, 0, st, xyzs, dirs, sh, density, n, vp, sigmas, rgbs); break;
        case 2: hipLaunchKernelGGL(voxel_fwd_kernel<2>, grid, block, 0, st, xyzs, dirs, sh, density, n, vp, sigmas, rgbs); break;
        case 3: hipLaunchKernelGGL(voxel_fwd_kernel<3>, grid, block, 0, st, xyzs, dirs, sh, density, n, vp, sigmas, rgbs); break;
        case 4: hipLaunchKernelGGL(voxel_fwd_kernel<4>, grid, block, 0, st, xyzs, dirs, sh, density, n, vp, sigmas, rgbs); break;
        default: return -1;
    }
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_voxel_density(const float* xyzs, const float* density, int n, int grid_size, float grid_min, float grid_radius, float* sigmas,
                      void* stream) {
    if (n <= 0) return 0;
    VoxParams vp;
    if (!vox_params(grid_size, grid_min, grid_radius, vp)) return -1;
    hipLaunchKernelGGL(voxel_density_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, xyzs, density, n, vp, sigmas);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_voxel_bwd(const float* xyzs, const float* dirs, const float* sigmas, const float* rgbs, const float* dsigmas, const float* drgbs,
                  int n, int grid_size, int sh_degree, float grid_min, float grid_radius, float* dsh, float* ddensity, void* stream) {
    if (n <= 0) return 0;
    VoxParams vp;
    if (!vox_params(grid_size, grid_min, grid_radius, vp)) return -1;
    const int per_block = 64 * VOX_BWD_WAVES;
    const dim3 grid((n + per_block - 1) / per_block), block(per_block);
    hipStream_t st = (hipStream_t)stream;
#define NGP_VOX_BWD(DEG) hipLaunchKernelGGL(voxel_bwd_kernel<DEG>, grid, block, 0, st, xyzs, dirs, sigmas, rgbs, dsigmas, drgbs, n, vp, dsh, \
                                            ddensity)
    switch (sh_degree) {
        case 0: NGP_VOX_BWD(0); break;
        case 1: NGP_VOX_BWD(1); break;
        case 2: NGP_VOX_BWD(2); break;
        case 3: NGP_VOX_BWD(3); break;
        case 4: NGP_VOX_BWD(4); break;
        default: return -1;
    }
#undef NGP_VOX_BWD
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_voxel_trilinear_fwd(const float* xyzs, const float* dirs, const float* sh, const float* density, int n, int grid_size,
                            int sh_degree, float grid_min, float grid_radius, float* sigmas, float* rgbs, void* stream) {
    if (n <= 0) return 0;
    VoxParams vp;
    if (!vox_params(grid_size, grid_min, grid_radius, vp)) return -1;
    const dim3 grid((n + 255) / 256), block(256);
    hipStream_t st = (hipStream_t)stream;
#define NGP_VOX_TRI_FWD(DEG) hipLaunchKernelGGL(voxel_tri_fwd_kernel<DEG>, grid, block, 0, st, xyzs, dirs, sh, density, n, vp, sigmas, rgbs)
    switch (sh_degree) {
        case 0: NGP_VOX_TRI_FWD(0); break;
        case 1: NGP_VOX_TRI_FWD(1); break;
        case 2: NGP_VOX_TRI_FWD(2); break;
        case 3: NGP_VOX_TRI_FWD(3); break;
        case 4: NGP_VOX_TRI_FWD(4); break;
        default: return -1;
    }
#undef NGP_VOX_TRI_FWD
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_voxel_trilinear_density(const float* xyzs, const float* density, int n, int grid_size, float grid_min, float grid_radius,
                                float* sigmas, void* stream) {
    if (n <= 0) return 0;
    VoxParams vp;
    if (!vox_params(grid_size, grid_min, grid_radius, vp)) return -1;
    hipLaunchKernelGGL(voxel_tri_density_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, xyzs, density, n, vp, sigmas);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_voxel_trilinear_bwd(const float* xyzs, const float* dirs, const float* sigmas, const float* rgbs, const float* dsigmas,
                            const float* drgbs, int n, int grid_size, int sh_degree, float grid_min, float grid_radius, float* dsh,
                            float* ddensity, void* stream) {
    if (n <= 0) return 0;
    VoxParams vp;
    if (!vox_params(grid_size, grid_min, grid_radius, vp)) return -1;
    const int per_block = 64 * VOX_BWD_WAVES;
    const dim3 grid((n + per_block - 1) / per_block), block(per_block);
    hipStream_t st = (hipStream_t)stream;
#define NGP_VOX_TRI_BWD(DEG) hipLaunchKernelGGL(voxel_tri_bwd_kernel<DEG>, grid, block, 0, st, xyzs, dirs, sigmas, rgbs, dsigmas, drgbs, n, vp, \
                                                dsh, ddensity)
    switch (sh_degree) {
        case 0: NGP_VOX_TRI_BWD(0); break;
        case 1: NGP_VOX_TRI_BWD(1); break;
        case 2: NGP_VOX_TRI_BWD(2); break;
        case 3: NGP_VOX_TRI_BWD(3); break;
        case 4: NGP_VOX_TRI_BWD(4); break;
        default: return -1;
    }
#undef NGP_VOX_TRI_BWD
    NGP_LAUNCH_CHECK();
    return 0;
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
