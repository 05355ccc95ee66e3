// hash_grad_input.hip -- gradient of the multiresolution hash-grid encoding with respect to the sample POSITION, for gfx950.
//
// The forward (hash_grid.hip: ngp_hash_fwd_f32 / ngp_hash_fwd_bf16_ex / ngp_hash_fwd_f16) evaluates, on level l with
// pos_k = x_k * scale_l + 0.5 and (cell, fr) = cell_frac<HALF_CELL>(x, scale_l),
//     enc[l,f] = sum_c w_c(fr) * T[off_l + idx_c, f],      w_c = prod_j (fr_j on the far side of corner c along j, else 1 - fr_j).
// This file computes, for the gradient denc of a loss with respect to enc,
//     dx_k = sum_l scale_l * sum_f denc[l,f] * sum_c s_k(c) * prod_{j != k} w_j(c) * T[off_l + idx_c, f],     s_k(c) = +1 far / -1 near,
// i.e. the derivative of the function AS THE FORWARD EVALUATES IT: the forward's f32 cell and fraction (the f16-rounded cell for the
// half2 encoder), d fr / d pos = 1, and on a cell face (fr == 0) the derivative of the cell floorf selects (the one-sided derivative
// towards larger coordinates).  Positions outside [0, 1] and NaN positions take the cell the forward's f2u_sat gives them;
// level_index stays below the level's entry count for any input, so no read leaves the table (a NaN position yields a NaN row).
// Cells, fractions and entry indices come from hash_common.h, so they are the forward's bit for bit.
//
// Mapping: one lane per (sample, level), level fastest -- the generic forward gather's mapping -- with a sample's levels padded to
// the next power of two G <= 16, so that a sample's lanes never straddle a wave.  A lane gathers its eight corners (8 x F values,
// all in flight together), reads its F gradient values from the natural [n, L*F] row (consecutive lanes, consecutive addresses),
// and forms t_c = sum_f denc_f * T_c,f.  Per axis the signed corner sum is taken as four weighted DIFFERENCES,
//     sum_{a,b} w_j(a) * w_m(b) * (t[far along k, a, b] - t[near along k, a, b]),
// so a table that is constant over the cell gives exactly 0.  The G lanes of a sample are then summed with a fixed xor-shuffle tree
// (log2 G steps): no atomics, the same bits on every run.  Lane 0 of the group writes the row: dx is WRITTEN, never accumulated.
// All products and sums are f32.  F = 2, L = 16: 16 x (8 x 8 B gathered + 8 B of denc) + 12 B position + 12 B dx = 1176 B per sample
// (bf16 / f16 table: 4-byte gathers, 664 / 600 B).
#include "ngp_device.h"
#include "hash_common.h"
#include "hash_lanes.h"
#include <hip/hip_fp16.h>

namespace ngp {

enum { TABLE_F32 = 0, TABLE_BF16 = 1, TABLE_F16 = 2 };

// KIND TABLE_F32: f32 table [entries, F], f32 denc.  TABLE_BF16: bf16 pairs (F = 2), f32 denc.  TABLE_F16: the half2 encoder -- f16
// pairs (F = 2), f16 denc, the cell rounded to f16 before the subtract (HALF_CELL).
template <int F, int KIND>
__global__ void __launch_bounds__(256) hash_bwd_input_kernel(const float* __restrict__ xyzs, const void* __restrict__ table_v,
                                                             const void* __restrict__ denc_v, ngp_hash_levels lv, int n, int group,
                                                             float* __restrict__ dxyzs) {
    static_assert(KIND == TABLE_F32 || F == 2, "the 16-bit tables pack feature pairs");
    __shared__ LevelLDS L;
    load_levels(lv, L);
    const int nl = lv.n_levels;
    const long long total = (long long)n * group;
    // the loop bound is the same for every lane of a block (the shuffles below need whole groups; a group's lanes share `i`)
    for (long long base = (long long)blockIdx.x * blockDim.x; base < total; base += (long long)gridDim.x * blockDim.x) {
        const long long gid = base + threadIdx.x;
        const long long i = gid / group;
        const int level = (int)(gid - i * group);
        float d[3] = {0.0f, 0.0f, 0.0f};
        if (gid < total && level < nl) {
            const float x[3] = {xyzs[3 * (size_t)i], xyzs[3 * (size_t)i + 1], xyzs[3 * (size_t)i + 2]};
            const LevelView l = level_at(L, lv, level);
            uint32_t cell[3];
            float fr[3];
            cell_frac<KIND == TABLE_F16>(x, l.scale, cell, fr);
            float g[F];
            const size_t row = ((size_t)i * nl + level) * F;
            if constexpr (KIND == TABLE_F16) {
                const float2 gh = __half22float2(*reinterpret_cast<const __half2*>(reinterpret_cast<const __half*>(denc_v) + row));
                g[0] = gh.x; g[1] = gh.y;
            } else {
                // = load_row<F>(gp, g), spelled out: through the call F = 8 goes from 92 to 106 VGPRs and loses a wave per SIMD
                const float* gp = reinterpret_cast<const float*>(denc_v) + row;
                if constexpr (F == 2) { const float2 t = *reinterpret_cast<const float2*>(gp); g[0] = t.x; g[1] = t.y; }
                else if constexpr (F == 4) { const float4 t = *reinterpret_cast<const float4*>(gp); g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w; }
                else {
#pragma unroll
                    for (int f = 0; f < F; ++f) g[f] = gp[f];
                }
            }
            float v[8][F];
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) {
                const size_t e = (size_t)l.offset + level_index(l.dense, l.mode, l.size, l.res, cell[0] + (ci & 1), cell[1] + ((ci >> 1) & 1), cell[2] + (ci >> 2));
                if constexpr (KIND == TABLE_BF16) {
                    const float2 t = bf16x2_to_f32(reinterpret_cast<const uint32_t*>(table_v)[e]);
                    v[ci][0] = t.x; v[ci][1] = t.y;
                } else if constexpr (KIND == TABLE_F16) {
                    const float2 t = __half22float2(reinterpret_cast<const __half2*>(table_v)[e]);
                    v[ci][0] = t.x; v[ci][1] = t.y;
                } else {
                    const float* p = reinterpret_cast<const float*>(table_v) + e * F;
                    load_row<F>(p, v[ci]);
                }
            }
            float t[8];                                        // t_c = sum_f denc_f * T_c,f
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) {
                float s = g[0] * v[ci][0];
#pragma unroll
                for (int f = 1; f < F; ++f) s += g[f] * v[ci][f];
                t[ci] = s;
            }
            const float w[3][2] = {{1.0f - fr[0], fr[0]}, {1.0f - fr[1], fr[1]}, {1.0f - fr[2], fr[2]}};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int j = (k + 1) % 3, m = (k + 2) % 3;    // the two other axes
                float s = 0.0f;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int near = (a << j) | (b << m);  // corner with bit k clear
                        s += (w[j][a] * w[m][b]) * (t[near | (1 << k)] - t[near]);
                    }
                d[k] = l.scale * s;
            }
        }
        group_tree_sum3(d, group);
        if (gid < total && level == 0) {
            float* o = dxyzs + 3 * (size_t)i;
            o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
        }
    }
}

template <int F, int KIND>
static int launch_bwd_input(const float* xyzs, const void* table, const void* denc, const ngp_hash_levels* lv, int n, float* dxyzs, void* stream) {
    const SampleLevelGrid g = sample_level_grid(lv, n);
    hipLaunchKernelGGL((hash_bwd_input_kernel<F, KIND>), dim3(g.blocks), dim3(256), 0, (hipStream_t)stream, xyzs, table, denc, *lv, n,
                       g.group, dxyzs);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_hash_bwd_input_f32(const float* xyzs, const float* table, const float* denc, const ngp_hash_levels* lv, int n, float* dxyzs,
                           void* stream) {
    if (n <= 0) return 0;
    if (lv->n_levels < 1 || lv->n_levels > NGP_MAX_LEVELS) return -1;
    switch (lv->n_features) {
        case 1: return launch_bwd_input<1, TABLE_F32>(xyzs, table, denc, lv, n, dxyzs, stream);
        case 2: return launch_bwd_input<2, TABLE_F32>(xyzs, table, denc, lv, n, dxyzs, stream);
        case 4: return launch_bwd_input<4, TABLE_F32>(xyzs, table, denc, lv, n, dxyzs, stream);
        case 8: return launch_bwd_input<8, TABLE_F32>(xyzs, table, denc, lv, n, dxyzs, stream);
        default: return -1;
    }
}

int ngp_hash_bwd_input_bf16(const float* xyzs, const uint16_t* table, const float* denc, const ngp_hash_levels* lv, int n, float* dxyzs,
                            void* stream) {
    if (n <= 0) return 0;
    if (lv->n_levels < 1 || lv->n_levels > NGP_MAX_LEVELS || lv->n_features != 2) return -1;
    return launch_bwd_input<2, TABLE_BF16>(xyzs, table, denc, lv, n, dxyzs, stream);
}

int ngp_hash_bwd_input_f16(const float* xyzs, const uint16_t* table, const uint16_t* denc, const ngp_hash_levels* lv, int n, float* dxyzs,
                           void* stream) {
    if (n <= 0) return 0;
    if (lv->n_levels < 1 || lv->n_levels > NGP_MAX_LEVELS || lv->n_features != 2) return -1;
    return launch_bwd_input<2, TABLE_F16>(xyzs, table, denc, lv, n, dxyzs, stream);
}

}  // extern "C"
