// hash_grad_input2.hip -- the DOUBLE backward of the multiresolution hash-grid encoding through its position gradient, for gfx950:
// what a loss on dx (normals, an eikonal term, a gradient penalty) needs to train the table and everything upstream of denc and x.
//
// The first backward (hash_grad_input.hip) evaluates, on level l with (cell, fr) = cell_frac(x, scale_l), w_j(b) = b ? fr_j : 1 - fr_j,
// T_c the F table values of corner c, g = denc[i,l,:] and t_c = g . T_c,
//     dx_k = sum_l scale_l * sum_c s_k(c) * prod_{j != k} w_j(c_j) * t_c,          s_k(c) = +1 far / -1 near.
// With v = ddx[i,:] the gradient of a loss with respect to dx and A_c = sum_k v_k * s_k(c) * prod_{j != k} w_j(c_j), this file computes
//     d_denc[i,l,f]         = scale_l * sum_c A_c * T_c,f                                                    (gather)
//     d_x[i,m]              = sum_l scale_l^2 * sum_{k != m} v_k * M_km                                      (gather)
//     d_table[off_l+idx_c,f] += scale_l * A_c * g_f                                                          (scatter)
// M_km = sum_b w_j(b) * (t[1_k,1_m,b] - t[0_k,1_m,b] - t[1_k,0_m,b] + t[0_k,0_m,b]), j the third axis: M is symmetric and its diagonal
// is exactly 0 (inside a cell the encoding is linear along each axis), so three mixed terms M_xy, M_yz, M_zx are all there is.
// d fr / d pos = 1 and, on a cell face, the cell floorf selects -- the face rule of the first backward.  Cells, fractions and entry
// indices come from hash_common.h: they are the forward's bit for bit, level_index stays below the level's entry count for ANY input
// (NaN and out-of-range positions included), so no access leaves the table; a NaN position gives a NaN row and touches no other row.
//
// Gather (hash_bwd2_gather_kernel): the mapping of hash_bwd_input_kernel -- one lane per (sample, level), level fastest, a sample's
// levels padded to a power of two G <= 16 so its lanes share a wave.  A lane gathers its eight corners (8 x F values, all in flight
// together), reads its F values of denc from the natural [n, L*F] row and the sample's ddx (one 12-byte row per group: a broadcast).
// d_denc is taken per feature in the first backward's difference form, per axis k
//     sum_{a,b} w_j(a) * w_m(b) * (T[far_k,a,b] - T[near_k,a,b]),
// so a table that is constant over the cell gives exactly 0; each lane writes its own F values.  d_x goes through the same fixed
// xor-shuffle tree over the group's lanes and lane 0 writes the row.  Both outputs are WRITTEN, never accumulated; no atomics: the
// same bits on every run.  Either output pointer may be null: its arithmetic and store are skipped.  All arithmetic is f32.
// F = 2, L = 16: 16 x (64 B gathered + 8 B denc + 8 B d_denc) + 12 B position + 12 B ddx + 12 B d_x = 1316 B per sample.
//
// Scatter (hash_bwd2_table_f32x2_kernel, F = 2; hash_bwd2_table_kernel<F> otherwise): the first-order scatter-add of hash_grid.hip with
// scale_l * A_c in place of the trilinear weight -- for F = 2 the same body, scatter_runs_f32x2 (hash_lanes.h).  It does not read the
// table, so one kernel serves the fp32 and the bf16-copy encoder (the gradient goes to the fp32 master).  Float atomics: the summation
// order, and with it the last bits of d_table, is NOT deterministic from run to run, as in the first-order scatter.
#include "ngp_device.h"
#include "hash_common.h"
#include "hash_lanes.h"

namespace ngp {

// BF16: the table is the bf16 storage copy (pairs, F = 2), widened exactly; everything else is the f32 kind.
// The lane mapping, corner gather and difference loop are hash_bwd_input_kernel's, spelled out in both: through shared helpers they
// compile to other schedules, this kernel to a slower one (profiles/hash_lanes_refactor.md).  The rest comes from hash_lanes.h.
template <int F, bool BF16>
__global__ void __launch_bounds__(256) hash_bwd2_gather_kernel(const float* __restrict__ xyzs, const void* __restrict__ table_v,
                                                               const float* __restrict__ denc, const float* __restrict__ ddx,
                                                               ngp_hash_levels lv, int n, int group, float* __restrict__ d_denc,
                                                               float* __restrict__ d_xyzs) {
    static_assert(!BF16 || F == 2, "the bf16 table packs feature pairs");
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
            const float u[3] = {ddx[3 * (size_t)i], ddx[3 * (size_t)i + 1], ddx[3 * (size_t)i + 2]};
            const LevelView l = level_at(L, lv, level);
            uint32_t cell[3];
            float fr[3];
            cell_frac<false>(x, l.scale, cell, fr);
            float g[F];
            const size_t row = ((size_t)i * nl + level) * F;
            load_row<F>(denc + row, g);
            float v[8][F];
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) {
                const size_t e = (size_t)l.offset + level_index(l.dense, l.mode, l.size, l.res, cell[0] + (ci & 1), cell[1] + ((ci >> 1) & 1), cell[2] + (ci >> 2));
                if constexpr (BF16) {
                    const float2 t = bf16x2_to_f32(reinterpret_cast<const uint32_t*>(table_v)[e]);
                    v[ci][0] = t.x; v[ci][1] = t.y;
                } else {
                    const float* p = reinterpret_cast<const float*>(table_v) + e * F;
                    load_row<F>(p, v[ci]);
                }
            }
            const float w[3][2] = {{1.0f - fr[0], fr[0]}, {1.0f - fr[1], fr[1]}, {1.0f - fr[2], fr[2]}};
            if (d_denc) {                                          // d_denc_f = scale * sum_k u_k * (difference form of axis k, feature f)
                float o[F];
#pragma unroll
                for (int f = 0; f < F; ++f) {
                    float acc = 0.0f;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int j = (k + 1) % 3, m = (k + 2) % 3;    // the two other axes
                        float s = 0.0f;
#pragma unroll
                        for (int a = 0; a < 2; ++a)
#pragma unroll
                            for (int b = 0; b < 2; ++b) {
                                const int near = (a << j) | (b << m);  // corner with bit k clear
                                s += (w[j][a] * w[m][b]) * (v[near | (1 << k)][f] - v[near][f]);
                            }
                        acc += u[k] * s;
                    }
                    o[f] = l.scale * acc;
                }
                float* op = d_denc + row;
                store_row<F>(op, o);
            }
            if (d_xyzs) {
                float t[8];                                        // t_c = sum_f denc_f * T_c,f
#pragma unroll
                for (int ci = 0; ci < 8; ++ci) {
                    float s = g[0] * v[ci][0];
#pragma unroll
                    for (int f = 1; f < F; ++f) s += g[f] * v[ci][f];
                    t[ci] = s;
                }
                float M[3];                                        // M[j] = the mixed term of the two axes other than j
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int k = (j + 1) % 3, m = (j + 2) % 3;
                    float s = 0.0f;
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int c0 = b << j;
                        s += w[j][b] * ((t[c0 | (1 << k) | (1 << m)] - t[c0 | (1 << m)]) - (t[c0 | (1 << k)] - t[c0]));
                    }
                    M[j] = s;
                }
                const float s2 = l.scale * l.scale;
                d[0] = s2 * (u[1] * M[2] + u[2] * M[1]);           // M_xy = M[2], M_yz = M[0], M_zx = M[1]
                d[1] = s2 * (u[0] * M[2] + u[2] * M[0]);
                d[2] = s2 * (u[0] * M[1] + u[1] * M[0]);
            }
        }
        if (d_xyzs) {                                              // uniform over the grid: every lane of the wave takes the shuffles
            group_tree_sum3(d, group);
            if (gid < total && level == 0) {
                float* o = d_xyzs + 3 * (size_t)i;
                o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
            }
        }
    }
}

// Generic F: one lane per (sample, level), F*8 independent atomics (the shape of hash_bwd_f32_kernel).
template <int F>
__global__ void __launch_bounds__(256) hash_bwd2_table_kernel(const float* __restrict__ xyzs, const float* __restrict__ denc,
                                                              const float* __restrict__ ddx, ngp_hash_levels lv, int n,
                                                              float* __restrict__ dtable) {
    __shared__ LevelLDS L;
    load_levels(lv, L);
    const int nl = lv.n_levels;
    const long long total = (long long)n * nl;
    for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += (long long)gridDim.x * blockDim.x) {
        const long long i = gid / nl;
        const int level = (int)(gid - i * nl);
        float g[F];
        bool any = false;
#pragma unroll
        for (int f = 0; f < F; ++f) { g[f] = denc[(size_t)gid * F + f]; any |= (g[f] != 0.0f); }
        const float u[3] = {ddx[3 * (size_t)i], ddx[3 * (size_t)i + 1], ddx[3 * (size_t)i + 2]};
        if (!any || (u[0] == 0.0f && u[1] == 0.0f && u[2] == 0.0f)) continue;       // exact-zero rows contribute nothing
        const float x[3] = {xyzs[3 * (size_t)i], xyzs[3 * (size_t)i + 1], xyzs[3 * (size_t)i + 2]};
        const LevelView l = level_at(L, lv, level);
        uint32_t cell[3];
        float fr[3];
        cell_frac<false>(x, l.scale, cell, fr);
        const float w[3][2] = {{1.0f - fr[0], fr[0]}, {1.0f - fr[1], fr[1]}, {1.0f - fr[2], fr[2]}};
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) {
            const int xb = ci & 1, yb = (ci >> 1) & 1, zb = ci >> 2;
            const size_t e = (size_t)l.offset + level_index(l.dense, l.mode, l.size, l.res, cell[0] + xb, cell[1] + yb, cell[2] + zb);
            const float a = l.scale * corner_A(w, u, xb, yb, zb);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const float c = a * g[f];
                if (c != 0.0f) unsafeAtomicAdd(dtable + e * F + f, c);
            }
        }
    }
}

// F = 2: scatter_runs_f32x2 (hash_lanes.h), the body of hash_bwd_f32x2_kernel, with scale_l * A_c in place of the trilinear weight.
struct SecondOrderRows {
    const float *__restrict__ xyzs, *__restrict__ denc, *__restrict__ ddx;
    int nl;
    float u[3];
    __device__ __forceinline__ int count(int n) const { return n; }
    __device__ __forceinline__ void fetch(int i, bool valid, float (&p)[3]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = u[k] = 0.f;
        if (valid) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { p[k] = xyzs[3 * (size_t)i + k]; u[k] = ddx[3 * (size_t)i + k]; }
        }
    }
    __device__ __forceinline__ float grad(int i, int level, int f) const { return denc[(size_t)i * (size_t)(nl * 2) + level * 2 + f]; }
    __device__ __forceinline__ void seen(float) const {}
    __device__ __forceinline__ float weight(const float fr[3], float scale, int xb, int yb, int zb) const {
        const float w[3][2] = {{1.0f - fr[0], fr[0]}, {1.0f - fr[1], fr[1]}, {1.0f - fr[2], fr[2]}};
        return scale * corner_A(w, u, xb, yb, zb);
    }
};
__global__ void __launch_bounds__(256) hash_bwd2_table_f32x2_kernel(const float* __restrict__ xyzs, const float* __restrict__ denc,
                                                                    const float* __restrict__ ddx, ngp_hash_levels lv, int n, float* __restrict__ dtable) {
    scatter_runs_f32x2(lv, n, dtable, blockDim.x, SecondOrderRows{xyzs, denc, ddx, lv.n_levels, {}});
}

template <int F, bool BF16>
static int launch_bwd2_gather(const float* xyzs, const void* table, const float* denc, const float* ddx, const ngp_hash_levels* lv, int n,
                              float* d_denc, float* d_xyzs, void* stream) {
    if (!d_denc && !d_xyzs) return 0;
    const SampleLevelGrid g = sample_level_grid(lv, n);
    hipLaunchKernelGGL((hash_bwd2_gather_kernel<F, BF16>), dim3(g.blocks), dim3(256), 0, (hipStream_t)stream, xyzs, table, denc, ddx,
                       *lv, n, g.group, d_denc, d_xyzs);
    NGP_LAUNCH_CHECK();
    return 0;
}

template <int F>
static int launch_bwd2_table(const float* xyzs, const float* denc, const float* ddx, const ngp_hash_levels* lv, int n, float* dtable,
                             void* stream) {
    const long long lanes = (long long)n * lv->n_levels;
    long long blocks = (lanes + 255) / 256;
    if (blocks > 256LL * 16) blocks = 256LL * 16;
    hipLaunchKernelGGL(hash_bwd2_table_kernel<F>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, xyzs, denc, ddx, *lv, n, dtable);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_hash_bwd2_gather_f32(const float* xyzs, const float* table, const float* denc, const float* ddx, const ngp_hash_levels* lv, int n,
                             float* d_denc, float* d_xyzs, void* stream) {
    if (n <= 0) return 0;
    if (lv->n_levels < 1 || lv->n_levels > NGP_MAX_LEVELS) return -1;
    switch (lv->n_features) {
        case 1: return launch_bwd2_gather<1, false>(xyzs, table, denc, ddx, lv, n, d_denc, d_xyzs, stream);
        case 2: return launch_bwd2_gather<2, false>(xyzs, table, denc, ddx, lv, n, d_denc, d_xyzs, stream);
        case 4: return launch_bwd2_gather<4, false>(xyzs, table, denc, ddx, lv, n, d_denc, d_xyzs, stream);
        case 8: return launch_bwd2_gather<8, false>(xyzs, table, denc, ddx, lv, n, d_denc, d_xyzs, stream);
        default: return -1;
    }
}

int ngp_hash_bwd2_gather_bf16(const float* xyzs, const uint16_t* table, const float* denc, const float* ddx, const ngp_hash_levels* lv,
                              int n, float* d_denc, float* d_xyzs, void* stream) {
    if (n <= 0) return 0;
    if (lv->n_levels < 1 || lv->n_levels > NGP_MAX_LEVELS || lv->n_features != 2) return -1;
    return launch_bwd2_gather<2, true>(xyzs, table, denc, ddx, lv, n, d_denc, d_xyzs, stream);
}

int ngp_hash_bwd2_table_f32(const float* xyzs, const float* denc, const float* ddx, const ngp_hash_levels* lv, int n, float* dtable,
                            void* stream) {
    if (n <= 0) return 0;
    if (lv->n_levels < 1 || lv->n_levels > NGP_MAX_LEVELS) return -1;
    switch (lv->n_features) {
        case 1: return launch_bwd2_table<1>(xyzs, denc, ddx, lv, n, dtable, stream);
        case 2: {
            const int tiles = (n + 15) / 16;
            const int g2 = tiles < 4 ? 1 : (tiles / 4 < 8192 ? (tiles + 3) / 4 : 8192);
            hipLaunchKernelGGL(hash_bwd2_table_f32x2_kernel, dim3(g2), dim3(256), 0, (hipStream_t)stream, xyzs, denc, ddx, *lv, n, dtable);
            NGP_LAUNCH_CHECK();
            return 0;
        }
        case 4: return launch_bwd2_table<4>(xyzs, denc, ddx, lv, n, dtable, stream);
        case 8: return launch_bwd2_table<8>(xyzs, denc, ddx, lv, n, dtable, stream);
        default: return -1;
    }
}

}  // extern "C"
