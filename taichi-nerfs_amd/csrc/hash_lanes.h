// hash_lanes.h -- lane-level pieces the hash encoder's gather and scatter kernels share, defined once: row access, the bf16 widening,
// the level view, A_c, the group tree, the gather kernels' launch shape, and the run-merging scatter (run head /
// tail, segmented scan, the F = 2 body).  The kernels must agree bit for bit on cells, indices, run boundaries and summation order.
// Used by hash_grid.hip (hash_fwd_f32_kernel's rows, hash_bwd_f32x2_kernel, hash_bwd_f16x2_kernel), hash_grad_input.hip
// (hash_bwd_input_kernel) and hash_grad_input2.hip (hash_bwd2_gather_kernel, hash_bwd2_table_kernel, hash_bwd2_table_f32x2_kernel).
#pragma once
#include "ngp_device.h"
#include "hash_common.h"
#include <hip/hip_fp16.h>

namespace ngp {

// Rows of F floats: one 8- or 16-byte access for F = 2 / 4.
template <int F>
__device__ __forceinline__ void load_row(const float* p, float (&r)[F]) {
    if constexpr (F == 2) { const float2 t = *reinterpret_cast<const float2*>(p); r[0] = t.x; r[1] = t.y; }
    else if constexpr (F == 4) { const float4 t = *reinterpret_cast<const float4*>(p); r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w; }
    else {
#pragma unroll
        for (int f = 0; f < F; ++f) r[f] = p[f];
    }
}
template <int F>
__device__ __forceinline__ void store_row(float* p, const float (&r)[F]) {
    if constexpr (F == 2) *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]);
    else if constexpr (F == 4) *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
    else {
#pragma unroll
        for (int f = 0; f < F; ++f) p[f] = r[f];
    }
}

// A bf16 pair (uint32 per entry) widened to f32: exact, so a kernel on the bf16 copy equals the f32 kernel on the rounded table.
__device__ __forceinline__ float2 bf16x2_to_f32(uint32_t u) {
    return make_float2(__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u));
}

// One level's constants.
struct LevelView { uint32_t res, size, mode, offset; float scale; bool dense; };
__device__ __forceinline__ LevelView level_at(const LevelLDS& L, const ngp_hash_levels& lv, int level) {
    return {L.res[level], L.size[level], L.mode[level], L.offset[level], L.scale[level], level < lv.begin_fast_hash_level};
}

// A_c of corner (xb, yb, zb) for w[axis][bit] and u = ddx: sum_k u_k * s_k(c) * prod_{j != k} w_j(c_j), s_k = +1 far / -1 near.
__device__ __forceinline__ float corner_A(const float (&w)[3][2], const float u[3], int xb, int yb, int zb) {
    const float ax = (xb ? u[0] : -u[0]) * (w[1][yb] * w[2][zb]);
    const float ay = (yb ? u[1] : -u[1]) * (w[2][zb] * w[0][xb]);
    const float az = (zb ? u[2] : -u[2]) * (w[0][xb] * w[1][yb]);
    return (ax + ay) + az;
}

// Fixed-order xor-shuffle tree over a group's lanes (group is a power of two <= 16 and divides the wave: partners stay in the group).
__device__ __forceinline__ void group_tree_sum3(float (&d)[3], int group) {
    for (int step = group >> 1; step >= 1; step >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] += __shfl_xor(d[k], step, NGP_WAVE);
    }
}

// Launch shape of the gather kernels: one lane per (sample, level), a sample's levels padded to the next power of two `group` <= 16.
struct SampleLevelGrid { int group; unsigned blocks; };
static inline SampleLevelGrid sample_level_grid(const ngp_hash_levels* lv, int n) {
    int group = 1;
    while (group < lv->n_levels) group <<= 1;
    const long long lanes = (long long)n * group;
    long long blocks = (lanes + 255) / 256;
    if (blocks > 256LL * 16) blocks = 256LL * 16;            // 256 CUs x 16 blocks, block-stride beyond that
    return {group, (unsigned)blocks};
}

// The run-merging scatter: a wave holds 64 / STRIDE consecutive samples of one level, STRIDE lanes each.  A run is a stretch of
// consecutive valid samples in one cell: `head` marks its first sample (or the tile's first, or an invalid lane), `tail` its last
// valid one (`last` = the tile's last sample slot).
template <int STRIDE>
__device__ __forceinline__ void run_head_tail(const uint32_t cell[3], bool valid, int s_in, int last, bool& head, bool& tail) {
    const uint32_t cx = cell[0], cy = cell[1], cz = cell[2];
    const uint32_t pcx = __shfl_up(cx, STRIDE, 64), pcy = __shfl_up(cy, STRIDE, 64), pcz = __shfl_up(cz, STRIDE, 64);
    const int pvalid = __shfl_up((int)valid, STRIDE, 64);
    head = (s_in == 0) || !valid || !pvalid || cx != pcx || cy != pcy || cz != pcz;
    const int nhead = __shfl_down((int)head, STRIDE, 64);
    tail = valid && ((s_in == last) || nhead);
}
// Segmented inclusive scan over samples (lane distance STRIDE = one sample): afterwards a run's tail holds the run's sums.
template <int STRIDE, int N>
__device__ __forceinline__ void seg_scan_up(float (&v)[N], bool head) {
    const int lane = threadIdx.x & 63;
    bool hf = head;
#pragma unroll
    for (int d = STRIDE; d < 64; d <<= 1) {
        const int hup = __shfl_up((int)hf, d, 64);
        float vup[N];
#pragma unroll
        for (int k = 0; k < N; ++k) vup[k] = __shfl_up(v[k], d, 64);
        if (lane >= d && !hf) {
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] += vup[k];
            hf = hup != 0;
        }
    }
}

// The F = 2 float-atomic scatter, shaped by what the MI355X atomic pipeline charges for (profiles/microbench/atomics2.hip):
// a float atomic instruction costs one request per DISTINCT 64-byte line it touches (~21 G lines/s chip-wide),
// adjacent lanes on one line are free, and duplicate addresses inside an instruction are NOT merged.
//   * lane quad = (sample, x-corner bit, feature): the four lanes of a quad hit (e, f0) (e, f1) (e', f0) (e', f1)
//     where e' is the x-neighbour entry -- adjacent (dense levels) or e^small-mask (xor hash) -- so the quad lands
//     on one 64-B line 7 times out of 8: ~4 line requests per (sample, level) instead of 16 scattered atomics.
//   * one wave = 16 consecutive samples x one level; consecutive samples of a ray sit in the same cell on the
//     coarse/mid levels, so equal-cell runs are summed with a segmented wave scan and only the last lane of a
//     run issues atomics (removes the in-instruction duplicates and ~60 % of all requests).
// Sums that are exactly 0 issue no atomic.  The policy S says what is scattered -- how a sample is fetched: S.count(n) samples (a
// device-side count may lower n), S.fetch(i, valid, p) its position and what else S keeps of it (zeros past the end), S.grad(i, level,
// f) its gradient, S.seen(g) on every value that passes -- and S.weight(fr, scale, xb, yb, zb), the factor of a corner.  bdim is the
// kernel's blockDim.x: read inside a device function it compiles to the general form (a load, a select for a partial last block).
template <class Policy>
__device__ __forceinline__ void scatter_runs_f32x2(const ngp_hash_levels& lv, int n, float* __restrict__ dtable, unsigned bdim, Policy S) {
    __shared__ LevelLDS L;
    load_levels(lv, L);
    n = S.count(n);
    const int nl = lv.n_levels;
    const int lane = threadIdx.x & 63;
    const int s_in = lane >> 2, xb = (lane >> 1) & 1, f = lane & 1;
    const int n_tiles = (n + 15) >> 4;
    const int waves_per_block = bdim >> 6;
    for (int tile = blockIdx.x * waves_per_block + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * waves_per_block) {
        const int i = tile * 16 + s_in;                  // position in the gradient rows (and in the live list, when there is one)
        const bool valid = i < n;
        float p[3];
        S.fetch(i, valid, p);
        for (int level = 0; level < nl; ++level) {
            const float g = valid ? S.grad(i, level, f) : 0.0f;
            S.seen(g);
            const LevelView l = level_at(L, lv, level);
            uint32_t cell[3];
            float fr[3];
            cell_frac<false>(p, l.scale, cell, fr);
            bool head, tail;
            run_head_tail<4>(cell, valid, s_in, 15, head, tail);
            float v[4];
            uint32_t e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {              // k = (z bit, y bit)
                e[k] = l.offset + level_index(l.dense, l.mode, l.size, l.res, cell[0] + (uint32_t)xb, cell[1] + (uint32_t)(k & 1), cell[2] + (uint32_t)(k >> 1));
                v[k] = S.weight(fr, l.scale, xb, k & 1, k >> 1) * g;
            }
            seg_scan_up<4>(v, head);
            if (tail) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (v[k] != 0.0f) unsafeAtomicAdd(dtable + (size_t)e[k] * 2 + f, v[k]);
            }
        }
    }
}

}  // namespace ngp
