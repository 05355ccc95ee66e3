// triplane.hip -- tri-plane position encoding (fwd gather / bwd scatter-add) for gfx950.
//
// Replaces modules/triplane.py of the reference: the forward kernel (:35-98) and its Taichi-autodiff backward (the glue's
// `kernel.grad`, :186-198).  NGP(pos_encoder_type='triplane') builds it with base_res 16, 8 levels, 4 features.
//
// Layout: table = 3 planes (x,y), (y,z), (z,x) of max_res^2 entries x F features each; entry (plane p, index, feature j) is
// p*max_res^2*F + index*F + j, index = a + b*max_res with `a` the plane's first coordinate.  out / dout are [n, L*F] FEATURE-major
// (column j*L + level) -- the hash encoder's are level-major.  Every level indexes the same full-resolution planes: grid point g of a
// level of resolution res maps to u32(f32(g) / f32(res) * f32(max_res - 1)).  Inputs are clamped to [0, 1] (the reference reads out of
// bounds for anything else).
// Kernels:
//   triplane_fwd_kernel  one lane per (sample, level), level fastest: twelve 16-byte gathers (4 corners x 3 planes) and 4 outputs
//   triplane_bwd_kernel  one lane per sample, looping over the levels; re-gathers the three per-plane sums (the gradient depends on the
//                        table) and scatters 12 x F products per level.  The first `lds_levels` levels -- whose (res+1)^2 grid points
//                        of all three planes fit TP_LDS_FLOATS -- are summed in LDS per workgroup and each touched point is flushed
//                        once.  On every level the lanes of a wave first merge runs of equal destinations (consecutive samples of one
//                        ray share cells) and only each run's first lane issues the (LDS or global) float atomics.
#include "ngp_device.h"
#include "hash_common.h"

namespace ngp {

constexpr int TP_F = 4;                         // the reference's feature_per_level (networks.py:101-107); float4 gathers
constexpr int TP_LDS_FLOATS = 20480;            // 80 KB: levels 0-1 at max_res 1024 (57 KB) and at 4096 (78 KB)
constexpr int TP_BWD_THREADS = 512;
constexpr int TP_BWD_MAX_BLOCKS = 512;          // two 80-KB workgroups per CU (256 CUs); samples beyond stride through

struct TriLevels {
    uint32_t res[NGP_MAX_LEVELS];
    int n_levels;
    uint32_t max_res;
    int lds_levels;                                          // backward: levels [0, lds_levels) accumulate in LDS
    uint32_t lds_base[NGP_MAX_LEVELS + 1];                   // first float of level l's LDS block (3 planes x (res+1)^2 x F)
};

// Per-axis corner data of one (sample, level): the two grid points' full-resolution coordinates and their weights.
struct Axis {
    uint32_t ori[2];
    float w[2];
};

__device__ __forceinline__ uint32_t to_full_res(uint32_t g, uint32_t res, uint32_t max_res) {
    // the reference's `pos_grid_local / resolution * (max_res - 1)` then a truncating cast: f32 divide (correctly rounded: no
    // -ffast-math anywhere in the build) and a multiply, kept separate by -ffp-contract=off
    return (uint32_t)(((float)g / (float)res) * (float)(max_res - 1u));
}

__device__ __forceinline__ void axis_of(float x, uint32_t res, uint32_t max_res, uint32_t& g, Axis& a) {
    x = fminf(fmaxf(x, 0.0f), 1.0f);
    const float pos = x * (float)(res - 1u) + 0.5f;
    g = (uint32_t)floorf(pos);
    const float fr = pos - (float)g;
    a.w[0] = 1.0f - fr;
    a.w[1] = fr;
    a.ori[0] = to_full_res(g, res, max_res);
    a.ori[1] = to_full_res(g + 1u, res, max_res);
}

__device__ __forceinline__ void load_xyz(const float* __restrict__ xyzs, long i, const XyzNorm& nm, float v[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = norm01(nm, xyzs[i * 3 + k]);
}

// Plane p pairs axes (p, (p + 1) % 3): (x,y), (y,z), (z,x).  Corner c: bit 0 steps the first coordinate, bit 1 the second.
// lf[p] = sum over c = 0..3, in that order, of w_c[p] * T[p, corner c]; the weight is (1 * w_a) * w_b as the reference forms it.
__device__ __forceinline__ void plane_sums(const float* __restrict__ table, const Axis ax[3], uint32_t max_res, float4 lf[3],
                                           float w[3][4], uint32_t idx[3][4]) {
    const size_t plane = (size_t)max_res * max_res;
    float4 t[3][4];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const int a = p, b = (p + 1) % 3;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            idx[p][c] = ax[a].ori[c & 1] + ax[b].ori[c >> 1] * max_res;
            w[p][c] = ax[a].w[c & 1] * ax[b].w[c >> 1];
            t[p][c] = *reinterpret_cast<const float4*>(table + ((size_t)p * plane + idx[p][c]) * TP_F);
        }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            s.x = s.x + w[p][c] * t[p][c].x;
            s.y = s.y + w[p][c] * t[p][c].y;
            s.z = s.z + w[p][c] * t[p][c].z;
            s.w = s.w + w[p][c] * t[p][c].w;
        }
        lf[p] = s;
    }
}

__global__ void __launch_bounds__(256) triplane_fwd_kernel(const float* __restrict__ xyzs, const float* __restrict__ table, TriLevels lv,
                                                           int n, XyzNorm nm, float* __restrict__ out) {
    const int L = lv.n_levels;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long)n * L) return;
    const long i = tid / L;
    const int level = (int)(tid - i * L);
    float v[3];
    load_xyz(xyzs, i, nm, v);
    const uint32_t res = lv.res[level];
    Axis ax[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t g;
        axis_of(v[k], res, lv.max_res, g, ax[k]);
    }
    float4 lf[3];
    float w[3][4];
    uint32_t idx[3][4];
    plane_sums(table, ax, lv.max_res, lf, w, idx);
    float* o = out + i * (long)(L * TP_F) + level;
    // ((1 * lf0) * lf1) * lf2 = (lf0 * lf1) * lf2 exactly
    o[0 * L] = (lf[0].x * lf[1].x) * lf[2].x;
    o[1 * L] = (lf[0].y * lf[1].y) * lf[2].y;
    o[2 * L] = (lf[0].z * lf[1].z) * lf[2].z;
    o[3 * L] = (lf[0].w * lf[1].w) * lf[2].w;
}

// Merge runs of equal `key` over consecutive lanes of the wave: afterwards the first lane of each run holds the run's sum in v.
// Every lane of the wave must call it (the shuffles are wave-wide); lanes with key == ~0u form runs of their own and are skipped
// by the caller.  Returns whether this lane heads its run.
__device__ __forceinline__ bool merge_runs(uint32_t key, float4& v) {
    const int lane = threadIdx.x & (NGP_WAVE - 1);
    const uint32_t prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    if (heads == ~0ull) return head;                          // every destination distinct in this wave: nothing to merge
    const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const int seg = __popcll(heads & le);
#pragma unroll
    for (int off = 1; off < NGP_WAVE; off <<= 1) {            // segmented suffix sum (Hillis-Steele): runs are contiguous
        const int oseg = __shfl_down(seg, off);
        const float ox = __shfl_down(v.x, off), oy = __shfl_down(v.y, off), oz = __shfl_down(v.z, off), ow = __shfl_down(v.w, off);
        if (lane + off < NGP_WAVE && oseg == seg) {
            v.x += ox; v.y += oy; v.z += oz; v.w += ow;
        }
    }
    return head;
}

__global__ void __launch_bounds__(TP_BWD_THREADS) triplane_bwd_kernel(const float* __restrict__ xyzs, const float* __restrict__ dout,
                                                                      const float* __restrict__ table, TriLevels lv, int n, XyzNorm nm,
                                                                      float* __restrict__ dtable) {
    __shared__ float acc[TP_LDS_FLOATS];
    const int L = lv.n_levels;
    const uint32_t M = lv.max_res;
    const size_t plane = (size_t)M * M;
    const uint32_t lds_end = lv.lds_base[lv.lds_levels];
    for (uint32_t k = threadIdx.x; k < lds_end; k += blockDim.x) acc[k] = 0.0f;
    __syncthreads();

    const int lane = threadIdx.x & (NGP_WAVE - 1);
    const long stride = (long)gridDim.x * blockDim.x;
    // the loop bound is wave-uniform (the wave's first sample), so every lane of a wave takes part in merge_runs' shuffles
    for (long base = (long)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += stride) {
        const long i = base + lane;
        const bool live = i < n;
        float v[3] = {0.0f, 0.0f, 0.0f};
        if (live) load_xyz(xyzs, i, nm, v);
        for (int level = 0; level < L; ++level) {
            float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (live) {
                const float* dr = dout + i * (long)(L * TP_F) + level;
                d = make_float4(dr[0 * L], dr[1 * L], dr[2 * L], dr[3 * L]);
            }
            const bool any = live && (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f || d.w != 0.0f);
            const uint32_t res = lv.res[level];
            Axis ax[3];
            uint32_t g[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) axis_of(v[k], res, M, g[k], ax[k]);
            float4 lf[3] = {};
            float w[3][4] = {};
            uint32_t idx[3][4] = {};
            if (any) plane_sums(table, ax, M, lf, w, idx);
            // d out_j / d lf_p = product of the other two planes' sums
            float4 dl[3];
            dl[0] = make_float4(d.x * (lf[1].x * lf[2].x), d.y * (lf[1].y * lf[2].y), d.z * (lf[1].z * lf[2].z), d.w * (lf[1].w * lf[2].w));
            dl[1] = make_float4(d.x * (lf[0].x * lf[2].x), d.y * (lf[0].y * lf[2].y), d.z * (lf[0].z * lf[2].z), d.w * (lf[0].w * lf[2].w));
            dl[2] = make_float4(d.x * (lf[0].x * lf[1].x), d.y * (lf[0].y * lf[1].y), d.z * (lf[0].z * lf[1].z), d.w * (lf[0].w * lf[1].w));
            if (level < lv.lds_levels) {                       // wave-uniform branch
                // merged first: the lanes of a wave mostly share these coarse cells, and same-address LDS adds serialise
                const uint32_t r1 = res + 1u;
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    const int a = p, b = (p + 1) % 3;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const uint32_t ga = g[a] + (c & 1), gb = g[b] + (c >> 1);         // <= res: inside the (res+1)^2 block
                        const uint32_t key = any ? lv.lds_base[level] + ((uint32_t)p * r1 * r1 + gb * r1 + ga) * TP_F : ~0u;
                        float4 gv = make_float4(w[p][c] * dl[p].x, w[p][c] * dl[p].y, w[p][c] * dl[p].z, w[p][c] * dl[p].w);
                        if (merge_runs(key, gv) && key != ~0u) {
                            float* e = acc + key;
                            atomicAdd(e + 0, gv.x);
                            atomicAdd(e + 1, gv.y);
                            atomicAdd(e + 2, gv.z);
                            atomicAdd(e + 3, gv.w);
                        }
                    }
                }
                continue;
            }
#pragma unroll
            for (int p = 0; p < 3; ++p) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t key = any ? (uint32_t)(p * plane + idx[p][c]) : ~0u;
                    float4 gv = make_float4(w[p][c] * dl[p].x, w[p][c] * dl[p].y, w[p][c] * dl[p].z, w[p][c] * dl[p].w);
                    if (merge_runs(key, gv) && key != ~0u) {
                        float* e = dtable + (size_t)key * TP_F;
                        unsafeAtomicAdd(e + 0, gv.x);
                        unsafeAtomicAdd(e + 1, gv.y);
                        unsafeAtomicAdd(e + 2, gv.z);
                        unsafeAtomicAdd(e + 3, gv.w);
                    }
                }
            }
        }
    }
    __syncthreads();
    // flush: every touched LDS float once (a grid point maps to one full-resolution entry; where two points of a level map to the
    // same entry both adds land there)
    for (int level = 0; level < lv.lds_levels; ++level) {
        const uint32_t res = lv.res[level], r1 = res + 1u, n_floats = lv.lds_base[level + 1] - lv.lds_base[level];
        const float* blk = acc + lv.lds_base[level];
        for (uint32_t k = threadIdx.x; k < n_floats; k += blockDim.x) {
            const float s = blk[k];
            if (s == 0.0f) continue;
            const uint32_t j = k % TP_F, pt = k / TP_F, p = pt / (r1 * r1), rem = pt - p * r1 * r1, gb = rem / r1, ga = rem - gb * r1;
            const uint32_t index = to_full_res(ga, res, M) + to_full_res(gb, res, M) * M;
            unsafeAtomicAdd(dtable + ((size_t)p * plane + index) * TP_F + j, s);
        }
    }
}

static bool tri_levels(const ngp_triplane_levels* in, TriLevels& lv) {
    if (!in || in->n_levels < 1 || in->n_levels > NGP_MAX_LEVELS || in->n_features != TP_F) return false;
    // 3 * max_res^2 * F < 2^32 (u32 entry keys) and resolutions exact in f32
    if (in->max_res < 2 || in->max_res > 16384) return false;
    lv = TriLevels{};
    lv.n_levels = in->n_levels;
    lv.max_res = (uint32_t)in->max_res;
    uint32_t used = 0;
    lv.lds_levels = 0;
    bool fits = true;
    for (int l = 0; l < in->n_levels; ++l) {
        const uint32_t r = in->resolution[l];
        if (r < 2 || r > (1u << 20)) return false;
        lv.res[l] = r;
        const unsigned long long need = 3ull * (r + 1ull) * (r + 1ull) * TP_F;
        if (fits && used + need <= (unsigned long long)TP_LDS_FLOATS) {
            lv.lds_base[l] = used;
            used += (uint32_t)need;
            lv.lds_levels = l + 1;
            lv.lds_base[l + 1] = used;
        } else {
            fits = false;
        }
    }
    return true;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_triplane_levels_init(ngp_triplane_levels* lv, double base_res, double max_res, int levels, int features) {
    if (!lv || levels < 2 || levels > NGP_MAX_LEVELS || features < 1 || max_res < 2.0 || max_res > 16384.0) return -1;
    *lv = ngp_triplane_levels{};
    // modules/utils.py:31-39 (f64), then the in-kernel grid_scale / grid_resolution of triplane.py:27-33 in f32 -- the very arithmetic of
    // ngp_hash_levels_init
    const double log_b = log(max_res / base_res) / (double)(levels - 1);
    for (int i = 0; i < levels; ++i) {
        const float sc = (float)base_res * expf((float)i * (float)log_b) - 1.0f;
        lv->scale[i] = sc;
        lv->resolution[i] = (uint32_t)ceilf(sc) + 1u;
    }
    lv->n_levels = levels;
    lv->n_features = features;
    lv->max_res = (int32_t)max_res;
    return 0;
}

int ngp_triplane_fwd_f32(const float* xyzs, const float* table, const ngp_triplane_levels* lvin, int n, int normalize, float lo,
                         float hi, float* out, void* stream) {
    if (n <= 0) return 0;
    TriLevels lv;
    if (!tri_levels(lvin, lv)) return -1;
    const long long lanes = (long long)n * lv.n_levels;
    const int grid = (int)((lanes + 255) / 256);
    XyzNorm nm = {normalize, lo, hi};
    hipLaunchKernelGGL(triplane_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, xyzs, table, lv, n, nm, out);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_triplane_bwd_f32(const float* xyzs, const float* dout, const float* table, const ngp_triplane_levels* lvin, int n,
                         int normalize, float lo, float hi, float* dtable, void* stream) {
    if (n <= 0) return 0;
    TriLevels lv;
    if (!tri_levels(lvin, lv)) return -1;
    long long blocks = ((long long)n + TP_BWD_THREADS - 1) / TP_BWD_THREADS;
    if (blocks > TP_BWD_MAX_BLOCKS) blocks = TP_BWD_MAX_BLOCKS;
    XyzNorm nm = {normalize, lo, hi};
    hipLaunchKernelGGL(triplane_bwd_kernel, dim3((unsigned)blocks), dim3(TP_BWD_THREADS), 0, (hipStream_t)stream, xyzs, dout, table, lv, n,
                       nm, dtable);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
