// sdf_trace.hip -- the geometry value of a trained SDFField and a sphere tracer over it, for gfx950.
//
// ngp_hip/surface.py renders a signed-distance field through the training path: dozens of samples per ray, sdf_and_grad through
// autograd on each, the NeuS compositor.  At test time a surface needs ONE point per pixel: walk the ray by the distance the field
// reports, stop at the zero crossing, shade there.  This file holds the field value as one device function and two kernels on it:
//   sdf_point        x01 = (x - lo) / (hi - lo) (XyzNorm, the two f32 operations of SDFField._geometry); the F = 2 embedding of up to 16
//                    dense / hashed levels through the corner rule of hash_common.h / hash_lanes.h with the multiply-then-add
//                    accumulation of hash_fwd_f32_kernel (bit-identical to ops.hash_fwd_f32, positions on faces and outside the box
//                    included; every index stays inside its level); [x | enc] -> `depth` hidden layers of `width` -> row 0 of the last
//                    layer.  Every sum runs in input-index order as explicit fmaf, bias first; the activation is torch's
//                    Softplus(beta = 100): z = 100 h; z > 20 ? h : log1pf(expf(z)) / 100.  All arithmetic is fp32.
//   sdf_eval_kernel  one lane per point, grid-stride: f[n] and, optionally, the embedding rows.
//   sdf_trace_kernel one lane owns a ray and runs the sphere-tracing rule of include/ngp_hip.h ("sphere tracing").
//
// WEIGHTS.  One fp32 pack: W0[width][3+2L] | b0[width] | (Wi[width][width] | bi[width]).. | w_out[width] | b_out; 6529 floats = 26 KB
// for the default 35 -> 64 -> 64 -> 1.  Every lane of a wave needs the same weight at the same time.  deploy.hip reads its 1280 weights
// as scalar loads at compile-time offsets of a fully unrolled network; that does not carry over: 6529 multiply-adds unrolled are 50 KB
// of v_fma alone against a 64 KB instruction cache, and 26 KB of weights do not stay in a 16 KB scalar cache.  deploy.hip's other
// finding -- an LDS copy whose loop-invariant reads got hoisted into 512 VGPRs -- came from the unrolled form too.  Here each block
// stages the pack into LDS once and a layer is a RUNTIME loop over its neurons: the reads depend on the loop counter, so nothing can
// be hoisted, and the inner loops (compile-time indices into register arrays) are 9 or 16 ds_read_b128 of one address for all lanes
// (a broadcast: 4 weights per 4 LDS cycles, the rate at which one wave per SIMD issues v_fma_f32).  To keep every register index a
// compile-time constant without a second activation array, layers go in pairs: neuron o of the first layer is a dot product over the
// inputs in registers (row o of W, padded to 36 floats with zeros: fmaf(0, 0, t) = t), and its activation is at once added into all
// accumulators of the next layer, acc[k] = fmaf(h_o, W'[k][o], acc[k]) -- o ascending = input-index order, the accumulators start at
// the bias.  That walk reads a COLUMN of W', so the staging transposes W' in LDS.  Depth 1 adds h_o into the output sum directly.
// The embedding is produced by a runtime loop over groups of four levels (32 gathers in flight, one basic block per group) and goes
// through a per-lane LDS column, because a register array cannot be indexed by the loop counter without scratch.
// LDS per 256-thread block (width 64, depth 2): weights 26.4 KB + embedding columns 32 KB + coarse occupancy 4 KB + level table:
// 63 KB, two blocks per CU.  Compiler resource usage (hipcc 7, -O3, gfx950) of the default instantiations:
//   sdf_trace_kernel<64, 2, true>   VGPRs: 253  SGPRs: 106  scratch: 0 B  LDS: 63568 B  (one cascade)
//   sdf_trace_kernel<64, 2, false>  VGPRs: 253  SGPRs: 106  scratch: 0 B  LDS: 63568 B
//   sdf_eval_kernel<64, 2>          VGPRs: 254  SGPRs: 105  scratch: 0 B  LDS: 59472 B
//   width 16 / 32, depth 1 / 2      VGPRs: 151-218 (trace), 110-174 (eval); scratch: 0 B everywhere
// 256 registers and 63.6 KB of LDS both allow two blocks = eight waves per CU, two per SIMD (the compiler's own occupancy line says 1:
// it rates the 256-thread block against its registers alone).  The 64 accumulators, the 36 inputs and a group's 32 gathered rows
// account for the registers; nothing spills.
//
// LANES.  The launch is at most SDF_MAX_BLOCKS blocks (two per CU); the rays are dealt to the waves in chunks of 64 consecutive rays,
// chunk c to wave c mod n_waves, so every wave's pool is spread over the whole batch.  Measured against the first version, 256
// CONSECUTIVE rays per wave (profiles/sdf_trace.json): a 96 x 96 frame 8.8 ms against 12.1, an 800 x 800 frame 19.4 ms against
// 15.7 -- with consecutive rays the 12 % of that frame that meets the surface sat in ~300 of 2500 waves, one busy wave per CU, but
// those waves' lanes moved in step; spread out, every round of a wave waits for freshly started rays to walk through empty space
// (hundreds of dt_min skips) before anyone evaluates: 54 % of the evaluation slots idle against 43 %.  The walk is the thing to cut
// next (a cap on skips per round, so that waiting lanes evaluate while others walk); neither layout is near the arithmetic.  A lane whose ray has finished writes its five outputs and takes the next unstarted ray of the wave's pool (rank
// among the finished lanes by ballot: a wave-uniform counter, no atomic, no LDS), so lanes idle only while the pool's last rays finish.  Each round every live lane first walks through empty occupancy cells (probe_cell / skip_target, the
// coarse bits in LDS first: cheap and divergent) up to its next evaluation point; then the lanes that need a value call sdf_point
// TOGETHER, once per round -- a bisection step is such a round too -- and each steps its own state machine.  An output is a function
// of its ray alone: which lane or round evaluates a point does not enter any value, and nothing is accumulated across rays.
#include "ngp_device.h"
#include "hash_common.h"
#include "hash_lanes.h"
#include "march_common.h"

namespace ngp {

constexpr int SDF_NIN = 36;                       // 3 + 2 * NGP_MAX_LEVELS inputs, padded to whole float4s
constexpr int SDF_BLOCK = 256;
constexpr int SDF_MAX_BLOCKS = 512;               // 256 CUs x the two blocks that fit a CU's LDS
constexpr int SDF_LEVEL_GROUP = 4;                // levels whose 32 gathers are issued together
enum { SDF_MISS = 0, SDF_HIT = 1, SDF_INSIDE = 2, SDF_ABANDONED = 3 };

// where the staged network sits in LDS (float offsets, all multiples of 4: rows are read as float4)
template <int W, int D>
struct SdfLds {
    static constexpr int W0 = 0, B0 = W * SDF_NIN, W1T = B0 + W, B1 = W1T + (D == 2 ? W * W : 0), WO = B1 + (D == 2 ? W : 0), BO = WO + W,
                         FLOATS = BO + 4;
};

template <int W, int D>
__device__ __forceinline__ void sdf_stage_weights(const float* __restrict__ wpack, int nin, float* __restrict__ ws) {
    using O = SdfLds<W, D>;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int k = tid; k < W * SDF_NIN; k += nt) {
        const int o = k / SDF_NIN, j = k - o * SDF_NIN;
        ws[O::W0 + k] = j < nin ? wpack[o * nin + j] : 0.0f;
    }
    const float* p = wpack + W * nin;
    for (int k = tid; k < W; k += nt) ws[O::B0 + k] = p[k];
    p += W;
    if constexpr (D == 2) {
        for (int k = tid; k < W * W; k += nt) {
            const int o = k / W, kk = k - o * W;                   // LDS [input o][output kk] <- pack [output kk][input o]
            ws[O::W1T + k] = p[kk * W + o];
        }
        for (int k = tid; k < W; k += nt) ws[O::B1 + k] = p[W * W + k];
        p += W * W + W;
    }
    for (int k = tid; k < W; k += nt) ws[O::WO + k] = p[k];
    if (tid == 0) ws[O::BO] = p[W];
    __syncthreads();
}

__device__ __forceinline__ float sdf_softplus(float h) {           // torch.nn.Softplus(beta = 100, threshold = 20)
    const float z = 100.0f * h;
    return z > 20.0f ? h : log1pf(expf(z)) / 100.0f;
}

// The field's geometry value at the world position xyz: the only spelling of it in the library.  L: the level table in LDS; ws: the
// staged network; enc_col: this lane's LDS column (element c at enc_col[c * SDF_BLOCK]); enc_out (wave-uniform, may be null): row i
// of it receives the 2 * n_levels embedding floats.
template <int W, int D>
__device__ __forceinline__ float sdf_point(const float xyz[3], const float* __restrict__ table, const ngp_hash_levels& lv, const LevelLDS& L,
                                           const XyzNorm& nm, const float* __restrict__ ws, float* __restrict__ enc_col,
                                           float* __restrict__ enc_out, size_t i) {
    using O = SdfLds<W, D>;
    const int nl = lv.n_levels;
    const float p01[3] = {norm01(nm, xyz[0]), norm01(nm, xyz[1]), norm01(nm, xyz[2])};
    const float2* __restrict__ rows = reinterpret_cast<const float2*>(table);

    // ---- embedding: groups of four levels, a group's 32 gathers in one basic block (a level past the last repeats the last one and
    // is not stored).  Corner rule and accumulation of hash_fwd_f32_kernel<2>: acc = 0; acc += w_c * v_c, c = 0..7, mul then add.
#pragma unroll 1
    for (int g = 0; g < nl; g += SDF_LEVEL_GROUP) {
        float2 v[SDF_LEVEL_GROUP][8];
        float w[SDF_LEVEL_GROUP][8];
#pragma unroll
        for (int u = 0; u < SDF_LEVEL_GROUP; ++u) {
            const int level = min(g + u, nl - 1);
            const LevelView l = level_at(L, lv, level);
            uint32_t cell[3];
            float fr[3];
            cell_frac<false>(p01, l.scale, cell, fr);
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) {
                const uint32_t e = l.offset + level_index(l.dense, l.mode, l.size, l.res, cell[0] + (uint32_t)(ci & 1),
                                                          cell[1] + (uint32_t)((ci >> 1) & 1), cell[2] + (uint32_t)(ci >> 2));
                v[u][ci] = rows[e];
                w[u][ci] = corner_weight(ci, fr);
            }
        }
#pragma unroll
        for (int u = 0; u < SDF_LEVEL_GROUP; ++u) {
            float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) { a0 += w[u][ci] * v[u][ci].x; a1 += w[u][ci] * v[u][ci].y; }
            if (g + u < nl) {
                enc_col[(2 * (g + u)) * SDF_BLOCK] = a0;
                enc_col[(2 * (g + u) + 1) * SDF_BLOCK] = a1;
            }
        }
    }
    float in[SDF_NIN];
    in[0] = xyz[0]; in[1] = xyz[1]; in[2] = xyz[2]; in[SDF_NIN - 1] = 0.0f;
#pragma unroll
    for (int c = 0; c < 2 * NGP_MAX_LEVELS; ++c) in[3 + c] = c < 2 * nl ? enc_col[c * SDF_BLOCK] : 0.0f;   // the lane's own stores
    if (enc_out) {
#pragma unroll
        for (int l = 0; l < NGP_MAX_LEVELS; ++l)
            if (l < nl) *reinterpret_cast<float2*>(enc_out + i * (size_t)(2 * nl) + 2 * l) = make_float2(in[3 + 2 * l], in[4 + 2 * l]);
    }

    // ---- network
    float f = ws[O::BO];
    if constexpr (D == 1) {
#pragma unroll 1
        for (int o = 0; o < W; ++o) {
            const float4* __restrict__ wr = reinterpret_cast<const float4*>(ws + O::W0 + o * SDF_NIN);
            float t = ws[O::B0 + o];
#pragma unroll
            for (int q = 0; q < SDF_NIN / 4; ++q) {
                const float4 w4 = wr[q];
                t = fmaf(in[4 * q], w4.x, t); t = fmaf(in[4 * q + 1], w4.y, t); t = fmaf(in[4 * q + 2], w4.z, t); t = fmaf(in[4 * q + 3], w4.w, t);
            }
            f = fmaf(sdf_softplus(t), ws[O::WO + o], f);
        }
    } else {
        float acc[W];
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] = ws[O::B1 + k];
#pragma unroll 1
        for (int o = 0; o < W; ++o) {
            const float4* __restrict__ wr = reinterpret_cast<const float4*>(ws + O::W0 + o * SDF_NIN);
            float t = ws[O::B0 + o];
#pragma unroll
            for (int q = 0; q < SDF_NIN / 4; ++q) {
                const float4 w4 = wr[q];
                t = fmaf(in[4 * q], w4.x, t); t = fmaf(in[4 * q + 1], w4.y, t); t = fmaf(in[4 * q + 2], w4.z, t); t = fmaf(in[4 * q + 3], w4.w, t);
            }
            const float h = sdf_softplus(t);
            const float4* __restrict__ wc = reinterpret_cast<const float4*>(ws + O::W1T + o * W);
#pragma unroll
            for (int q = 0; q < W / 4; ++q) {
                const float4 w4 = wc[q];
                acc[4 * q] = fmaf(h, w4.x, acc[4 * q]); acc[4 * q + 1] = fmaf(h, w4.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(h, w4.z, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(h, w4.w, acc[4 * q + 3]);
            }
        }
#pragma unroll
        for (int k = 0; k < W; ++k) f = fmaf(sdf_softplus(acc[k]), ws[O::WO + k], f);
    }
    return f;
}

template <int W, int D>
__global__ void __launch_bounds__(SDF_BLOCK) sdf_eval_kernel(const float* __restrict__ xyzs, const float* __restrict__ table, ngp_hash_levels lv,
                                                             const float* __restrict__ wpack, XyzNorm nm, int n, float* __restrict__ f_out,
                                                             float* __restrict__ enc_out) {
    __shared__ LevelLDS L;
    __shared__ __attribute__((aligned(16))) float ws[SdfLds<W, D>::FLOATS];
    __shared__ float enc_s[2 * NGP_MAX_LEVELS][SDF_BLOCK];
    load_levels(lv, L);
    sdf_stage_weights<W, D>(wpack, 3 + 2 * lv.n_levels, ws);
    for (long long i = (long long)blockIdx.x * SDF_BLOCK + threadIdx.x; i < (long long)n; i += (long long)gridDim.x * SDF_BLOCK) {
        const float p[3] = {xyzs[3 * (size_t)i], xyzs[3 * (size_t)i + 1], xyzs[3 * (size_t)i + 2]};
        f_out[i] = sdf_point<W, D>(p, table, lv, L, nm, ws, &enc_s[0][threadIdx.x], enc_out, (size_t)i);
    }
}

struct SdfTraceParams {
    float eps, step_scale, min_step;
    int n_refine, max_evals;
};

template <int W, int D, bool CASC1>
__global__ void __launch_bounds__(SDF_BLOCK) sdf_trace_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                              const uint8_t* __restrict__ bits, const uint32_t* __restrict__ coarse,
                                                              const float* __restrict__ table, ngp_hash_levels lv,
                                                              const float* __restrict__ wpack, XyzNorm nm, MarchParams p, SdfTraceParams tp,
                                                              int n_rays, int32_t* __restrict__ status_out, float* __restrict__ t_out,
                                                              float* __restrict__ xyz_out, int32_t* __restrict__ n_eval_out,
                                                              float* __restrict__ f_last_out, unsigned long long* __restrict__ stats) {
    __shared__ LevelLDS L;
    __shared__ uint32_t coarse_s[MARCH_MAX_COARSE_WORDS];
    __shared__ __attribute__((aligned(16))) float ws[SdfLds<W, D>::FLOATS];
    __shared__ float enc_s[2 * NGP_MAX_LEVELS][SDF_BLOCK];
    load_levels(lv, L);
    const bool use_coarse = load_coarse(p, coarse, coarse_s);
    sdf_stage_weights<W, D>(wpack, 3 + 2 * lv.n_levels, ws);

    const int lane = threadIdx.x & 63;
    // the wave's pool: chunks wave, wave + n_waves, ..; pool position q is ray (wave + (q >> 6) n_waves) 64 + (q & 63)
    const int n_chunks = (int)(((long long)n_rays + 63) >> 6), n_waves = (int)gridDim.x * (SDF_BLOCK / 64);
    const int wave = (int)blockIdx.x * (SDF_BLOCK / 64) + (int)(threadIdx.x >> 6);
    if (wave >= n_chunks) return;                                                    // (no block barrier below)
    const int end = ((n_chunks - wave + n_waves - 1) / n_waves) * 64;                // pool positions; the batch's last chunk may be short
    int next = 0;                                                                    // wave-uniform: the pool's next unstarted position

    int r = -1, n_eval = 0, k_ref = 0;
    bool done = true, refine = false, have_prev = false;
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 1.f}, d_inv[3] = {0.f, 0.f, 1.f};
    float t = 0.f, t2 = 0.f, prev_t = 0.f, prev_f = 0.f, ta = 0.f, fa = 0.f, tb = 0.f, fb = 0.f, f_last = 0.f;
    unsigned long long slots = 0ull, used = 0ull;                                    // wave-uniform: lane slots of the evaluation rounds

    auto finish = [&](int status, float tf) {
        const size_t rr = (size_t)r;
        status_out[rr] = status;
        t_out[rr] = tf;
        xyz_out[3 * rr] = o[0] + tf * d[0]; xyz_out[3 * rr + 1] = o[1] + tf * d[1]; xyz_out[3 * rr + 2] = o[2] + tf * d[2];
        n_eval_out[rr] = n_eval;
        f_last_out[rr] = f_last;
        done = true;
    };

    for (;;) {
        // ---- finished lanes take the wave's next rays
        const unsigned long long fmask = __ballot(done);
        if (fmask != 0ull && next < end) {
            const int cand = next + __popcll(fmask & ((1ull << lane) - 1ull));
            const long long ray = ((long long)(wave + (cand >> 6) * n_waves) << 6) + (cand & 63);
            if (done && cand < end && ray < (long long)n_rays) {
                r = (int)ray;
#pragma unroll
                for (int k = 0; k < 3; ++k) { o[k] = rays_o[3 * (size_t)r + k]; d[k] = rays_d[3 * (size_t)r + k]; d_inv[k] = 1.0f / d[k]; }
                const float2 h = ray_aabb_slab(o, d_inv, p.scale);
                t = h.x; t2 = h.y;
                n_eval = 0; k_ref = 0; refine = false; have_prev = false; f_last = 0.0f; done = false;
                if (!(t2 >= 0.0f && t2 < INFINITY)) finish(SDF_MISS, -1.0f);           // a miss on the slab (t2 = -1), or no finite exit
            }
            next = min(end, next + __popcll(fmask));
        }
        if (!__any(!done)) {
            if (next >= end) break;
            continue;
        }
        // ---- every live lane walks to its next evaluation point
        bool pending = false;
        float te = t;
        if (!done) {
            if (refine) {
                te = 0.5f * (ta + tb);
                pending = true;
            } else {
                for (;;) {
                    if (!(t < t2)) { finish(SDF_MISS, t2); break; }
                    CellProbe c;
                    probe_cell<CASC1>(p, o, d, t, p.dt_min, c);
                    bool occ = true;
                    if (use_coarse) { const uint32_t cb = c.idx >> 9; occ = (coarse_s[cb >> 5] >> (cb & 31u)) & 1u; }
                    if (occ) occ = (bits[c.idx >> 3] >> (c.idx & 7u)) & 1u;
                    if (occ) {
                        if (n_eval >= tp.max_evals) finish(SDF_ABANDONED, t);
                        else { pending = true; te = t; }
                        break;
                    }
                    const float tn = skip_target(p, d, d_inv, t, c) + p.dt_min;      // inside the next cell, never on its face
                    have_prev = false;
                    if (!(tn > t)) { finish(SDF_ABANDONED, t); break; }              // t so large that the skip is below its ulp
                    t = tn;
                }
            }
        }
        const unsigned long long pmask = __ballot(pending);
        if (pmask == 0ull) continue;
        slots += 64ull; used += (unsigned long long)__popcll(pmask);
        // ---- one evaluation for every lane that needs one
        if (pending) {
            const float x[3] = {o[0] + te * d[0], o[1] + te * d[1], o[2] + te * d[2]};
            const float f = sdf_point<W, D>(x, table, lv, L, nm, ws, &enc_s[0][threadIdx.x], nullptr, 0);
            n_eval += 1;
            f_last = f;
            if (!(fabsf(f) < INFINITY)) {
                finish(SDF_ABANDONED, te);
            } else if (!refine) {
                if (f > tp.eps) {
                    prev_t = t; prev_f = f; have_prev = true;
                    const float step = f * tp.step_scale;
                    t = t + fmaxf(step, tp.min_step);
                } else if (f >= 0.0f) {
                    finish(SDF_HIT, t);
                } else if (!have_prev) {
                    finish(SDF_INSIDE, t);
                } else {
                    ta = prev_t; fa = prev_f; tb = t; fb = f; k_ref = 0; refine = true;
                }
            } else {
                if (f >= 0.0f) { ta = te; fa = f; } else { tb = te; fb = f; }
                k_ref += 1;
            }
            if (!done && refine && k_ref >= tp.n_refine) {
                const float num = (tb - ta) * fa, den = fa - fb;
                const float th = ta + num / den;
                if (fabsf(th) < INFINITY) finish(SDF_HIT, th); else finish(SDF_ABANDONED, tb);
            }
        }
    }
    if (stats && lane == 0) {
        atomicAdd(stats, slots);
        atomicAdd(stats + 1, used);
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" {

// the F = 2 level table of at most 16 levels, every level inside the table, and a network this file instantiates -- or false
static bool sdf_arch_ok(const ngp_hash_levels* lv, int width, int depth) {
    if (!lv || lv->n_levels < 1 || lv->n_levels > NGP_MAX_LEVELS || lv->n_features != 2 || lv->total_entries < 1) return false;
    for (int l = 0; l < lv->n_levels; ++l) {
        if (lv->map_size[l] == 0 || lv->resolution[l] == 0) return false;
        if ((uint64_t)lv->offset[l] + lv->map_size[l] > (uint64_t)lv->total_entries) return false;
    }
    return (width == 16 || width == 32 || width == 64) && (depth == 1 || depth == 2);
}

#define SDF_DISPATCH(CALL)                                                   \
    do {                                                                     \
        if (depth == 1) {                                                    \
            if (width == 16) { CALL(16, 1); } else if (width == 32) { CALL(32, 1); } else { CALL(64, 1); } \
        } else {                                                             \
            if (width == 16) { CALL(16, 2); } else if (width == 32) { CALL(32, 2); } else { CALL(64, 2); } \
        }                                                                    \
    } while (0)

int ngp_sdf_eval(const float* xyzs, const float* table, const ngp_hash_levels* lv, const float* wpack, int width, int depth, float scale,
                 int n, float* f, float* enc_out, void* stream) {
    if (n < 0 || !sdf_arch_ok(lv, width, depth) || !(scale > 0.0f && scale < INFINITY)) return -1;
    if (!xyzs || !table || !wpack || !f) return -1;
    if (((uintptr_t)table & 7u) || ((uintptr_t)enc_out & 7u)) return -1;              // 8-byte gathers / stores
    if (n == 0) return 0;
    const XyzNorm nm = {1, -scale, scale};
    int blocks = (n + SDF_BLOCK - 1) / SDF_BLOCK;
    if (blocks > 256 * 2) blocks = 256 * 2;
#define SDF_EVAL_CALL(W, D) \
    hipLaunchKernelGGL((sdf_eval_kernel<W, D>), dim3(blocks), dim3(SDF_BLOCK), 0, (hipStream_t)stream, xyzs, table, *lv, wpack, nm, n, f, enc_out)
    SDF_DISPATCH(SDF_EVAL_CALL);
#undef SDF_EVAL_CALL
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_sdf_trace(const float* rays_o, const float* rays_d, const uint8_t* density_bitfield, const uint32_t* coarse, const float* table,
                  const ngp_hash_levels* lv, const float* wpack, int width, int depth, int cascades, float scale, int grid_size, int n_rays,
                  float eps, float step_scale, float min_step, int n_refine, int max_evals, int32_t* status, float* t, float* xyz,
                  int32_t* n_eval, float* f_last, unsigned long long* stats, void* stream) {
    if (n_rays < 0 || !sdf_arch_ok(lv, width, depth) || !(scale > 0.0f && scale < INFINITY)) return -1;
    if (!rays_o || !rays_d || !density_bitfield || !table || !wpack || !status || !t || !xyz || !n_eval || !f_last) return -1;
    if ((uintptr_t)table & 7u) return -1;
    // the occupancy grid: a power-of-two edge of whole 8^3 blocks whose coarse bits fit the LDS table
    if (cascades < 1 || cascades > 8 || grid_size < 8 || grid_size > 1024 || (grid_size & (grid_size - 1))) return -1;
    const unsigned long long coarse_bits = ((unsigned long long)grid_size * grid_size * grid_size >> 9) * (unsigned long long)cascades;
    if (coarse_bits > 32ull * MARCH_MAX_COARSE_WORDS) return -1;
    if (!(eps >= 0.0f && eps < INFINITY) || !(step_scale > 0.0f && step_scale < INFINITY) || !(min_step >= 0.0f && min_step < INFINITY)) return -1;
    if (n_refine < 0 || n_refine > 64 || max_evals < 0 || max_evals > (1 << 20)) return -1;
    if (n_rays == 0) return 0;
    const XyzNorm nm = {1, -scale, scale};
    const MarchParams p = make_march_params(cascades, grid_size, scale, 0.0f);
    const SdfTraceParams tp = {eps, step_scale, min_step, n_refine, max_evals};
    long long blocks = ((long long)n_rays + SDF_BLOCK - 1) / SDF_BLOCK;               // a chunk of 64 rays per wave, or
    if (blocks > SDF_MAX_BLOCKS) blocks = SDF_MAX_BLOCKS;                            // a pool of chunks per wave of a full launch
#define SDF_TRACE_CALL(W, D)                                                                                                              \
    do {                                                                                                                                  \
        if (cascades == 1)                                                                                                                \
            hipLaunchKernelGGL((sdf_trace_kernel<W, D, true>), dim3((unsigned)blocks), dim3(SDF_BLOCK), 0, (hipStream_t)stream, rays_o, rays_d,     \
                               density_bitfield, coarse, table, *lv, wpack, nm, p, tp, n_rays, status, t, xyz, n_eval, f_last, stats);    \
        else                                                                                                                              \
            hipLaunchKernelGGL((sdf_trace_kernel<W, D, false>), dim3((unsigned)blocks), dim3(SDF_BLOCK), 0, (hipStream_t)stream, rays_o, rays_d,    \
                               density_bitfield, coarse, table, *lv, wpack, nm, p, tp, n_rays, status, t, xyz, n_eval, f_last, stats);    \
    } while (0)
    SDF_DISPATCH(SDF_TRACE_CALL);
#undef SDF_TRACE_CALL
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
