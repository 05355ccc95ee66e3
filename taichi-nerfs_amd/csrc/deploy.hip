// deploy.hip -- per-sample shading of the exported "deployment" model (train.py --deployment) for gfx950.
//
// Replaces, for inference from an exported model, hash_encode + sigma_rgb_layer of the reference's
// deployment/InstantNGP/taichi_ngp/kernels.py (:385-445, :449-518) with ONE launch: world position + direction in, (sigma, rgb) out.
//   x01 = xyz + 0.5; 4 dense levels x 8 corners, one 16-byte gather per corner (4 features), trilinear weights and the
//   mul-then-add accumulation of hash_fwd_f32_kernel<4>, through the same corner rule (hash_common.h: bit-identical embedding);
//   d / |d| -> (d + 1) / 2 -> the 16 SH terms of kernels.py:141-173, in that file's operation order (sh16_quad, ngp_device.h);
//   16 -> 16 (ReLU) -> 16, sigma = exp(out[0]);  [SH16 | 16] -> 16 (ReLU) -> 3, sigmoid; every sum runs over its inputs in index
//   order, as the reference's loops do.  All arithmetic is fp32.  The embedding and the SH terms are separate multiplies and adds
//   (the library is built with -ffp-contract=off; the embedding is checked bit for bit); the 1280 multiply-adds of the two networks
//   are explicit fmaf (one rounding instead of two: they are checked against a tolerance, profiles/PARITY_NOTES.md).
// Weight layout = what save_deployment_model writes: sigma_w[512] = W1 [16 out][16 in] | W2 [16 out][16 in];
// rgb_w[768] = W3 [16 out][32 in] | W4, the first 3 rows of a zero-padded [16][16].
//
// INDEXING.  kernels.py:427-431 forms the dense index x + y*res + z*res^2 and applies no modulo, so a corner at coordinate `res`
// reads the next level's rows, and on the last level past the table.  This kernel follows the TRAINING encoder instead (dense index
// modulo the level's entry count, hash_encoder.py:71, the level table of ngp_hash_levels_init): it equals the deployment kernel
// wherever that one stays inside its level, it is what the model was trained with, and every index is < map_size, so no position --
// inside the box, on its faces or outside -- reads out of bounds.
//
// One lane per sample, grid-stride.  The 1280 weights are read at compile-time offsets from wave-uniform pointers, so they arrive as
// scalar loads (s_load_dwordx16 through the scalar cache, 5 KB per wave and iteration) and feed v_fma_f32 as SGPR operands: no lane
// reads a weight from global memory and no LDS is used (an LDS copy read as broadcasts was tried first: the compiler hoisted the 1280
// loop-invariant reads into registers, 512 VGPRs and spills).  The 16-float embedding stays in registers.  The 45 MB table is the
// only per-sample memory traffic besides 24 B in and 16 B out: 32 gathers x 16 B = 512 B per sample.  175 VGPRs, no scratch: two
// waves per SIMD.
//
// deploy_render_kernel (ngp_deploy_render) renders whole rays with the same shading, one launch per frame: see the comment above it.
#include "ngp_device.h"
#include "hash_common.h"
#include "march_common.h"

namespace ngp {

struct DeployLevels {
    float scale[4];
    uint32_t res[4], size[4], offset[4];
};

__device__ __forceinline__ void deploy_sh16(float dx, float dy, float dz, float* __restrict__ sh) {
    const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float x = (dx / nrm + 1.0f) / 2.0f, y = (dy / nrm + 1.0f) / 2.0f, z = (dz / nrm + 1.0f) / 2.0f;
    const float4 q[4] = {sh16_quad<0>(x, y, z), sh16_quad<1>(x, y, z), sh16_quad<2>(x, y, z), sh16_quad<3>(x, y, z)};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        sh[4 * g] = q[g].x; sh[4 * g + 1] = q[g].y; sh[4 * g + 2] = q[g].z; sh[4 * g + 3] = q[g].w;
    }
}

// The shading of ONE sample, the only spelling of it in the library: world position xyz, direction d -> sigma, rgb and, where enc_out
// is given (wave-uniform), row i of it = the 16-float embedding.  deploy_shade_kernel (one lane per sample of a list) and
// deploy_render_kernel (one lane per slot of its wave) both inline it; sw / rw must be wave-uniform (kernel arguments), so that the
// weights arrive as scalar loads.  The embedding's store sits between the gathers and the networks on purpose: with nothing there the
// compiler hoists the 1280 weight loads out of the caller's sample loop and spills them (1036 SGPR spills, twice the instructions).
__device__ __forceinline__ void deploy_shade_point(const float xyz[3], const float d[3], const float* __restrict__ table, const DeployLevels& lv,
                                                   const float* __restrict__ sw, const float* __restrict__ rw, float* __restrict__ enc_out,
                                                   size_t i, float& sigma, float rgb[3]) {
    const float px = xyz[0] + 0.5f, py = xyz[1] + 0.5f, pz = xyz[2] + 0.5f;
    const float dx = d[0], dy = d[1], dz = d[2];

    // ---- embedding: 4 levels x 8 corners (the corner rule of hash_common.h on a dense level, F = 4)
    float in[32];                               // [SH16 | geometry feature]; the embedding lives in `enc` until the first layer is done
    float enc[16];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const uint32_t res = lv.res[l], size = lv.size[l], res2 = res * res;
        const float p[3] = {px, py, pz};
        uint32_t cell[3];
        float fr[3];
        cell_frac<false>(p, lv.scale[l], cell, fr);
        const float4* lt = reinterpret_cast<const float4*>(table) + lv.offset[l];
        float4 v[8];
        float w[8];
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) {
            // the training encoder's dense index `% map_size`: level_index(dense, mode 0) without the subtract in front of
            // the modulo (one branch per corner instead of two in a kernel at 175 VGPRs) -- the same value for every
            // input, always < size, whatever the position and whatever table the caller hands over
            uint32_t h = (cell[0] + (ci & 1)) + (cell[1] + ((ci >> 1) & 1)) * res + (cell[2] + (ci >> 2)) * res2;
            if (h >= size) h %= size;
            v[ci] = lt[h];
            w[ci] = corner_weight(ci, fr);
        }
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
        for (int ci = 0; ci < 8; ++ci) {
            a0 += w[ci] * v[ci].x; a1 += w[ci] * v[ci].y; a2 += w[ci] * v[ci].z; a3 += w[ci] * v[ci].w;
        }
        enc[4 * l] = a0; enc[4 * l + 1] = a1; enc[4 * l + 2] = a2; enc[4 * l + 3] = a3;
    }
    if (enc_out) {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            reinterpret_cast<float4*>(enc_out)[4 * i + l] = make_float4(enc[4 * l], enc[4 * l + 1], enc[4 * l + 2], enc[4 * l + 3]);
    }

    // ---- density network: 16 -> 16 (ReLU) -> 16
    deploy_sh16(dx, dy, dz, in);
#pragma unroll
    for (int j = 0; j < 16; ++j) in[16 + j] = 0.0f;
#pragma unroll
    for (int o = 0; o < 16; ++o) {
        float t = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) t = fmaf(enc[j], sw[o * 16 + j], t);
        t = fmaxf(0.0f, t);
#pragma unroll
        for (int j = 0; j < 16; ++j) in[16 + j] = fmaf(t, sw[256 + j * 16 + o], in[16 + j]);
    }
    // ---- colour network: [SH16 | 16] -> 16 (ReLU) -> 3
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int o = 0; o < 16; ++o) {
        float t = 0.0f;
#pragma unroll
        for (int j = 0; j < 32; ++j) t = fmaf(in[j], rw[o * 32 + j], t);
        t = fmaxf(0.0f, t);
        s0 = fmaf(t, rw[512 + o], s0);
        s1 = fmaf(t, rw[512 + 16 + o], s1);
        s2 = fmaf(t, rw[512 + 32 + o], s2);
    }
    sigma = expf(in[16]);
    rgb[0] = 1.0f / (1.0f + expf(-s0));
    rgb[1] = 1.0f / (1.0f + expf(-s1));
    rgb[2] = 1.0f / (1.0f + expf(-s2));
}

__global__ void __launch_bounds__(256) deploy_shade_kernel(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                           const float* __restrict__ table, DeployLevels lv,
                                                           const float* __restrict__ sigma_w, const float* __restrict__ rgb_w, int n,
                                                           float* __restrict__ sigmas, float* __restrict__ rgbs,
                                                           float* __restrict__ enc_out) {
    const float* __restrict__ sw = sigma_w;    // wave-uniform addresses at compile-time offsets: scalar loads, SGPR operands
    const float* __restrict__ rw = rgb_w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float p[3] = {xyzs[3 * (size_t)i], xyzs[3 * (size_t)i + 1], xyzs[3 * (size_t)i + 2]};
        const float d[3] = {dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]};
        float sigma, rgb[3];
        deploy_shade_point(p, d, table, lv, sw, rw, enc_out, (size_t)i, sigma, rgb);
        sigmas[i] = sigma;
        rgbs[3 * (size_t)i] = rgb[0];
        rgbs[3 * (size_t)i + 1] = rgb[1];
        rgbs[3 * (size_t)i + 2] = rgb[2];
    }
}

// ---- a whole ray in one launch: slab test, occupancy march, shading, front-to-back compositing ------------------------------------
// One lane OWNS a ray, 64 consecutive rays per wave, one wave per block.  Per ray (scale 0.5, one cascade, grid 128, constant step):
//   (t1, t2) = ray_aabb_slab; the orbit t_{k+1} = t_k + dt from t1 and the examined / skipped / emitted rule of ray_march.py:46-74
//   with zero jitter (the sample sequence of ngp_march_train, bit for bit); the emitted samples are shaded and composited in order by
//   the serial loop of volume_train.py:34-48, and the march of the ray ends when T <= T_threshold, at max_samples samples or at t2.
// The wave repeats until no ray is alive:
//   search     -- only when some alive ray has no sample queued: every owner walks its orbit on, DEPLOY_BATCH speculative points per
//                 iteration as in march_test_kernel (march.hip), the coarse 8^3-block bits in LDS answering most of them without a
//                 global load, until DEPLOY_QUEUE sample positions wait in its LDS queue or its orbit has left the box.  The walk
//                 through empty space is a chain of dependent probes, and the wave waits for its slowest lane: queueing ahead
//                 makes that wait once per DEPLOY_QUEUE samples instead of once per sample;
//   share      -- the L rays that hold queued samples share the wave's 64 slots, q = 64 / L of their next samples each;
//   shade      -- lane i shades slot i (deploy_shade_point on the owner's ray, fetched by shuffles) and leaves (sigma, rgb) there;
//   composite  -- the owner composites its slots in sample order and stops at T <= T_threshold; what was queued or shaded behind that
//                 point is dropped.
// While all 64 rays are alive this is one sample per ray and round; when few are left the idle lanes shade those rays' next samples.
// The shading of a sample does not depend on the lane that computes it and the owner alone accumulates, in sample order: every
// output is a function of its ray.  Nothing per sample leaves the wave's LDS, nothing is read back, no atomic is used.
constexpr int DEPLOY_BATCH = 16;                 // orbit points probed speculatively per search step (march_test_kernel: ORBIT_BATCH = 8)
constexpr int DEPLOY_QUEUE = 32;                 // sample positions a ray queues ahead (a power of two: the queue is a ring)

__global__ void __launch_bounds__(64) deploy_render_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                           const uint8_t* __restrict__ bits, const uint32_t* __restrict__ coarse,
                                                           const float* __restrict__ table, DeployLevels lv,
                                                           const float* __restrict__ sigma_w, const float* __restrict__ rgb_w,
                                                           MarchParams p, int n_rays, int max_samples, float T_threshold,
                                                           float* __restrict__ rgb_out, float* __restrict__ opacity_out,
                                                           float* __restrict__ depth_out, int32_t* __restrict__ n_out,
                                                           float* __restrict__ t_last_out) {
    static_assert((DEPLOY_QUEUE & (DEPLOY_QUEUE - 1)) == 0, "the queue index wraps with a mask");
    __shared__ uint32_t coarse_s[MARCH_MAX_COARSE_WORDS];
    __shared__ float q_buf[DEPLOY_QUEUE][64];    // [ring position][owner lane] -> t of a queued sample
    __shared__ float q_t[64];                    // slot -> t of the sample
    __shared__ int q_owner[64];                  // slot -> owning lane, -1 = empty
    __shared__ float4 q_res[64];                 // slot -> (sigma, r, g, b)
    const bool use_coarse = load_coarse(p, coarse, coarse_s);
    const float* __restrict__ sw = sigma_w;
    const float* __restrict__ rw = rgb_w;
    const int lane = threadIdx.x;
    const long long r = (long long)blockIdx.x * 64 + lane;
    const bool has_ray = r < (long long)n_rays;
    const size_t rr = has_ray ? (size_t)r : 0;
    float o[3], d[3], d_inv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = rays_o[3 * rr + k]; d[k] = rays_d[3 * rr + k]; d_inv[k] = 1.0f / d[k]; }
    const float2 h = ray_aabb_slab(o, d_inv, p.scale);
    const float t2 = h.y;
    const float dt = calc_dt(0.0f, p.esf, p.dt_min, p.dt_max);                      // the step when exp_step_factor == 0
    float t = h.x;                                                                  // next orbit point (zero jitter: the orbit starts at t1)
    float t_target = -INFINITY;                                                     // orbit points below this are skipped
    float T = 1.0f, acc[3] = {0.0f, 0.0f, 0.0f}, dep = 0.0f, op = 0.0f, t_last = 0.0f;
    int n = 0, qh = 0, qn = 0;                                                      // composited samples; queue head and length
    bool live = has_ray && (n < max_samples) && (T > T_threshold);                  // volume_train.py:38 and the cap
    // ray_march.py:46.  A ray without a direction (d = 0 from inside the box: t2 = inf) would never leave: a miss.
    bool exhausted = !((0.0f <= t) && (t < t2) && (t2 < INFINITY));                 // the orbit has left the box
    for (;;) {
        const bool active = live && (qn > 0 || !exhausted);
        if (!__any(active)) break;
        if (__any(active && qn == 0)) {
            // ---- search: top the queue up; n + qn never exceeds max_samples
            const int room = min(DEPLOY_QUEUE, max_samples - n) - qn;
            int found = 0;
            bool searching = active && !exhausted && room > 0;
            while (searching) {
                float tb[DEPLOY_BATCH];
                bool ob[DEPLOY_BATCH];
                float tt = t;
#pragma unroll
                for (int u = 0; u < DEPLOY_BATCH; ++u) {
                    CellProbe c;
                    probe_cell<true>(p, o, d, tt, dt, c);
                    tb[u] = tt;
                    bool occ = true;
                    if (use_coarse) { const uint32_t cb = c.idx >> 9; occ = (coarse_s[cb >> 5] >> (cb & 31u)) & 1u; }
                    if (occ) occ = (bits[c.idx >> 3] >> (c.idx & 7u)) & 1u;          // ray_march.py:60-61
                    ob[u] = occ;
                    tt += dt;
                }
#pragma unroll
                for (int u = 0; u < DEPLOY_BATCH; ++u) {
                    if (!searching) break;
                    const float tu = tb[u];
                    if (!(tu < t2)) { exhausted = true; searching = false; break; }  // the orbit left the box
                    if (tu < t_target) continue;                                     // inside the running skip
                    if (ob[u]) {                                                     // emitted: ray_march.py:63-65
                        q_buf[(qh + qn) & (DEPLOY_QUEUE - 1)][lane] = tu;
                        qn += 1; found += 1;
                        t_target = -INFINITY;
                        if (found == room) { t = tu + dt; searching = false; }       // resume at the next orbit point
                    } else {
                        CellProbe c;
                        probe_cell<true>(p, o, d, tu, dt, c);
                        t_target = skip_target(p, d, d_inv, tu, c);                  // ray_march.py:68-71
                    }
                }
                if (searching) {
                    if (!(tt > t)) { exhausted = true; searching = false; }          // t so large that t + dt == t: the orbit has stopped
                    t = tt;
                }
            }
        }
        // ---- share: the rays that hold queued samples divide the 64 slots
        const bool has = live && qn > 0;
        const unsigned long long lm = __ballot(has);
        if (lm == 0ull) continue;                                                   // wave-uniform: the starved rays found nothing more
        const int quota = 64 / __popcll(lm);
        const int base = __popcll(lm & ((1ull << lane) - 1ull)) * quota;            // this ray's first slot: base + quota <= 64
        const int take = has ? min(quota, qn) : 0;
        q_owner[lane] = -1;
        wave_sync_lds();
        for (int j = 0; j < take; ++j) { q_owner[base + j] = lane; q_t[base + j] = q_buf[(qh + j) & (DEPLOY_QUEUE - 1)][lane]; }
        wave_sync_lds();
        // ---- shade: lane i takes slot i; the owner's ray comes by shuffle (all lanes take part: a shuffle reads active lanes only)
        const int ow = q_owner[lane];
        const int src = ow < 0 ? lane : ow;
        float so[3], sd[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { so[k] = __shfl(o[k], src); sd[k] = __shfl(d[k], src); }
        if (ow >= 0) {
            const float ts = q_t[lane];
            const float xyz[3] = {so[0] + ts * sd[0], so[1] + ts * sd[1], so[2] + ts * sd[2]};   // ray_march.py:88
            float sigma, c[3];
            deploy_shade_point(xyz, sd, table, lv, sw, rw, nullptr, 0, sigma, c);
            q_res[lane] = make_float4(sigma, c[0], c[1], c[2]);
        }
        wave_sync_lds();
        // ---- composite (volume_train.py:38-48): the owner, its slots in sample order
        for (int j = 0; j < take; ++j) {
            if (!(T > T_threshold)) break;
            const float4 s = q_res[base + j];
            const float ts = q_t[base + j];
            const float a = 1.0f - expf(-s.x * dt);
            const float w = a * T;
            acc[0] += w * s.y; acc[1] += w * s.z; acc[2] += w * s.w;
            dep += w * ts; op += w;
            T = T * (1.0f - a);
            n += 1;
            t_last = ts;
        }
        qh += take; qn -= take;
        live = live && (n < max_samples) && (T > T_threshold);
        wave_sync_lds();                                                            // the slots are reused by the next round
    }
    if (has_ray) {
        rgb_out[3 * rr] = acc[0]; rgb_out[3 * rr + 1] = acc[1]; rgb_out[3 * rr + 2] = acc[2];
        opacity_out[rr] = op; depth_out[rr] = dep; n_out[rr] = n; t_last_out[rr] = t_last;
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" {

// the four dense float4 levels of the deployment model, or false
static bool deploy_levels(const ngp_hash_levels* lv, DeployLevels& dl) {
    if (!lv || lv->n_levels != 4 || lv->n_features != 4 || lv->begin_fast_hash_level != 4) return false;   // four dense levels of float4 rows
    for (int l = 0; l < 4; ++l) {
        if (lv->map_size[l] == 0 || (uint64_t)lv->offset[l] + lv->map_size[l] > (uint64_t)lv->total_entries) return false;
        dl.scale[l] = lv->scale[l]; dl.res[l] = lv->resolution[l]; dl.size[l] = lv->map_size[l]; dl.offset[l] = lv->offset[l];
    }
    return true;
}

int ngp_deploy_shade(const float* xyzs, const float* dirs, const float* table, const ngp_hash_levels* lv, const float* sigma_w,
                     const float* rgb_w, int n, float* sigmas, float* rgbs, float* enc_out, void* stream) {
    if (n <= 0) return 0;
    DeployLevels dl;
    if (!deploy_levels(lv, dl)) return -1;
    if (!xyzs || !dirs || !table || !sigma_w || !rgb_w || !sigmas || !rgbs) return -1;
    if (((uintptr_t)table & 15u) || ((uintptr_t)enc_out & 15u)) return -1;                                // 16-byte gathers / stores
    int blocks = (n + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(deploy_shade_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, xyzs, dirs, table, dl, sigma_w, rgb_w, n,
                       sigmas, rgbs, enc_out);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_deploy_render(const float* rays_o, const float* rays_d, const uint8_t* density_bitfield, const uint32_t* coarse,
                      const float* table, const ngp_hash_levels* lv, const float* sigma_w, const float* rgb_w, int n_rays,
                      int max_samples, float T_threshold, float* rgb, float* opacity, float* depth, int32_t* n_samples, float* t_last,
                      void* stream) {
    if (n_rays <= 0) return 0;
    DeployLevels dl;
    if (!deploy_levels(lv, dl) || max_samples < 1) return -1;
    if (!rays_o || !rays_d || !density_bitfield || !table || !sigma_w || !rgb_w || !rgb || !opacity || !depth || !n_samples || !t_last)
        return -1;
    if ((uintptr_t)table & 15u) return -1;                                                                 // 16-byte gathers
    const MarchParams p = make_march_params(1, 128, 0.5f, 0.0f);             // the one occupancy shape a deployment model has
    hipLaunchKernelGGL(deploy_render_kernel, dim3((n_rays + 63) / 64), dim3(64), 0, (hipStream_t)stream, rays_o, rays_d, density_bitfield,
                       coarse, table, dl, sigma_w, rgb_w, p, n_rays, max_samples, T_threshold, rgb, opacity, depth, n_samples, t_last);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
