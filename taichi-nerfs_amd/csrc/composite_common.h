// composite_common.h -- the ray-side rules of the compositors, shared by composite.hip (volume compositor) and surface.hip (NeuS
// opacity).  One definition each: the 64-sample group step, the colour load / colour-gradient store and the closed-form backward
// walk of the volume compositor.  A kernel that composites a ray one wave per ray includes this header and calls these.  (The
// forward walk of the volume compositor stays written out in composite.hip's two kernels around group_step: see there.)
#pragma once
#include "ngp_device.h"
#include <hip/hip_fp16.h>

namespace ngp {

template <bool HALF>
__device__ __forceinline__ void load_rgb(const void* rgbs, size_t s, float c[3]) {
    if (HALF) {
        const __half* p = (const __half*)rgbs + 3 * s;
        c[0] = __half2float(p[0]); c[1] = __half2float(p[1]); c[2] = __half2float(p[2]);
    } else {
        const float* p = (const float*)rgbs + 3 * s;
        c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
    }
}

// the colour gradient of sample s, in the colours' own format
template <bool HALF>
__device__ __forceinline__ void store_rgb(void* d_rgbs, size_t s, float c0, float c1, float c2) {
    if (HALF) { __half* p = (__half*)d_rgbs + 3 * s; p[0] = __float2half(c0); p[1] = __float2half(c1); p[2] = __float2half(c2); }
    else { float* p = (float*)d_rgbs + 3 * s; p[0] = c0; p[1] = c1; p[2] = c2; }
}

// ---- the 64-sample group step ------------------------------------------------------------------------------------------------------
// T = transmittance entering the group (wave-uniform), a = this lane's opacity (0 on a lane without a sample).
struct GroupScan {
    float incl;               // prod_{i<=lane} (1 - a_i)
    float Ts;                 // T before this lane's sample
};

__device__ __forceinline__ GroupScan group_scan(float T, float a, int lane) {
    GroupScan g;
    g.incl = wave_scan_mul(1.0f - a, lane);
    float excl = __shfl_up(g.incl, 1, NGP_WAVE);
    if (lane == 0) excl = 1.0f;
    g.Ts = T * excl;
    return g;
}

struct GroupStep {
    float incl, Ts;
    uint64_t deadm;           // lanes whose sample lies at or behind early termination
    bool live;
    float w;                  // a * Ts on a live lane, else 0
};

// One group of a ray; T is carried on to the next group.
__device__ __forceinline__ GroupStep group_step(float T, float a, bool valid, float thr, int lane) {
    const GroupScan sc = group_scan(T, a, lane);
    GroupStep g;
    g.incl = sc.incl; g.Ts = sc.Ts;
    // liveness as a PREFIX by construction: the Kogge-Stone product is not guaranteed monotone to the last ulp, and the consumers of
    // the live count (ngp_live_compact, the fused live list, the backward sweeps of both compositors) take the live samples of a ray
    // to be exactly its first `count` ones
    g.deadm = __ballot(valid && !(g.Ts > thr));
    g.live = valid && (g.deadm == 0 || lane < __builtin_ctzll(g.deadm));
    g.w = g.live ? a * g.Ts : 0.0f;
    return g;
}
__device__ __forceinline__ float group_carry(float T, const GroupStep& g) {
    return g.deadm ? 0.0f : T * __shfl(g.incl, NGP_WAVE - 1, NGP_WAVE);    // a dead sample in this group ends the ray for good
}

// ---- closed-form backward walk ------------------------------------------------------------------------------
//   dL/dc_s     = g_rgb * w_s
//   dL/dsigma_s = delta_s * [ g_rgb.(c_s T+ - (R - rbar_s)) + g_dep (t_s T+ - (D - dbar_s)) + g_op (1 - O)
//                             + g_ws[s] T+ - (W - wbar_s) ]
// with T+ = T_s (1 - a_s), bars = inclusive prefix sums, R/D/O the forward outputs, W = sum_s g_ws[s] w_s.
// FULL = false: the form with g_dep = g_ws = 0, in which the depth and g_ws terms are absent (not multiplied by zero): ts, g_ws,
// g.gd, tot.D and tot.W are then never read, whatever the caller passes.
struct RayTotals {
    float R0, R1, R2, D, O, W;
};
struct RayCotangents {
    float gr0, gr1, gr2, gd, go;      // go: g_op plus the background blend's share
};

template <bool HALF, bool FULL>
__device__ __forceinline__ void composite_backward_walk(const float* __restrict__ sigmas, const void* __restrict__ rgbs,
                                                        const float* __restrict__ deltas, const float* __restrict__ ts,
                                                        const float* __restrict__ g_ws, float* __restrict__ d_sigmas,
                                                        void* __restrict__ d_rgbs, int start, int N, float thr, int lane,
                                                        const RayCotangents g, const RayTotals tot) {
    float T = 1.0f;
    float cr0 = 0.f, cr1 = 0.f, cr2 = 0.f, cd = 0.f, cw = 0.f;     // carries of the inclusive prefix sums
    for (int base = 0; base < N; base += NGP_WAVE) {
        const int j = base + lane;
        const bool valid = j < N;
        const size_t s = (size_t)start + j;
        if (!(T > thr)) {
            if (valid) {
                d_sigmas[s] = 0.0f;
                store_rgb<HALF>(d_rgbs, s, 0.0f, 0.0f, 0.0f);
            }
            continue;
        }
        float a = 0.0f, tm = 0.0f, dl = 0.0f, gw = 0.0f, c[3] = {0.f, 0.f, 0.f};
        if (valid) {
            dl = deltas[s];
            a = 1.0f - expf(-sigmas[s] * dl);
            if (FULL) tm = ts[s];
            load_rgb<HALF>(rgbs, s, c);
            if (FULL && g_ws) gw = g_ws[s];
        }
        const GroupStep st = group_step(T, a, valid, thr, lane);
        const float w = st.w;
        const float Tp = st.Ts * (1.0f - a);
        const float p0 = cr0 + wave_scan_add(w * c[0], lane);
        const float p1 = cr1 + wave_scan_add(w * c[1], lane);
        const float p2 = cr2 + wave_scan_add(w * c[2], lane);
        float pd = 0.0f, pw = 0.0f;
        if (FULL) pd = cd + wave_scan_add(w * tm, lane);
        if (FULL && g_ws) pw = cw + wave_scan_add(gw * w, lane);
        if (valid) {
            float ds = 0.0f, dc0 = 0.0f, dc1 = 0.0f, dc2 = 0.0f;
            if (st.live) {
                float acc = g.gr0 * (c[0] * Tp - (tot.R0 - p0)) + g.gr1 * (c[1] * Tp - (tot.R1 - p1)) + g.gr2 * (c[2] * Tp - (tot.R2 - p2));
                if (FULL) acc += g.gd * (tm * Tp - (tot.D - pd));
                acc += g.go * (1.0f - tot.O);
                if (FULL) acc += gw * Tp - (tot.W - pw);
                ds = dl * acc;
                dc0 = g.gr0 * w; dc1 = g.gr1 * w; dc2 = g.gr2 * w;
            }
            d_sigmas[s] = ds;
            // store_rgb<HALF>(d_rgbs, s, dc0, dc1, dc2), spelled out: through the function the compiler pairs the three fp16
            // conversions of composite_bwd_kernel<true> differently, and a product of -0 then leaves with another sign
            if (HALF) { __half* p = (__half*)d_rgbs + 3 * s; p[0] = __float2half(dc0); p[1] = __float2half(dc1); p[2] = __float2half(dc2); }
            else { float* p = (float*)d_rgbs + 3 * s; p[0] = dc0; p[1] = dc1; p[2] = dc2; }
        }
        cr0 = __shfl(p0, NGP_WAVE - 1, NGP_WAVE); cr1 = __shfl(p1, NGP_WAVE - 1, NGP_WAVE); cr2 = __shfl(p2, NGP_WAVE - 1, NGP_WAVE);
        if (FULL) cd = __shfl(pd, NGP_WAVE - 1, NGP_WAVE);
        if (FULL && g_ws) cw = __shfl(pw, NGP_WAVE - 1, NGP_WAVE);
        T = group_carry(T, st);
    }
}

}  // namespace ngp
