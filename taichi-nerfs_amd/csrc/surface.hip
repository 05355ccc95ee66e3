// surface.hip -- volume-render compositing driven by a signed distance (NeuS opacity), forward and backward, for gfx950.
//
// The compositor of composite.hip with another per-sample opacity: instead of a = 1 - exp(-sigma delta) the opacity comes from the
// signed distance f of the sample, its directional derivative c = dir . grad f and ONE global sharpness s (the inverse standard
// deviation of the logistic density, a learnable scalar read from device memory):
//
//     ic = -( relu(-c/2 + 1/2) (1 - r) + relu(-c) r )          r: cosine anneal ratio in [0, 1]
//     h  = ic delta / 2
//     p  = sigmoid((f - h) s),  n = sigmoid((f + h) s)
//     a  = clip( (p - n + 1e-5) / (p + 1e-5), 0, 1 )
//
// and then the loop of composite.hip unchanged (T = 1; stop at the first !(T > thr); w = a T; ...; T <- T (1 - a)).
//
// Shape: one 64-lane wave owns a ray, 64 consecutive samples are loaded coalesced, transmittance is a multiplicative wave scan with a
// per-ray carry, liveness is a prefix (ballot + ctz), a group is skipped when T <= thr at its start.  That 64-sample group step is
// composite.hip's own, defined once in composite_common.h: the forward calls group_step, the backward's sweep takes its first half,
// group_scan.  The forward keeps its own ray walk (another opacity source, the aux accumulators, the alphas store).  The backward is the REVERSE
// SWEEP of the loop (the adjoint X of the transmittance behind a sample obeys X_{j-1} = G_j a_j + (1 - a_j) X_j), not the closed
// form `total - prefix` of composite.hip: that form divides by 1 - a_j, and a NeuS opacity is exactly 1 as soon as a ray starts
// inside the surface.  The sweep runs the 64-sample groups of a ray last to first; inside a group the recurrence is a suffix scan
// of affine maps across the lanes.  The transmittance at the start of every group comes from a first, forward pass over the stored
// opacities (one float per sample), kept one group per lane.
//
// No atomics in either launch: the gradient of s is a per-ray wave reduction into a [n_rays] workspace in rays_a row order, summed
// by one block in a fixed order -- the same inputs give the same bits.
//
// Held, element by element, to the float64 model of tests/surface_reference.py within 4x the error of a serial float32 evaluation
// (tests/test_gpu_surface.py).
#include "ngp_device.h"
#include "composite_common.h"

namespace ngp {

constexpr float SURF_EPS = 1e-5f;

// relu that lets a NaN through (fmaxf would swallow it: a NaN input has to poison its ray, not vanish)
__device__ __forceinline__ float relu_nan(float x) { return x < 0.0f ? 0.0f : x; }
// 1 / (1 + exp(-x)): exp(-x) = inf gives 1 / inf = 0, never inf / inf
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

struct SurfAlpha {
    float a, p, n, h, v;      // v: the opacity before the clip
};

__device__ __forceinline__ SurfAlpha surf_alpha(float f, float c, float dl, float s, float r) {
    SurfAlpha o;
    const float ic = -(relu_nan(-c * 0.5f + 0.5f) * (1.0f - r) + relu_nan(-c) * r);
    o.h = ic * dl * 0.5f;
    o.p = sigmoid_f((f - o.h) * s);
    o.n = sigmoid_f((f + o.h) * s);
    o.v = (o.p - o.n + SURF_EPS) / (o.p + SURF_EPS);
    o.a = o.v < 0.0f ? 0.0f : (o.v > 1.0f ? 1.0f : o.v);       // (a NaN stays a NaN)
    return o;
}

__global__ void __launch_bounds__(256) surface_fwd_kernel(const float* __restrict__ sdf, const float* __restrict__ cosv,
                                                          const float* __restrict__ rgbs, const float* __restrict__ aux,
                                                          const float* __restrict__ deltas, const float* __restrict__ ts,
                                                          const int32_t* __restrict__ rays_a, const float* __restrict__ inv_s, float r,
                                                          float thr, int n_rays, float bg, int32_t* __restrict__ total_samples,
                                                          float* __restrict__ opacity, float* __restrict__ depth, float* __restrict__ rgb,
                                                          float* __restrict__ rgb_out, float* __restrict__ aux_out, float* __restrict__ ws,
                                                          float* __restrict__ alphas) {
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= n_rays) return;
    const int lane = lane_id();
    const int ray_idx = rays_a[3 * n], start = rays_a[3 * n + 1], N = rays_a[3 * n + 2];
    const float s = inv_s[0];
    float T = 1.0f;                       // transmittance entering the current group (wave-uniform)
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, x0 = 0.f, x1 = 0.f, x2 = 0.f, dep = 0.f, op = 0.f;
    int cnt = 0;
    for (int base = 0; base < N; base += NGP_WAVE) {
        const int j = base + lane;
        const bool valid = j < N;
        const size_t k = (size_t)start + j;
        if (!(T > thr)) {                 // everything from here on is behind early termination
            if (valid) { ws[k] = 0.0f; alphas[k] = 0.0f; }
            continue;
        }
        float a = 0.0f, tm = 0.0f, c[3] = {0.f, 0.f, 0.f}, x[3] = {0.f, 0.f, 0.f};
        if (valid) {
            a = surf_alpha(sdf[k], cosv[k], deltas[k], s, r).a;
            tm = ts[k];
            c[0] = rgbs[3 * k]; c[1] = rgbs[3 * k + 1]; c[2] = rgbs[3 * k + 2];
            if (aux) { x[0] = aux[3 * k]; x[1] = aux[3 * k + 1]; x[2] = aux[3 * k + 2]; }
        }
        const GroupStep g = group_step(T, a, valid, thr, lane);          // the live samples are a prefix: the backward relies on it
        const float w = g.w;
        if (valid) { ws[k] = w; alphas[k] = g.live ? a : 0.0f; }
        r0 += w * c[0]; r1 += w * c[1]; r2 += w * c[2];
        x0 += w * x[0]; x1 += w * x[1]; x2 += w * x[2];
        dep += w * tm; op += w;
        cnt += g.live ? 1 : 0;
        T = group_carry(T, g);
    }
    r0 = wave_sum(r0); r1 = wave_sum(r1); r2 = wave_sum(r2);
    dep = wave_sum(dep); op = wave_sum(op); cnt = wave_sum_i(cnt);
    if (aux_out) { x0 = wave_sum(x0); x1 = wave_sum(x1); x2 = wave_sum(x2); }
    if (lane == 0) {
        rgb[3 * ray_idx] = r0; rgb[3 * ray_idx + 1] = r1; rgb[3 * ray_idx + 2] = r2;
        depth[ray_idx] = dep; opacity[ray_idx] = op; total_samples[ray_idx] = cnt;
        if (rgb_out) {
            const float b = bg * (1.0f - op);
            rgb_out[3 * ray_idx] = r0 + b; rgb_out[3 * ray_idx + 1] = r1 + b; rgb_out[3 * ray_idx + 2] = r2 + b;
        }
        if (aux_out) { aux_out[3 * ray_idx] = x0; aux_out[3 * ray_idx + 1] = x1; aux_out[3 * ray_idx + 2] = x2; }
    }
}

// Suffix scan of affine maps m_j(X) = B_j + A_j X across the 64 lanes: on return lane j holds m_j o m_{j+1} o ... o m_63.
__device__ __forceinline__ void wave_suffix_affine(float& A, float& B, int lane) {
#pragma unroll
    for (int d = 1; d < NGP_WAVE; d <<= 1) {
        const float Ao = __shfl_down(A, d, NGP_WAVE), Bo = __shfl_down(B, d, NGP_WAVE);
        if (lane + d < NGP_WAVE) { B = B + A * Bo; A = A * Ao; }
    }
}

__global__ void __launch_bounds__(256) surface_bwd_kernel(const float* __restrict__ g_op, const float* __restrict__ g_dep,
                                                          const float* __restrict__ g_rgb, const float* __restrict__ g_aux,
                                                          const float* __restrict__ g_ws, const float* __restrict__ sdf,
                                                          const float* __restrict__ cosv, const float* __restrict__ rgbs,
                                                          const float* __restrict__ aux, const float* __restrict__ deltas,
                                                          const float* __restrict__ ts, const int32_t* __restrict__ rays_a,
                                                          const float* __restrict__ inv_s, float r, int n_rays, float bg,
                                                          const int32_t* __restrict__ total_samples, const float* __restrict__ alphas,
                                                          float* __restrict__ d_sdf, float* __restrict__ d_cos, float* __restrict__ d_rgbs,
                                                          float* __restrict__ d_aux, float* __restrict__ ds_rows) {
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= n_rays) return;
    const int lane = lane_id();
    const int ray_idx = rays_a[3 * n], start = rays_a[3 * n + 1], N = rays_a[3 * n + 2];
    int M = total_samples[ray_idx];                                      // the forward's live count: the first M samples
    M = M < 0 ? 0 : (M > N ? N : M);
    const float s = inv_s[0];
    const float gr0 = g_rgb[3 * ray_idx], gr1 = g_rgb[3 * ray_idx + 1], gr2 = g_rgb[3 * ray_idx + 2];
    const bool has_aux = aux && g_aux;
    const float ga0 = has_aux ? g_aux[3 * ray_idx] : 0.0f, ga1 = has_aux ? g_aux[3 * ray_idx + 1] : 0.0f,
                ga2 = has_aux ? g_aux[3 * ray_idx + 2] : 0.0f;
    // g_rgb is the gradient of the BLENDED colour rgb + bg (1 - opacity) when bg != 0: the blend's share of d opacity is -bg sum_c g_rgb
    const float gd = g_dep ? g_dep[ray_idx] : 0.0f, go = (g_op ? g_op[ray_idx] : 0.0f) + (bg != 0.0f ? -bg * (gr0 + gr1 + gr2) : 0.0f);
    // samples behind the live count: exact zeros
    for (int j = (M & ~(NGP_WAVE - 1)) + lane; j < N; j += NGP_WAVE) {
        if (j < M) continue;
        const size_t k = (size_t)start + j;
        d_sdf[k] = 0.0f; d_cos[k] = 0.0f;
        d_rgbs[3 * k] = 0.0f; d_rgbs[3 * k + 1] = 0.0f; d_rgbs[3 * k + 2] = 0.0f;
        if (d_aux) { d_aux[3 * k] = 0.0f; d_aux[3 * k + 1] = 0.0f; d_aux[3 * k + 2] = 0.0f; }
    }
    const int n_groups = (M + NGP_WAVE - 1) / NGP_WAVE;
    float X = 0.0f;                        // adjoint of the transmittance behind the sample being processed (wave-uniform carry)
    float ds = 0.0f;                       // this lane's share of dL/ds
    // 64 groups at a time (one transmittance per lane), the blocks of 64 groups last to first; a ray of up to 4096 live samples is
    // one block, a longer one repeats the forward pass per block
    for (int blk = (n_groups - 1) / NGP_WAVE; blk >= 0 && n_groups > 0; --blk) {
        const int g_lo = blk * NGP_WAVE, g_hi = min(n_groups, g_lo + NGP_WAVE);
        // pass 1: the transmittance entering each group of this block, from the stored opacities
        float T = 1.0f, T_start = 0.0f;
        for (int g = 0; g < g_hi; ++g) {
            if (g >= g_lo && lane == g - g_lo) T_start = T;
            if (g + 1 < g_hi) {
                const int j = g * NGP_WAVE + lane;
                const float q = j < M ? 1.0f - alphas[(size_t)start + j] : 1.0f;
                T = T * __shfl(wave_scan_mul(q, lane), NGP_WAVE - 1, NGP_WAVE);
            }
        }
        // pass 2: the reverse sweep
        for (int g = g_hi - 1; g >= g_lo; --g) {
            const int j = g * NGP_WAVE + lane;
            const bool live = j < M;
            const size_t k = (size_t)start + j;
            const float Tg = __shfl(T_start, g - g_lo, NGP_WAVE);
            float f = 0.0f, c = 0.0f, dl = 0.0f, tm = 0.0f, gw = 0.0f, col[3] = {0.f, 0.f, 0.f}, x[3] = {0.f, 0.f, 0.f};
            SurfAlpha al = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (live) {
                f = sdf[k]; c = cosv[k]; dl = deltas[k]; tm = ts[k];
                al = surf_alpha(f, c, dl, s, r);
                col[0] = rgbs[3 * k]; col[1] = rgbs[3 * k + 1]; col[2] = rgbs[3 * k + 2];
                if (has_aux) { x[0] = aux[3 * k]; x[1] = aux[3 * k + 1]; x[2] = aux[3 * k + 2]; }
                if (g_ws) gw = g_ws[k];
            }
            const float a = al.a, q = 1.0f - a;
            const float Ts = group_scan(Tg, a, lane).Ts;                             // T before this sample
            // cotangent of w_j
            float G = (gr0 * col[0] + gr1 * col[1]) + gr2 * col[2];
            G += (ga0 * x[0] + ga1 * x[1]) + ga2 * x[2];
            G += gd * tm;
            G += go;
            G += gw;
            float A = live ? q : 1.0f, B = live ? G * a : 0.0f;
            wave_suffix_affine(A, B, lane);
            float An = __shfl_down(A, 1, NGP_WAVE), Bn = __shfl_down(B, 1, NGP_WAVE);
            if (lane == NGP_WAVE - 1) { An = 1.0f; Bn = 0.0f; }
            const float Xj = Bn + An * X;                                            // adjoint of T behind sample j
            if (live) {
                const float da = Ts * (G - Xj);                                      // dL/da_j
                const float w = a * Ts;
                float dadf = 0.0f, dadc = 0.0f, dads = 0.0f;
                if (!(al.v < 0.0f) && !(al.v > 1.0f)) {
                    const float pp = al.p * (1.0f - al.p), nn = al.n * (1.0f - al.n), den = al.p + SURF_EPS;
                    const float ppa = pp * (1.0f - a);
                    dadf = s * (ppa - nn) / den;
                    const float dadh = -s * (ppa + nn) / den;
                    const float ind = (1.0f - r) * 0.5f * ((-c * 0.5f + 0.5f) > 0.0f ? 1.0f : 0.0f) + r * (-c > 0.0f ? 1.0f : 0.0f);
                    dadc = dadh * (dl * 0.5f) * ind;
                    dads = ((f - al.h) * ppa - (f + al.h) * nn) / den;
                }
                d_sdf[k] = da * dadf;
                d_cos[k] = da * dadc;
                ds += da * dads;
                d_rgbs[3 * k] = gr0 * w; d_rgbs[3 * k + 1] = gr1 * w; d_rgbs[3 * k + 2] = gr2 * w;
                if (d_aux) { d_aux[3 * k] = ga0 * w; d_aux[3 * k + 1] = ga1 * w; d_aux[3 * k + 2] = ga2 * w; }
            }
            const float A0 = __shfl(A, 0, NGP_WAVE), B0 = __shfl(B, 0, NGP_WAVE);
            X = B0 + A0 * X;
        }
    }
    ds = wave_sum(ds);
    if (lane == 0) ds_rows[n] = ds;
}

// d_inv_s = sum of the per-ray rows, one block, fixed order: thread t sums rows t, t + 1024, ...; the 1024 partials meet through a
// wave butterfly and one LDS row.
__global__ void __launch_bounds__(1024) surface_ds_reduce_kernel(const float* __restrict__ rows, int n, float* __restrict__ out) {
    __shared__ float part[16];
    float v = 0.0f;
    for (int i = threadIdx.x; i < n; i += 1024) v += rows[i];
    v = wave_sum(v);
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    if (lane == 0) part[wave] = v;
    __syncthreads();
    if (wave == 0) {
        float t = lane < 16 ? part[lane] : 0.0f;
        t = wave_sum(t);
        if (lane == 0) out[0] = t;
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_surface_composite_fwd(const float* sdf, const float* cosv, const float* rgbs, const float* aux, const float* deltas,
                              const float* ts, const int32_t* rays_a, const float* inv_s, float cos_anneal, float T_threshold, int n_rays,
                              float bg, int32_t* total_samples, float* opacity, float* depth, float* rgb, float* rgb_out, float* aux_out,
                              float* ws, float* alphas, void* stream) {
    if (n_rays <= 0) return 0;
    if (!rays_a || !inv_s || !total_samples || !opacity || !depth || !rgb) return -1;
    if (aux_out && !aux) return -1;
    dim3 grid((n_rays + 3) / 4), block(256);
    hipLaunchKernelGGL(surface_fwd_kernel, grid, block, 0, (hipStream_t)stream, sdf, cosv, rgbs, aux, deltas, ts, rays_a, inv_s, cos_anneal,
                       T_threshold, n_rays, bg, total_samples, opacity, depth, rgb, rgb_out, aux_out, ws, alphas);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_surface_composite_bwd(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb, const float* dL_daux,
                              const float* dL_dws, const float* sdf, const float* cosv, const float* rgbs, const float* aux,
                              const float* deltas, const float* ts, const int32_t* rays_a, const float* inv_s, float cos_anneal, int n_rays,
                              float bg, const int32_t* total_samples, const float* alphas, float* d_sdf, float* d_cos, float* d_rgbs,
                              float* d_aux, float* d_inv_s, float* workspace, void* stream) {
    if (n_rays <= 0) return 0;
    if (!dL_drgb || !rays_a || !inv_s || !total_samples || !alphas || !d_inv_s || !workspace) return -1;
    if (d_aux && !aux) return -1;
    dim3 grid((n_rays + 3) / 4), block(256);
    hipLaunchKernelGGL(surface_bwd_kernel, grid, block, 0, (hipStream_t)stream, dL_dopacity, dL_ddepth, dL_drgb, dL_daux, dL_dws, sdf, cosv,
                       rgbs, aux, deltas, ts, rays_a, inv_s, cos_anneal, n_rays, bg, total_samples, alphas, d_sdf, d_cos, d_rgbs, d_aux,
                       workspace);
    NGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(surface_ds_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, workspace, n_rays, d_inv_s);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
