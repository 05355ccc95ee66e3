// resample.hip -- importance resampling along rays: inverse-CDF refinement of marched sections, for gfx950.
//
// A ray's samples are sections [lo_j, hi_j] = [t_j - delta_j / 2, t_j + delta_j / 2] with a weight each (the ws of any compositor).  K
// stratified draws u_k = (k + noise) / K are pushed through the inverse of the ray's cumulative weight; every draw that lands strictly
// inside a section cuts it there.  Sections are only ever cut: the union of a ray's sections, gaps included, is what it was.  The
// contract -- every rounding of it -- is in include/ngp_hip.h ("importance resampling").
//
// Shape: the march's count / scan / write chain (march.hip).
//   count  one 64-lane wave owns a ray, four waves per block.  Pass 1 walks the ray's sections in coalesced groups of 64: w = max(ws, 0)
//          + floor, an additive wave scan with a wave-uniform carry (the order of the sum is part of the contract), the CDF to the
//          wave's 4 KB row of LDS (a ray of up to 1024 sections, the march's max_samples) or, for a longer ray, to a [S] workspace
//          in global memory.  Pass 2 gives one lane per draw, 64 draws at a time: a binary search in the ray's CDF slice, t*, the kept test,
//          and the rank of a kept cut through ballot + popcount with a carry.  Kept cuts are staged compacted, (t*, section) at
//          [row, rank] of a [n, K] workspace, ascending by construction.  counts[row] = N + kept.
//   scan   the march's one-block scan, keeping the ray index of every row (rays_a may list the rays in any order).
//   write  one wave per ray.  A lane per section writes the section's first child (the whole section where nothing cut it: t and delta
//          are then copied bit for bit); a lane per kept cut writes the child that starts at that cut.  Child r + 1 of a ray's cut
//          number r in section j sits at j + r + 1; the first child of section j at j + (number of cuts in sections before j), found
//          by a binary search in the staged sections.
//
// No atomics, no fast-math, no contraction: the same inputs give the same bytes.  The one cross-lane hand-over through memory (pass 2
// reads CDF entries other lanes of the same wave wrote in pass 1) needs no hardware fence in LDS; on the global path it is ordered by a
// device-scope fence, which also drops whatever line of the slice a neighbouring ray's wave may have pulled into this CU's vector cache
// before the write (first measured with every ray on that path: 51.7 us for the count kernel at 8192 rays / 217 k sections / K = 32).
#include "ngp_device.h"

namespace ngp {

constexpr int RESAMPLE_LDS_SECTIONS = 1024;                  // = ngp_hip.surface.MAX_SAMPLES: 4 KB per wave, 16 KB per block

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }       // false for NaN and +-inf

struct ResampleRow {
    int ray_idx, start, N;
    bool ok;
};

// A row of rays_a that points outside the buffers is refused, not followed: it gets no samples and raises the launch's error flag.
__device__ __forceinline__ ResampleRow resample_row(const int32_t* __restrict__ rays_a, int n, int n_orig, long long S) {
    ResampleRow r;
    r.ray_idx = rays_a[3 * n]; r.start = rays_a[3 * n + 1]; r.N = rays_a[3 * n + 2];
    r.ok = r.ray_idx >= 0 && r.ray_idx < n_orig && r.start >= 0 && r.N >= 0 && (long long)r.start + (long long)r.N <= S;
    return r;
}

// One ray of the count kernel.  c_row: where the ray's CDF lives -- the wave's LDS row (LDS = true) or its slice of the global workspace;
// two instantiations, so that each addresses one memory.
template <bool LDS>
__device__ __forceinline__ void resample_count_ray(const float* __restrict__ ws, const float* __restrict__ deltas,
                                                   const float* __restrict__ ts, float nz, int N, int K, float floor_w, float* c_row,
                                                   float* __restrict__ stage_t, int32_t* __restrict__ stage_j, int32_t* count, int lane) {
    // pass 1: the CDF, 64 sections at a time; c_j = carry + (inclusive wave scan of the group)_j
    float carry = 0.0f;
    bool bad = false;
    for (int base = 0; base < N; base += NGP_WAVE) {
        const int j = base + lane;
        float w = 0.0f;
        bool nf = false;
        if (j < N) {
            const float x = ws[j];
            nf = !finite_f(x);
            w = (x < 0.0f ? 0.0f : x) + floor_w;
        }
        bad = bad || __ballot(nf) != 0;
        const float c = carry + wave_scan_add(w, lane);
        if (j < N) c_row[j] = c;
        carry = __shfl(c, NGP_WAVE - 1, NGP_WAVE);
    }
    const float c_last = carry;
    if (bad || !(c_last > 0.0f) || !finite_f(c_last)) {       // copied through by the write kernel: no cuts
        if (lane == 0) *count = N;
        return;
    }
    // pass 2 reads entries other lanes of this wave wrote.  LDS: a wave's DS operations complete in order, the fence only keeps the
    // compiler from moving them.  Global: a device-scope fence (see the head of the file).
    if (LDS) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    else __threadfence();
    // pass 2: one lane per draw
    const float Kf = (float)K;
    int kept_before = 0;
    float prev_carry = 0.0f;
    for (int base = 0; base < K; base += NGP_WAVE) {
        const int k = base + lane;
        float tstar = 0.0f;
        int sec = 0;
        bool inr = false;
        if (k < K) {
            const float u = ((float)k + nz) / Kf;
            const float target = u * c_last;
            int lo = 0, hi = N;
            while (lo < hi) {                                  // the first section with c_j > target
                const int mid = (lo + hi) >> 1;
                if (c_row[mid] > target) hi = mid; else lo = mid + 1;
            }
            sec = lo;
            if (sec < N) {
                const float c_prev = sec > 0 ? c_row[sec - 1] : 0.0f;
                const float x = ws[sec];
                const float w = (x < 0.0f ? 0.0f : x) + floor_w;
                const float t = ts[sec], dl = deltas[sec];
                const float lo_e = t - 0.5f * dl, hi_e = t + 0.5f * dl;
                tstar = lo_e + (target - c_prev) / w * dl;
                inr = lo_e < tstar && tstar < hi_e;            // (false for the NaN / inf of a zero weight)
            }
        }
        float prev = __shfl_up(tstar, 1, NGP_WAVE);
        if (lane == 0) prev = prev_carry;
        const bool keep = inr && !(k > 0 && tstar == prev);
        const uint64_t m = __ballot(keep);
        if (keep) {
            const int r = kept_before + __popcll(m & ((1ull << lane) - 1ull));
            stage_t[r] = tstar;
            stage_j[r] = sec;
        }
        kept_before += __popcll(m);
        prev_carry = __shfl(tstar, NGP_WAVE - 1, NGP_WAVE);
    }
    if (lane == 0) *count = N + kept_before;
}

__global__ void __launch_bounds__(256) resample_count_kernel(const float* __restrict__ ws, const float* __restrict__ deltas,
                                                             const float* __restrict__ ts, const int32_t* __restrict__ rays_a,
                                                             const float* __restrict__ noise, int n_rays, int n_orig, long long S, int K,
                                                             float floor_w, float* cdf, float* __restrict__ stage_t,
                                                             int32_t* __restrict__ stage_j, int32_t* __restrict__ counts,
                                                             int32_t* __restrict__ total) {
    __shared__ float cdf_lds[4][RESAMPLE_LDS_SECTIONS];
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= n_rays) return;
    const int lane = lane_id();
    const ResampleRow row = resample_row(rays_a, n, n_orig, S);
    if (!row.ok) {
        if (lane == 0) { counts[n] = 0; total[1] = 1; }
        return;
    }
    const size_t s0 = (size_t)row.start, st0 = (size_t)n * (size_t)K;
    const float nz = noise[row.ray_idx];
    // the ray's CDF lives in this wave's LDS row when it fits (the march's max_samples does), in the global workspace otherwise
    if (row.N <= RESAMPLE_LDS_SECTIONS)
        resample_count_ray<true>(ws + s0, deltas + s0, ts + s0, nz, row.N, K, floor_w, cdf_lds[threadIdx.x >> 6], stage_t + st0,
                                 stage_j + st0, counts + n, lane);
    else
        resample_count_ray<false>(ws + s0, deltas + s0, ts + s0, nz, row.N, K, floor_w, cdf + s0, stage_t + st0, stage_j + st0,
                                  counts + n, lane);
}

// march_scan_kernel with the ray index of every row carried over: exclusive prefix sum over the per-row counts -> rays_a_out + total[0].
__global__ void __launch_bounds__(1024) resample_scan_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ rays_a,
                                                             int n_rays, int32_t* __restrict__ rays_a_out, int32_t* __restrict__ total) {
    __shared__ int wave_tot[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (n_rays + 1023) >> 10;
    const int lo = min(tid * per, n_rays), hi = min(lo + per, n_rays);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += counts[i];
    const int inc = wave_scan_add_i(sum, lane);
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    int woff = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) woff += (w < wv) ? wave_tot[w] : 0;
    int run = woff + inc - sum;
    for (int i = lo; i < hi; ++i) {
        const int c = counts[i];
        rays_a_out[3 * i] = rays_a[3 * i]; rays_a_out[3 * i + 1] = run; rays_a_out[3 * i + 2] = c;
        run += c;
    }
    if (tid == 1023) total[0] = woff + inc;
}

__device__ __forceinline__ void resample_emit(size_t p, float t, float dl, int parent_idx, const float (&o)[3], const float (&d)[3],
                                              float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas_out,
                                              float* __restrict__ ts_out, int32_t* __restrict__ parent) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        xyzs[3 * p + a] = o[a] + t * d[a];                     // the march's own expression (march_write_kernel)
        dirs[3 * p + a] = d[a];
    }
    ts_out[p] = t;
    deltas_out[p] = dl;
    parent[p] = parent_idx;
}

__global__ void __launch_bounds__(256) resample_write_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                             const float* __restrict__ deltas, const float* __restrict__ ts,
                                                             const int32_t* __restrict__ rays_a, const int32_t* __restrict__ rays_a_out,
                                                             const float* __restrict__ stage_t, const int32_t* __restrict__ stage_j,
                                                             int n_rays, int n_orig, long long S, int K, float* __restrict__ xyzs,
                                                             float* __restrict__ dirs, float* __restrict__ deltas_out,
                                                             float* __restrict__ ts_out, int32_t* __restrict__ parent) {
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= n_rays) return;
    const int lane = lane_id();
    const ResampleRow row = resample_row(rays_a, n, n_orig, S);
    const int N = row.N;
    const int cnt = rays_a_out[3 * n + 2];
    if (!row.ok || cnt <= 0) return;
    const int M = min(max(cnt - N, 0), K);                     // kept cuts of this ray
    const size_t s0 = (size_t)row.start, p0 = (size_t)rays_a_out[3 * n + 1], st0 = (size_t)n * (size_t)K;
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { o[a] = rays_o[3 * row.ray_idx + a]; d[a] = rays_d[3 * row.ray_idx + a]; }
    // the first child of every section
    for (int j = lane; j < N; j += NGP_WAVE) {
        int lo = 0, hi = M;
        while (lo < hi) {                                      // cuts in the sections before j
            const int mid = (lo + hi) >> 1;
            if (stage_j[st0 + mid] < j) lo = mid + 1; else hi = mid;
        }
        float t = ts[s0 + j], dl = deltas[s0 + j];
        if (lo < M && stage_j[st0 + lo] == j) {
            const float a = t - 0.5f * dl, b = stage_t[st0 + lo];
            t = 0.5f * (a + b); dl = b - a;
        }
        resample_emit(p0 + j + lo, t, dl, row.start + j, o, d, xyzs, dirs, deltas_out, ts_out, parent);
    }
    // the child that starts at every kept cut
    for (int r = lane; r < M; r += NGP_WAVE) {
        const int j = stage_j[st0 + r];
        if (j < 0 || j >= N) continue;
        const float a = stage_t[st0 + r];
        float b;
        if (r + 1 < M && stage_j[st0 + r + 1] == j) b = stage_t[st0 + r + 1];
        else b = ts[s0 + j] + 0.5f * deltas[s0 + j];
        resample_emit(p0 + j + r + 1, 0.5f * (a + b), b - a, row.start + j, o, d, xyzs, dirs, deltas_out, ts_out, parent);
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_resample_count(const float* ws, const float* deltas, const float* ts, const int32_t* rays_a, const float* noise, int n_rays,
                       int n_orig, long long n_samples, int K, float floor_w, float* cdf, float* stage_t, int32_t* stage_j,
                       int32_t* counts, int32_t* total, void* stream) {
    if (n_rays <= 0) return 0;
    if (!rays_a || !noise || !stage_t || !stage_j || !counts || !total || K < 1 || n_orig < 1 || n_samples < 0 || !(floor_w >= 0.0f))
        return -1;
    if (n_samples > 0 && (!ws || !deltas || !ts || !cdf)) return -1;
    dim3 grid((n_rays + 3) / 4), block(256);
    hipLaunchKernelGGL(resample_count_kernel, grid, block, 0, (hipStream_t)stream, ws, deltas, ts, rays_a, noise, n_rays, n_orig,
                       n_samples, K, floor_w, cdf, stage_t, stage_j, counts, total);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_resample_scan(const int32_t* counts, const int32_t* rays_a, int n_rays, int32_t* rays_a_out, int32_t* total, void* stream) {
    if (n_rays <= 0) return 0;
    if (!counts || !rays_a || !rays_a_out || !total) return -1;
    hipLaunchKernelGGL(resample_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, rays_a, n_rays, rays_a_out, total);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_resample_write(const float* rays_o, const float* rays_d, const float* deltas, const float* ts, const int32_t* rays_a,
                       const int32_t* rays_a_out, const float* stage_t, const int32_t* stage_j, int n_rays, int n_orig,
                       long long n_samples, int K, float* xyzs, float* dirs, float* deltas_out, float* ts_out, int32_t* parent,
                       void* stream) {
    if (n_rays <= 0) return 0;
    if (!rays_o || !rays_d || !deltas || !ts || !rays_a || !rays_a_out || !stage_t || !stage_j || !xyzs || !dirs || !deltas_out ||
        !ts_out || !parent || K < 1 || n_orig < 1 || n_samples < 0)
        return -1;
    dim3 grid((n_rays + 3) / 4), block(256);
    hipLaunchKernelGGL(resample_write_kernel, grid, block, 0, (hipStream_t)stream, rays_o, rays_d, deltas, ts, rays_a, rays_a_out, stage_t,
                       stage_j, n_rays, n_orig, n_samples, K, xyzs, dirs, deltas_out, ts_out, parent);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
