// ray_grad.hip -- first-order adjoints of the ray geometry: samples -> rays (ngp_march_train_bwd) and rays -> camera poses
// (ngp_sample_rays_bwd, ngp_get_rays_bwd).  Together with the hash encoder's position gradient (hash_grad_input.hip) they carry a
// loss on the rendered colour back to rays_o / rays_d and to the [3,4] camera-to-world matrices (pose refinement).
//
// Both reductions follow the library's rule for sums: plain loads, a fixed order, no float atomics.  Each output element is owned
// by one wave (march) or one block (poses); the order in which its terms meet depends on the inputs' shapes only, so two launches
// give the same bytes, and a NaN stays inside the ray / image it belongs to.  The orders differ from a serial loop, so the kernels
// are tolerance-checked against a float64 evaluation (tests/ray_grad_reference.py), like the composites.
#include "ngp_device.h"

namespace ngp {

// ---- adjoint of march.hip's sample write: xyzs[s] = o + t[s] d, dirs[s] = d, t held constant ---------------------------------
// One wave per rays_a row (ray_idx, start, N).  Lane l adds the samples l, l + 64, ... of the ray in that order (each a coalesced
// 12-byte row), then one xor butterfly (32, 16, ..., 1) combines the 64 partial sums.  The rays_d term is (t * dx) + dd: two f32
// roundings (the build keeps -ffp-contract=off).
template <bool HAS_X, bool HAS_D>
__global__ void __launch_bounds__(256) march_train_bwd_kernel(const float* __restrict__ d_xyzs, const float* __restrict__ d_dirs,
                                                              const float* __restrict__ ts, const int32_t* __restrict__ rays_a,
                                                              int n_rays, float* __restrict__ d_rays_o, float* __restrict__ d_rays_d) {
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= n_rays) return;
    const int lane = lane_id();
    const int ray_idx = rays_a[3 * n], start = rays_a[3 * n + 1], N = rays_a[3 * n + 2];
    if (ray_idx < 0 || ray_idx >= n_rays) return;          // a malformed row owns no output row
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f;
#pragma unroll 4
    for (int j = lane; j < N; j += NGP_WAVE) {
        const size_t s = (size_t)start + j;
        float x0 = 0.f, x1 = 0.f, x2 = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (HAS_X) {
            const float t = ts[s];
            x0 = d_xyzs[3 * s]; x1 = d_xyzs[3 * s + 1]; x2 = d_xyzs[3 * s + 2];
            o0 += x0; o1 += x1; o2 += x2;
            x0 = t * x0; x1 = t * x1; x2 = t * x2;
        }
        if (HAS_D) { g0 = d_dirs[3 * s]; g1 = d_dirs[3 * s + 1]; g2 = d_dirs[3 * s + 2]; }
        e0 += x0 + g0; e1 += x1 + g1; e2 += x2 + g2;
    }
    o0 = wave_sum(o0); o1 = wave_sum(o1); o2 = wave_sum(o2);
    e0 = wave_sum(e0); e1 = wave_sum(e1); e2 = wave_sum(e2);
    if (lane == 0) {
        float* po = d_rays_o + 3 * (size_t)ray_idx;
        float* pd = d_rays_d + 3 * (size_t)ray_idx;
        po[0] = o0; po[1] = o1; po[2] = o2;
        pd[0] = e0; pd[1] = e1; pd[2] = e2;
    }
}

// ---- adjoint of rays.hip's ray_from_pose, reduced per image ------------------------------------------------------------------
// rays_d[k][r] = sum_c dir[pix(k)][c] R[img(k)][r][c], rays_o[k][r] = t[img(k)][r]  =>
// d_poses[i][r][c] = sum_{k: img(k) = i} d_rays_d[k][r] dir[pix(k)][c] (c < 3), d_poses[i][r][3] = sum_{k: img(k) = i} d_rays_o[k][r].
// One 256-thread block per image: thread t visits k = t, t + 256, ... of ALL n rays in that order and keeps the twelve partial sums
// of the rays that belong to its image; the 256 partials meet in one xor butterfly per wave and (w0 + w1) + (w2 + w3) across the
// four waves.  The order is a function of (n, img_idx) alone.  Rays of an image outside [0, n_img) match no block.
constexpr int POSE_THREADS = 256;

__global__ void __launch_bounds__(POSE_THREADS) sample_rays_bwd_kernel(const float* __restrict__ directions,
                                                                       const int64_t* __restrict__ img_idx, long long img0,
                                                                       const int64_t* __restrict__ pix_idx,
                                                                       const float* __restrict__ d_rays_o,
                                                                       const float* __restrict__ d_rays_d, int n,
                                                                       float* __restrict__ d_poses) {
    __shared__ float part[POSE_THREADS / NGP_WAVE][12];
    const long long img = blockIdx.x;
    float acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.f;
    if (img_idx || img == img0) {
        for (int k = threadIdx.x; k < n; k += POSE_THREADS) {
            if (img_idx && img_idx[k] != img) continue;
            if (d_rays_d) {
                const float* dir = directions + 3 * (size_t)(pix_idx ? pix_idx[k] : (long long)k);
                const float c0 = dir[0], c1 = dir[1], c2 = dir[2];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float g = d_rays_d[3 * (size_t)k + r];
                    acc[4 * r] += g * c0; acc[4 * r + 1] += g * c1; acc[4 * r + 2] += g * c2;
                }
            }
            if (d_rays_o) {
#pragma unroll
                for (int r = 0; r < 3; ++r) acc[4 * r + 3] += d_rays_o[3 * (size_t)k + r];
            }
        }
    }
    const int lane = lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        acc[q] = wave_sum(acc[q]);
        if (lane == 0) part[wave][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < 12)
        d_poses[12 * (size_t)img + threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// per-ray poses (get_rays with c2w [n,3,4]): nothing to reduce, one lane per ray writes its twelve entries
__global__ void __launch_bounds__(256) get_rays_bwd_kernel(const float* __restrict__ directions, const float* __restrict__ d_rays_o,
                                                           const float* __restrict__ d_rays_d, int n, float* __restrict__ d_poses) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const float* dir = directions + 3 * (size_t)k;
        const float c0 = dir[0], c1 = dir[1], c2 = dir[2];
        float* out = d_poses + 12 * (size_t)k;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float g = d_rays_d ? d_rays_d[3 * (size_t)k + r] : 0.f;
            out[4 * r] = g * c0; out[4 * r + 1] = g * c1; out[4 * r + 2] = g * c2;
            out[4 * r + 3] = d_rays_o ? d_rays_o[3 * (size_t)k + r] : 0.f;
        }
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_march_train_bwd(const float* d_xyzs, const float* d_dirs, const float* ts, const int32_t* rays_a, int n_rays, float* d_rays_o,
                        float* d_rays_d, void* stream) {
    if (n_rays <= 0) return 0;
    if (!rays_a || !d_rays_o || !d_rays_d || (d_xyzs && !ts)) return -1;
    dim3 grid((n_rays + 3) / 4), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (d_xyzs && d_dirs)
        hipLaunchKernelGGL((march_train_bwd_kernel<true, true>), grid, block, 0, st, d_xyzs, d_dirs, ts, rays_a, n_rays, d_rays_o, d_rays_d);
    else if (d_xyzs)
        hipLaunchKernelGGL((march_train_bwd_kernel<true, false>), grid, block, 0, st, d_xyzs, d_dirs, ts, rays_a, n_rays, d_rays_o, d_rays_d);
    else if (d_dirs)
        hipLaunchKernelGGL((march_train_bwd_kernel<false, true>), grid, block, 0, st, d_xyzs, d_dirs, ts, rays_a, n_rays, d_rays_o, d_rays_d);
    else
        hipLaunchKernelGGL((march_train_bwd_kernel<false, false>), grid, block, 0, st, d_xyzs, d_dirs, ts, rays_a, n_rays, d_rays_o, d_rays_d);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_sample_rays_bwd(const float* directions, const int64_t* img_idx, long long img0, const int64_t* pix_idx, const float* d_rays_o,
                        const float* d_rays_d, int n, int n_img, float* d_poses, void* stream) {
    if (n_img <= 0) return 0;
    if (n < 0 || !d_poses || (n > 0 && d_rays_d && !directions)) return -1;
    hipLaunchKernelGGL(sample_rays_bwd_kernel, dim3(n_img), dim3(POSE_THREADS), 0, (hipStream_t)stream, directions, img_idx, img0, pix_idx,
                       d_rays_o, d_rays_d, n, d_poses);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_get_rays_bwd(const float* directions, const float* d_rays_o, const float* d_rays_d, int n, float* d_poses, void* stream) {
    if (n <= 0) return 0;
    if (!d_poses || (d_rays_d && !directions)) return -1;
    int blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(get_rays_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, directions, d_rays_o, d_rays_d, n, d_poses);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
