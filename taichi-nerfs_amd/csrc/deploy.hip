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
#include "ngp_device.h"
#include "hash_common.h"

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

__global__ void __launch_bounds__(256) deploy_shade_kernel(const float* __restrict__ xyzs, const float* __restrict__ dirs,
                                                           const float* __restrict__ table, DeployLevels lv,
                                                           const float* __restrict__ sigma_w, const float* __restrict__ rgb_w, int n,
                                                           float* __restrict__ sigmas, float* __restrict__ rgbs,
                                                           float* __restrict__ enc_out) {
    const float* __restrict__ sw = sigma_w;    // wave-uniform addresses at compile-time offsets: scalar loads, SGPR operands
    const float* __restrict__ rw = rgb_w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float px = xyzs[3 * (size_t)i] + 0.5f, py = xyzs[3 * (size_t)i + 1] + 0.5f, pz = xyzs[3 * (size_t)i + 2] + 0.5f;
        const float dx = dirs[3 * (size_t)i], dy = dirs[3 * (size_t)i + 1], dz = dirs[3 * (size_t)i + 2];

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
                reinterpret_cast<float4*>(enc_out)[4 * (size_t)i + l] = make_float4(enc[4 * l], enc[4 * l + 1], enc[4 * l + 2], enc[4 * l + 3]);
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
        sigmas[i] = expf(in[16]);
        rgbs[3 * (size_t)i] = 1.0f / (1.0f + expf(-s0));
        rgbs[3 * (size_t)i + 1] = 1.0f / (1.0f + expf(-s1));
        rgbs[3 * (size_t)i + 2] = 1.0f / (1.0f + expf(-s2));
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_deploy_shade(const float* xyzs, const float* dirs, const float* table, const ngp_hash_levels* lv, const float* sigma_w,
                     const float* rgb_w, int n, float* sigmas, float* rgbs, float* enc_out, void* stream) {
    if (n <= 0) return 0;
    if (!lv || lv->n_levels != 4 || lv->n_features != 4 || lv->begin_fast_hash_level != 4) return -1;   // four dense levels of float4 rows
    if (!xyzs || !dirs || !table || !sigma_w || !rgb_w || !sigmas || !rgbs) return -1;
    if (((uintptr_t)table & 15u) || ((uintptr_t)enc_out & 15u)) return -1;                                // 16-byte gathers / stores
    DeployLevels dl;
    for (int l = 0; l < 4; ++l) {
        if (lv->map_size[l] == 0 || (uint64_t)lv->offset[l] + lv->map_size[l] > (uint64_t)lv->total_entries) return -1;
        dl.scale[l] = lv->scale[l]; dl.res[l] = lv->resolution[l]; dl.size[l] = lv->map_size[l]; dl.offset[l] = lv->offset[l];
    }
    int blocks = (n + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(deploy_shade_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, xyzs, dirs, table, dl, sigma_w, rgb_w, n,
                       sigmas, rgbs, enc_out);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
