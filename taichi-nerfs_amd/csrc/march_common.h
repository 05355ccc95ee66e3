// march_common.h -- the march step rule, the coarse-block table and the slab test, shared by march.hip (the march kernels),
// deploy.hip (the fused march-shade-composite of the deployment renderer) and sdf_trace.hip (the sphere tracer's empty-space skip).
// One definition each: a kernel that walks a ray through the occupancy grid includes this header and calls these.  (The occupancy
// test of a probed cell is NOT here: as a shared function it changed all three kernels' code and two of them measured slower,
// profiles/composite_refactor.md; each kernel spells its three lines.)
#pragma once
#include "ngp_device.h"

namespace ngp {

struct MarchParams {
    int cascades, grid_size;
    uint32_t grid_size3;
    float grid_size_f, grid_size_inv, grid_max;   // G, 1/G, G-1
    float scale, esf, dt_min, dt_max;
    float scale_inv, mb0, mb0_inv;                // 1/scale; mip_bound of cascade 0 = min(2^-1, scale) and its reciprocal
    unsigned long long rng_seed;                  // rng != 0: the jitter of ray r is rng_uniform(rng_seed, r) instead of noise[r]
    int rng;
    long long capacity;                           // one-launch march: rows of the output arrays (samples at or beyond it are dropped,
};                                                // `total` still counts them); 0 = the caller guarantees n_rays * max_samples rows

__host__ inline MarchParams make_march_params(int cascades, int grid_size, float scale, float esf) {
    MarchParams p;
    p.cascades = cascades;
    p.grid_size = grid_size;
    p.grid_size3 = (uint32_t)grid_size * (uint32_t)grid_size * (uint32_t)grid_size;
    p.grid_size_f = (float)grid_size;
    p.grid_size_inv = 1.0f / (float)grid_size;
    p.grid_max = (float)grid_size - 1.0f;
    p.rng_seed = 0ull; p.rng = 0; p.capacity = 0;
    p.scale = scale;
    p.esf = esf;
    p.dt_min = (float)(1.7320508075688772 / 1024);                       // utils.py:15
    p.dt_max = (float)(1.7320508075688772 * 2) * scale / (float)grid_size;  // utils.py:16,56-57
    p.scale_inv = 1.0f / scale;
    p.mb0 = 0.5f < scale ? 0.5f : scale;
    p.mb0_inv = 1.0f / p.mb0;
    return p;
}

struct CellProbe {
    float xyz[3];
    float nxyz[3];
    float mip_bound;
    uint32_t idx;
};

// ray_march.py:46-60 for one orbit point.  CASC1 (one cascade, e.g. Synthetic-NeRF): mip == 0 for every point, so
// mip_bound = min(0.5, scale) and its reciprocal are wave-uniform constants.  Otherwise 1/mip_bound is 2^(1-mip) (exact,
// what the IEEE division of 1 by a power of two returns) or the precomputed 1/scale -- bit-identical, no per-point divide.
template <bool CASC1>
__device__ __forceinline__ void probe_cell(const MarchParams& p, const float o[3], const float d[3], float t, float dt,
                                           CellProbe& c) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c.xyz[k] = o[k] + t * d[k];
    float mip_bound_inv;
    int mip = 0;
    if (CASC1) {
        c.mip_bound = p.mb0;
        mip_bound_inv = p.mb0_inv;
    } else {
        float mx = fmaxf(fmaxf(fabsf(c.xyz[0]), fabsf(c.xyz[1])), fabsf(c.xyz[2]));
        int mip_pos = min(p.cascades - 1, max(0, frexp_bit(mx) + 1));                  // utils.py:78-84
        int mip_dt = min(p.cascades - 1, max(0, frexp_bit(dt * p.grid_size_f)));       // utils.py:87-92
        mip = max(mip_pos, mip_dt);
        const float pw = ldexpf(1.0f, mip - 1);
        const bool use_pw = pw <= p.scale;                                             // min(2^(mip-1), scale)
        c.mip_bound = use_pw ? pw : p.scale;
        mip_bound_inv = use_pw ? ldexpf(1.0f, 1 - mip) : p.scale_inv;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = 0.5f * (c.xyz[k] * mip_bound_inv + 1.0f) * p.grid_size_f;
        c.nxyz[k] = fminf(p.grid_max, fmaxf(0.0f, v));
    }
    // nxyz is clamped into [0, G-1] and never NaN (fminf/fmaxf drop NaNs): the hardware cvt is the truncating cast
    c.idx = (uint32_t)mip * p.grid_size3 + morton3d((uint32_t)c.nxyz[0], (uint32_t)c.nxyz[1], (uint32_t)c.nxyz[2]);
}

// ray_march.py:68-71: t_target of the skip taken from an empty cell
__device__ __forceinline__ float skip_target(const MarchParams& p, const float d[3], const float d_inv[3], float t,
                                             const CellProbe& c) {
    float tmin = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = (((c.nxyz[k] + 0.5f + 0.5f * fsign(d[k])) * p.grid_size_inv * 2.0f - 1.0f) * c.mip_bound - c.xyz[k]) * d_inv[k];
        tmin = k ? fminf(tmin, v) : v;
    }
    return t + fmaxf(0.0f, tmin);
}

// ray-AABB slab test of the box [-scale, scale]^3 (intersection.py:22-37), near plane 0.01: (t1, t2), or (-1, -1) for a miss.
// d_inv = 1 / d per component; a zero component gives +-inf or NaN bounds, which fminf / fmaxf order or drop.
__device__ __forceinline__ float2 ray_aabb_slab(const float o[3], const float d_inv[3], float scale) {
    const float half_size = (scale - (-scale)) / 2.0f;
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t_min = (0.0f - half_size - o[k]) * d_inv[k], t_max = (0.0f + half_size - o[k]) * d_inv[k];
        const float lo = fminf(t_min, t_max), hi = fmaxf(t_min, t_max);
        a1 = k ? fmaxf(a1, lo) : lo;
        a2 = k ? fminf(a2, hi) : hi;
    }
    return (a2 > 0.0f) ? make_float2(fmaxf(a1, 0.01f), a2) : make_float2(-1.0f, -1.0f);
}

constexpr int MARCH_MAX_COARSE_WORDS = 1024;            // 32 768 coarse blocks: up to 8 cascades of a 128^3 grid
constexpr int ORBIT_BATCH = 8;      // orbit points probed speculatively per iteration by the kernels with one lane per ray

// coarse occupancy: one bit per 8^3 block of cells == per 512 consecutive Morton codes (64 bitfield bytes).
// A clear bit proves the cell empty without touching the bitfield: most batches of a trained scene never issue a
// global load at all, which is what this latency-bound kernel is waiting on.
__device__ __forceinline__ bool load_coarse(const MarchParams& p, const uint32_t* __restrict__ coarse, uint32_t* __restrict__ coarse_s) {
    const int coarse_words = coarse ? (int)((p.grid_size3 >> 9) * (uint32_t)p.cascades + 31u) >> 5 : 0;
    const bool use_coarse = coarse != nullptr && coarse_words <= MARCH_MAX_COARSE_WORDS;
    if (use_coarse) {
        for (int k = threadIdx.x; k < coarse_words; k += blockDim.x) coarse_s[k] = coarse[k];
        __syncthreads();
    }
    return use_coarse;
}

}  // namespace ngp
