// hash_common.h -- the hash-grid corner rule, defined once: which table entry is corner c of level l, and with what weight.
// Level modes, the dense / xor-hash index, cell and fraction, the trilinear weight and the pair-major address of a level's two
// features (hash_encoder.py:43-71, 100-137) + the level table in LDS and the position normalisation.  Used by hash_grid.hip,
// hash_bwd_lds.hip and deploy.hip; every kernel must agree on these bit for bit, so none of them spells them out itself.
#pragma once
#include "ngp_device.h"

namespace ngp {

constexpr uint32_t HASH_PRIME_Y = 2654435761u, HASH_PRIME_Z = 805459861u;      // fast_hash :43-51 (x's factor is 1)

// How a level's raw index is brought below its entry count: 0 conditional subtract, 1 mask, 2 real modulo.
__host__ __device__ __forceinline__ uint32_t level_mode(const ngp_hash_levels& lv, int level) {
    const uint32_t sz = lv.map_size[level];
    if (level < lv.begin_fast_hash_level) {
        // dense level: idx <= res^3 + res^2 + res < 2*size whenever size >= res^3, so one conditional
        // subtract equals `% size` (hash_encoder.py:71); anything else falls back to the real modulo.
        const uint64_t r = lv.resolution[level];
        return ((uint64_t)sz >= r * r * r && r >= 2) ? 0u : 2u;
    }
    return (sz != 0 && (sz & (sz - 1)) == 0) ? 1u : 2u;
}

// Entry (relative to the level's first) of grid point (gx, gy, gz).  Every mode gives `% size` of the raw index for ANY input
// -- mode 0 keeps the real modulo behind its subtract --, so the result is always < size; the modes only say which form is cheap.
__device__ __forceinline__ uint32_t level_index(bool dense, uint32_t mode, uint32_t size, uint32_t res, uint32_t gx, uint32_t gy,
                                                uint32_t gz) {
    uint32_t h = dense ? (gx + gy * res + gz * res * res) : (gx ^ (gy * HASH_PRIME_Y) ^ (gz * HASH_PRIME_Z));   // :53-60 / :43-51
    if (mode == 1u) h &= (size - 1u);
    else if (mode == 0u) { if (h >= size) { h -= size; if (h >= size) h %= size; } }
    else h = h % size;                                                                                          // :71
    return h;
}

// Cell and fraction of a position on a level (:100-110); level_cell is the cell of one coordinate alone (the scatter-add's prepass
// needs no fractions).  HALF_CELL: the half2 encoder casts the cell to f16 before the subtract (hash_encoder_half.py:133).
__device__ __forceinline__ float level_pos(float x, float scale) { return x * scale + 0.5f; }
__device__ __forceinline__ uint32_t level_cell(float x, float scale) { return f2u_sat(floorf(level_pos(x, scale))); }
template <bool HALF_CELL>
__device__ __forceinline__ void cell_frac(const float x[3], float scale, uint32_t cell[3], float fr[3]) {
    const float pos[3] = {level_pos(x[0], scale), level_pos(x[1], scale), level_pos(x[2], scale)};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cell[k] = f2u_sat(floorf(pos[k]));
        const float cf = (float)cell[k];
        fr[k] = pos[k] - (HALF_CELL ? f16_round(cf) : cf);
    }
}

// Trilinear weight of corner ci (bit d set: the far side along axis d), in the reference's product order
// ((1 * wx) * wy) * wz (:112-137).
__device__ __forceinline__ float corner_weight(int ci, const float fr[3]) {
    return ((1.0f * ((ci & 1) ? fr[0] : 1.0f - fr[0])) * ((ci & 2) ? fr[1] : 1.0f - fr[1])) * ((ci & 4) ? fr[2] : 1.0f - fr[2]);
}

// Where sample i's two features of `level` sit in the encoding / encoding-gradient buffer `enc`: the natural [n, n_levels * 2]
// rows, or (enc_pairs, 16 levels) eight pair-major planes [8][plane][4], plane p = levels p and 15 - p.  (It takes the buffer and
// returns an address, not an offset: each layout's small constant term then stays a pointer add of its own, which is the form
// the scatter-add's gathers were tuned with.)
__device__ __forceinline__ const float* enc_ptr(const float* enc, int level, size_t i, size_t plane, int enc_pairs, int n_levels) {
    return enc_pairs ? enc + ((size_t)(level < 8 ? level : 15 - level) * plane + i) * 4 + (level < 8 ? 0 : 2)
                     : enc + i * (size_t)(n_levels * 2) + level * 2;
}

struct LevelLDS {
    float scale[NGP_MAX_LEVELS];
    uint32_t res[NGP_MAX_LEVELS];
    uint32_t size[NGP_MAX_LEVELS];
    uint32_t offset[NGP_MAX_LEVELS];
    uint32_t mode[NGP_MAX_LEVELS];   // level_mode
};

__device__ __forceinline__ void load_levels(const ngp_hash_levels& lv, LevelLDS& s) {
    int t = threadIdx.x;
    if (t < NGP_MAX_LEVELS) {
        s.scale[t] = lv.scale[t];
        s.res[t] = lv.resolution[t];
        s.size[t] = lv.map_size[t];
        s.offset[t] = lv.offset[t];
        s.mode[t] = level_mode(lv, t);
    }
    __syncthreads();
}

struct XyzNorm {            // optional fused (x - lo) / (hi - lo) of reference networks.py:144 (same two f32 ops)
    int enabled;
    float lo, hi;
};
__device__ __forceinline__ float norm01(const XyzNorm& nm, float v) { return nm.enabled ? (v - nm.lo) / (nm.hi - nm.lo) : v; }

}  // namespace ngp
