// mesh_bvh.h -- what the three queries against the box hierarchy of a triangle mesh share: the shape of the implicit tree (mesh_sdf.hip
// builds it and states its layout), the limits the entries refuse beyond, and the three-float helpers.  mesh_sdf.hip asks the tree for
// the nearest face of a point, mesh_raycast.hip for the first face along a ray, mesh_winding.hip for the winding number of a point.
#pragma once
#include "ngp_device.h"

namespace ngp {

constexpr int MESH_SDF_MAX_DEPTH = 24;                         // one bit of `trail` per level: 2^24 leaves
constexpr int MESH_SDF_MAX_LEAF = NGP_MESH_SDF_MAX_LEAF;

struct MeshTree {
    long long leaves;        // ceil(n_faces / leaf_size)
    long long padded;        // P
    int depth;               // log2 P
};
__host__ __forceinline__ bool mesh_tree(long long n_faces, int leaf_size, MeshTree& t) {
    if (n_faces < 1 || n_faces > 0x7fffffffll || leaf_size < 1 || leaf_size > MESH_SDF_MAX_LEAF) return false;
    t.leaves = (n_faces + leaf_size - 1) / leaf_size;
    t.padded = 1;
    t.depth = 0;
    while (t.padded < t.leaves) { t.padded <<= 1; ++t.depth; }
    return t.depth <= MESH_SDF_MAX_DEPTH;
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3_load(const float* __restrict__ p, long long i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ V3 v3_sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float v3_dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

}  // namespace ngp
