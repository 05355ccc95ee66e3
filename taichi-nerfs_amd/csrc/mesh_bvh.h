// mesh_bvh.h -- everything the queries against the box hierarchy of a triangle mesh do with the tree, once: its shape (mesh_sdf.hip
// builds it and states its layout), the limits the entries refuse beyond, the faces of a leaf, the bottom-up sweep of a build, the
// statement of the two-sided walk of a query, the microbenchmarks' counters and the three-float helpers.  mesh_sdf.hip asks the tree for the nearest face
// of a point, mesh_raycast.hip for the first face along a ray, mesh_winding.hip for the winding number of a point.
//
// THE WALK of the two sibling queries (mesh_sdf_query_kernel, mesh_raycast_kernel) is stackless: the tree is implicit, so sibling
// ((i - 1) ^ 1) + 1 and parent (i - 1) >> 1 are arithmetic, and one bit per level (`trail`, bit d = at depth d the second of the two
// children has been taken) replaces the stack -- no per-lane array, nothing in scratch or LDS.  The query gives every node a sort key (the
// distance query's lower bound, the ray cast's entry parameter) and has a limit; a node is entered iff key < limit.  Going down the lane
// takes the child with the smaller key first, the first of two equal ones, so the limit tightens early; coming back up it tests the
// sibling's box again, against the limit as it is by then (one 24-byte read instead of a stored bound).  Depth <= MESH_SDF_MAX_DEPTH = 24
// (2^24 leaves), the entries refuse more.
// TERMINATION.  Floats decide one thing only: whether a node is entered.  Every transition -- down to a child, across to the sibling, up
// to the parent -- is index arithmetic on `node`, `depth` and the trail bits, each node is gone down into at most once and left upwards
// at most once, so the walk ends after at most 3 (2 P - 1) steps for any key and limit, hence for any bit pattern in the query's
// inputs (NaN, +-inf, denormals): a comparison with a NaN is false and enters nothing.  A leaf adds at most leaf_size faces.
// The walk is stated and proved here once but WRITTEN in each of the two kernels, state for state alike: as one template over a query
// (key, limit, leaf) it gave the same bits and box counts, but the compiler laid the loops of mesh_raycast_kernel out otherwise (the leaf
// loop in the outermost loop of the walk) and 800 x 800 primary rays took a third longer; mesh_sdf_query_kernel missed the timing rule
// by 0.5 to 2.6 % on three workloads.  profiles/mesh_tree_refactor.md has the numbers.  Who changes one copy changes the other.
#pragma once
#include "ngp_device.h"

namespace ngp {

constexpr int MESH_SDF_MAX_DEPTH = 24;                         // one bit of `trail` per level: 2^24 leaves
constexpr int MESH_SDF_MAX_LEAF = NGP_MESH_SDF_MAX_LEAF;
constexpr int MESH_SWEEP_BLOCK = 256;                          // lanes per block of the build kernels, one lane per node

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

// the mesh below a tree, as every kernel takes it: order[s] = the caller's index of the face at sorted position s
struct MeshGeometry {
    const float* vertices;
    const int32_t* faces;
    const int32_t* order;
    int n_faces, leaf_size, padded;
};
// false: a null array, or a tree the entries refuse
__host__ __forceinline__ bool mesh_geometry(const float* vertices, const int32_t* faces, const int32_t* order, long long n_faces,
                                            int leaf_size, MeshGeometry& g, MeshTree& t) {
    if (!vertices || !faces || !order || !mesh_tree(n_faces, leaf_size, t)) return false;
    g = {vertices, faces, order, (int)n_faces, leaf_size, (int)t.padded};
    return true;
}

// a build: the leaves, then the inner levels bottom up, nodes [first, first + count) a launch
template <class Leaves, class Level>
__host__ __forceinline__ void mesh_tree_sweep(const MeshTree& t, hipStream_t stream, Leaves leaf_launch, Level level_launch) {
    const dim3 block(MESH_SWEEP_BLOCK);
    leaf_launch(dim3((unsigned)((t.padded + MESH_SWEEP_BLOCK - 1) / MESH_SWEEP_BLOCK)), block, stream);
    for (int d = t.depth - 1; d >= 0; --d) {
        const int count = 1 << d;
        level_launch(dim3((unsigned)((count + MESH_SWEEP_BLOCK - 1) / MESH_SWEEP_BLOCK)), block, stream, count - 1, count);
    }
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3_load(const float* __restrict__ p, long long i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ V3 v3_add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 v3_sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 v3_scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float v3_dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 v3_cross(V3 u, V3 v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }

// fn(s, f) for the sorted positions s of leaf k and the caller's face f = order[s], in ascending s: "the face met first stays"
template <class Fn>
__device__ __forceinline__ void mesh_leaf_faces(const MeshGeometry& g, long long k, Fn&& fn) {
    const long long s0 = k * g.leaf_size;
    for (int j = 0; j < g.leaf_size && s0 + j < g.n_faces; ++j) fn(s0 + j, (long long)g.order[s0 + j]);
}

__device__ __forceinline__ void mesh_face_corners(const MeshGeometry& g, long long f, V3& a, V3& b, V3& c) {
    a = v3_load(g.vertices, g.faces[3 * f]);
    b = v3_load(g.vertices, g.faces[3 * f + 1]);
    c = v3_load(g.vertices, g.faces[3 * f + 2]);
}

// N per-lane tallies of a query's work, for the microbenchmarks' builds of one file alone (-DNGP_MESH_TREE_COUNT); tally 0 is "boxes
// tested".  The product library has no counters: there the struct is empty and its calls are nothing.
#ifdef NGP_MESH_TREE_COUNT
static __device__ unsigned long long mesh_tree_counters[4];
template <int N>
struct MeshTally {
    unsigned long long n[N] = {};
    __device__ __forceinline__ void add(int i, int by = 1) { n[i] += by; }
    __device__ __forceinline__ void flush() const {
#pragma unroll
        for (int i = 0; i < N; ++i) atomicAdd(&mesh_tree_counters[i], n[i]);
    }
};
// read and clear
__host__ inline int mesh_tally_read(unsigned long long* out, int n) {
    const unsigned long long zero[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(mesh_tree_counters), n * sizeof(zero[0]));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(mesh_tree_counters), zero, n * sizeof(zero[0]));
    return -(int)e;
}
#define NGP_MESH_TALLY_ENTRY(name, N) int name(unsigned long long* out) { return ngp::mesh_tally_read(out, N); }
#else
template <int N>
struct MeshTally {
    __device__ __forceinline__ void add(int, int = 1) {}
    __device__ __forceinline__ void flush() const {}
};
#define NGP_MESH_TALLY_ENTRY(name, N)
#endif

}  // namespace ngp
