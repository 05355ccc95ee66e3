// mesh_edit.h -- what the mesh-editing files (mesh_components.hip, mesh_simplify.hip, mesh_smooth.hip) share, once.  They run one
// scheme: keys per face or vertex, torch.sort, the first slot of every run of equal keys flagged, mesh_scan (mesh_scan.h) numbering the
// runs, a kernel per run, results emitted through a vertex map and a face map.  Here: the key that sorts last, the two strengths of
// "is this face usable", the workspace carving, the wave count, the run-boundary tests and the run numbering, the bisection, the f64
// area vector, the f64 wave sum, the face re-index kernel and the block count.  Integer results depend on the input alone; the float
// helpers are evaluated as written (-ffp-contract=off), every operation a rounding of its own, in the order stated.
#pragma once
#include "ngp_device.h"
#include "mesh_scan.h"

namespace ngp {

constexpr long long MESH_NO_KEY = 0x7fffffffffffffffll;     // a slot that does not count: sorts behind every real key

static inline unsigned mesh_blocks(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// A workspace, carved front to back with every array on a 16-byte boundary.  Over a null base nothing is placed and `used` ends as the
// byte count: a file states its layout once, in one function, and its *_bytes entry reads `used` off that same function.
struct MeshCarve {
    char* base;
    long long used;
    template <typename T>
    T* take(long long count) {
        T* p = base ? (T*)(base + used) : nullptr;
        used += ((long long)sizeof(T) * count + 15) & ~15ll;
        return p;
    }
};

// ---- faces -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mesh_face_indices(const int32_t* __restrict__ faces, long long f, int idx[3]) {
    idx[0] = faces[3 * f]; idx[1] = faces[3 * f + 1]; idx[2] = faces[3 * f + 2];
}

// usable, the weak form: three indices inside [0, V).  A face that repeats an index passes.  (`&`, not `&&`: three compares and no
// branch, so the three index loads stay one load in front of the test.)
__device__ __forceinline__ bool mesh_face_in_range(const int idx[3], int n_vertices) {
    return ((unsigned)idx[0] < (unsigned)n_vertices) & ((unsigned)idx[1] < (unsigned)n_vertices) & ((unsigned)idx[2] < (unsigned)n_vertices);
}

// usable, the strong form: three indices inside [0, V), no two the same
__device__ __forceinline__ bool mesh_face_distinct(const int idx[3], int n_vertices) {
    return mesh_face_in_range(idx, n_vertices) & (idx[0] != idx[1]) & (idx[1] != idx[2]) & (idx[2] != idx[0]);
}

// the face's corners a, b, c in f64 and its doubled area vector nn = (b - a) x (c - a), every product and difference a rounding of its
// own; returns |nn|^2 = (x + y) + z, and the face has area iff that is > 0.  0.5 nn is the area vector, 0.5 sqrt(|nn|^2) the area.
__device__ __forceinline__ double mesh_area_vector(const float* __restrict__ vertices, const int idx[3], double a[3], double b[3],
                                                   double c[3], double nn[3]) {
    double u[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)vertices[3ll * idx[0] + k];
        b[k] = (double)vertices[3ll * idx[1] + k];
        c[k] = (double)vertices[3ll * idx[2] + k];
        u[k] = b[k] - a[k];
        w[k] = c[k] - a[k];
    }
    nn[0] = u[1] * w[2] - u[2] * w[1];
    nn[1] = u[2] * w[0] - u[0] * w[2];
    nn[2] = u[0] * w[1] - u[1] * w[0];
    return (nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2];
}

// out_faces[face_map[f]] = face f through vertex_map, for every f whose face_map is in [0, n_out): a mapped face is a usable face
static __global__ void __launch_bounds__(256) mesh_reindex_faces_kernel(const int32_t* __restrict__ faces, int n_faces, int n_vertices,
                                                                        const int32_t* __restrict__ vertex_map,
                                                                        const int32_t* __restrict__ face_map, int n_out,
                                                                        int32_t* __restrict__ out_faces) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const int m = face_map[f];
    if ((unsigned)m >= (unsigned)n_out) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = faces[3 * f + k];
        out_faces[3ll * m + k] = (unsigned)v < (unsigned)n_vertices ? vertex_map[v] : -1;
    }
}

// ---- the wave -------------------------------------------------------------------------------------------------------------------------
// *counter += the number of lanes with `on`: a ballot, then one integer atomic per wave.  EVERY lane of the wave calls it (a lane past
// the end of its array calls it with on = false): no early return in front of it.
__device__ __forceinline__ void mesh_wave_count(int32_t* counter, bool on, int lane) {
    const unsigned long long m = __ballot(on);
    if (m && lane == __ffsll((long long)m) - 1) atomicAdd(counter, __popcll(m));
}

// the sum of x over the 64 lanes, in every lane: the xor tree 32, 16, ... 1, a fixed order
__device__ __forceinline__ double mesh_wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// ---- sorted keys ----------------------------------------------------------------------------------------------------------------------
// slot i is the first / the last of its run of equal keys, i in [0, n)
__device__ __forceinline__ bool mesh_run_head(const long long* __restrict__ keys, long long i) { return i == 0 || keys[i - 1] != keys[i]; }
__device__ __forceinline__ bool mesh_run_tail(const long long* __restrict__ keys, long long i, long long n) {
    return i + 1 == n || keys[i + 1] != keys[i];
}

// the first slot of sorted_keys[0, n) whose key is >= target; n where there is none
__device__ __forceinline__ long long mesh_lower_bound(const long long* __restrict__ sorted_keys, long long n, long long target) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sorted_keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

static __global__ void __launch_bounds__(256) mesh_run_heads_kernel(const long long* __restrict__ sorted_keys, long long n,
                                                                    uint8_t* __restrict__ heads) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    heads[i] = sorted_keys[i] != MESH_NO_KEY && mesh_run_head(sorted_keys, i) ? 1 : 0;
}

// number the runs of a sorted key list: heads[i] = slot i is the first of a run of real keys, run[i] = the number of the run slot i lies
// in (-1 in front of the first), the number of runs to *total.  Four launches; chunk: int32 [mesh_scan_chunks(n)] of scratch.
static inline void mesh_number_runs(const long long* sorted_keys, long long n, uint8_t* heads, int32_t* chunk, int32_t* run, int32_t* total,
                                    hipStream_t s) {
    hipLaunchKernelGGL(mesh_run_heads_kernel, dim3(mesh_blocks(n, 256)), dim3(256), 0, s, sorted_keys, n, heads);
    mesh_scan<true>(heads, 1, n, chunk, run, total, s);
}

}  // namespace ngp
