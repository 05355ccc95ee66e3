// mesh_smooth.hip -- the vertex adjacency of a triangle mesh (CSR, built on the device), Taubin's lambda | mu smoothing over it with a
// bounded displacement, and area-weighted vertex normals, for gfx950.  The contract is the comment above ngp_mesh_adjacency_* in
// include/ngp_hip.h and DESIGN.md section 3, "Smoothing"; tests/mesh_smooth_reference.py restates it serially.
//
//   sm_edge_keys_kernel       a lane per face: six directed keys u V + w (both directions of the three edges), INT64_MAX for a bad face
//       torch.sort of the 6 T keys: plumbing
//   mesh_number_runs          the first slot of every run of equal keys, the run number of every slot (mesh_edit.h: mesh_run_heads_kernel,
//                             mesh_scan<true>); the number of runs is E2
//   sm_build_kernel           a lane per slot: the head of run e writes neighbours[e] = key mod V and multiplicity[e] = the run's length,
//                             walked forward and cut at 255
//   sm_rows_kernel            a lane per row bound: row_start[v] = the run at the lower bound of v V in the sorted keys (mesh_lower_bound)
//   sm_vertex_flags_kernel    a lane per vertex: boundary / non-manifold / unused from its row, bad from its coordinates; two counters
//   sm_pass_kernel<CLAMP>     a lane per vertex: the serial row walk, three f64 sums in ascending neighbour order, one division, the update,
//                             the rounding to f32 and the f32 clamp around x0.  Ping-pong: it reads x_in and writes x_out.
//   sm_normal_keys_kernel     a lane per face: three incidence keys, the corner's vertex or INT64_MAX
//       torch.sort (stable) of the 3 T keys: plumbing
//   sm_normals_kernel         a lane per vertex: mesh_lower_bound finds its run, the f64 area vectors (mesh_area_vector) are summed in
//                             ascending slot order
//
// From mesh_edit.h: MESH_NO_KEY, mesh_face_indices with mesh_face_distinct (a good face here: in range AND no repeated index), MeshCarve
// (the workspace, sm_workspace), mesh_wave_count, mesh_run_tail, mesh_number_runs, mesh_lower_bound, mesh_area_vector, mesh_blocks.
//
// The f64 expressions are evaluated as written: the library is compiled with -ffp-contract=off (HIPCC_FLAGS in ngp_hip/lib.py), so
// x + factor * (m - x) is a subtraction, a multiplication and an addition with a rounding each, never an fma; no fast-math flag is
// given, so the f64 division and square root are the correctly rounded ones.
// No float atomics: every sum's order is fixed by the sorted keys, so two runs write the same bytes.  Integer atomics count (one per
// wave); the adjacency is integer arithmetic only and depends on the set of faces alone.
#include "ngp_device.h"
#include "mesh_edit.h"

namespace ngp {

constexpr int SM_MAX_MULTIPLICITY = 255;                    // multiplicity is uint8 and saturates here
enum { SM_EDGES = 0, SM_BAD_FACES = 1, SM_BAD_VERTICES = 2, SM_BOUNDARY_VERTICES = 3, SM_COUNTS = 4 };
enum { SM_BOUNDARY = 1, SM_NONMANIFOLD = 2, SM_UNUSED = 4, SM_BAD = 8 };

struct SmWorkspace {
    int32_t* run;             // [6 T]: the run number of every sorted slot
    uint8_t* heads;           // [6 T]: the first slot of a run
    int32_t* chunk;           // [chunks(6 T)]
    long long bytes;
};
static SmWorkspace sm_workspace(void* base, long long n_keys) {
    MeshCarve c{(char*)base, 0};
    SmWorkspace w;
    w.run = c.take<int32_t>(n_keys);
    w.heads = c.take<uint8_t>(n_keys);
    w.chunk = c.take<int32_t>(mesh_scan_chunks(n_keys));
    w.bytes = c.used;
    return w;
}

// six directed keys per face, u V + w < V^2 < 2^62: MESH_NO_KEY (a bad face's slots) sorts behind them
__global__ void __launch_bounds__(256) sm_edge_keys_kernel(const int32_t* __restrict__ faces, int n_faces, int n_vertices,
                                                           long long* __restrict__ keys, int32_t* counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (f < n_faces) {
        int u[3];
        mesh_face_indices(faces, f, u);
        bad = !mesh_face_distinct(u, n_vertices);
        const int w[3] = {u[1], u[2], u[0]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            keys[6 * f + 2 * k] = bad ? MESH_NO_KEY : (long long)u[k] * n_vertices + w[k];
            keys[6 * f + 2 * k + 1] = bad ? MESH_NO_KEY : (long long)w[k] * n_vertices + u[k];
        }
    }
    mesh_wave_count(&counts[SM_BAD_FACES], bad, threadIdx.x & 63);
}

__global__ void __launch_bounds__(256) sm_build_kernel(const long long* __restrict__ sorted_keys, const uint8_t* __restrict__ heads,
                                                       const int32_t* __restrict__ run, long long n, int n_vertices,
                                                       int32_t* __restrict__ neighbours, uint8_t* __restrict__ multiplicity) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !heads[i]) return;
    const long long k = sorted_keys[i];
    const int e = run[i];
    if ((unsigned long long)e >= (unsigned long long)n) return;             // neighbours and multiplicity hold n = 6 T slots
    int m = 1;
    while (m < SM_MAX_MULTIPLICITY && !mesh_run_tail(sorted_keys, i + m - 1, n)) ++m;
    neighbours[e] = (int)(k % n_vertices);
    multiplicity[e] = (uint8_t)m;
}

// row_start[v], v in [0, V]: the number of the run at the first slot whose key is >= v V; E2 where that slot holds no real key
__global__ void __launch_bounds__(256) sm_rows_kernel(const long long* __restrict__ sorted_keys, const int32_t* __restrict__ run,
                                                      long long n, int n_vertices, const int32_t* __restrict__ counts,
                                                      int32_t* __restrict__ row_start) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v > n_vertices) return;
    const long long lo = mesh_lower_bound(sorted_keys, n, v * n_vertices);  // the target is <= V^2 < 2^62
    row_start[v] = lo < n && sorted_keys[lo] != MESH_NO_KEY ? run[lo] : counts[SM_EDGES];
}

__global__ void __launch_bounds__(256) sm_vertex_flags_kernel(const float* __restrict__ vertices, int n_vertices,
                                                              const int32_t* __restrict__ row_start,
                                                              const uint8_t* __restrict__ multiplicity, long long n_slots,
                                                              uint8_t* __restrict__ vertex_flags, int32_t* counts) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    int flags = 0;
    if (v < n_vertices) {
        const float x = vertices[3 * v], y = vertices[3 * v + 1], z = vertices[3 * v + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) flags |= SM_BAD;
        long long e0 = row_start[v], e1 = row_start[v + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > n_slots ? n_slots : e1;
        if (e0 >= e1) flags |= SM_UNUSED;
        for (long long e = e0; e < e1; ++e) {
            const int m = multiplicity[e];
            if (m == 1) flags |= SM_BOUNDARY;
            if (m >= 3) flags |= SM_NONMANIFOLD;
        }
        vertex_flags[v] = (uint8_t)flags;
    }
    const int lane = threadIdx.x & 63;
    mesh_wave_count(&counts[SM_BAD_VERTICES], flags & SM_BAD, lane);
    mesh_wave_count(&counts[SM_BOUNDARY_VERTICES], flags & SM_BOUNDARY, lane);
}

struct SmMove { float v[3]; };

template <bool CLAMP>
__global__ void __launch_bounds__(256) sm_pass_kernel(const float* __restrict__ x_in, const float* __restrict__ x0,
                                                      const int32_t* __restrict__ row_start, const int32_t* __restrict__ neighbours,
                                                      const uint8_t* __restrict__ multiplicity, const uint8_t* __restrict__ vertex_flags,
                                                      const uint8_t* __restrict__ fixed, int n_vertices, long long n_slots, double factor,
                                                      int boundary_mode, SmMove max_move, float* __restrict__ x_out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    const float x[3] = {x_in[3 * v], x_in[3 * v + 1], x_in[3 * v + 2]};
    float out[3] = {x[0], x[1], x[2]};
    const int flags = vertex_flags[v];
    const bool boundary = flags & SM_BOUNDARY;
    bool moves = !(flags & (SM_UNUSED | SM_BAD)) && !(fixed && fixed[v]) && !(boundary_mode == NGP_MESH_SMOOTH_FIXED && boundary);
    if (moves) {
        const bool along = boundary_mode == NGP_MESH_SMOOTH_CURVE && boundary;       // a boundary vertex: across boundary edges only
        long long e0 = row_start[v], e1 = row_start[v + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > n_slots ? n_slots : e1;
        double s[3] = {0.0, 0.0, 0.0};
        int count = 0;
        for (long long e = e0; e < e1; ++e) {                                        // ascending neighbour index: the row's order
            const int j = neighbours[e];
            if ((unsigned)j >= (unsigned)n_vertices || (vertex_flags[j] & SM_BAD)) continue;
            if (along && multiplicity[e] != 1) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] += (double)x_in[3ll * j + k];
            ++count;
        }
        if (count > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double xi = (double)x[k];
                const double m = s[k] / (double)count;
                const double y = xi + factor * (m - xi);
                float r = (float)y;
                if (CLAMP) {
                    const float o = x0[3 * v + k];
                    const float lo = o - max_move.v[k], hi = o + max_move.v[k];
                    r = r < lo ? lo : r;
                    r = r > hi ? hi : r;
                }
                out[k] = r;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) x_out[3 * v + k] = out[k];
}

__global__ void __launch_bounds__(256) sm_normal_keys_kernel(const int32_t* __restrict__ faces, int n_faces, int n_vertices,
                                                             long long* __restrict__ keys) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    int idx[3];
    mesh_face_indices(faces, f, idx);
    const bool good = mesh_face_distinct(idx, n_vertices);
#pragma unroll
    for (int k = 0; k < 3; ++k) keys[3 * f + k] = good ? (long long)idx[k] : MESH_NO_KEY;
}

__global__ void __launch_bounds__(256) sm_normals_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int n_faces,
                                                         int n_vertices, const long long* __restrict__ sorted_keys,
                                                         const long long* __restrict__ order, float* __restrict__ normals) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    const long long n = 3ll * n_faces;
    double s[3] = {0.0, 0.0, 0.0};
    for (long long i = mesh_lower_bound(sorted_keys, n, v); i < n && sorted_keys[i] == v; ++i) {      // ascending slot: the sort is stable
        const long long f = order[i] / 3;
        if (f < 0 || f >= n_faces) continue;
        int idx[3];
        mesh_face_indices(faces, f, idx);
        if (!mesh_face_distinct(idx, n_vertices)) continue;
        double a[3], b[3], c[3], nn[3];
        mesh_area_vector(vertices, idx, a, b, c, nn);
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += 0.5 * nn[k];
    }
    const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    const bool ok = len > 0.0 && len < INFINITY;                                      // false for a NaN too
#pragma unroll
    for (int k = 0; k < 3; ++k) normals[3 * v + k] = ok ? (float)(s[k] / len) : 0.0f;
}

}  // namespace ngp

using namespace ngp;

static bool sm_sizes_ok(int n_faces, int n_vertices) { return n_vertices >= 1 && n_faces >= 1 && 6ll * n_faces <= 0x7fffffffll; }

extern "C" {

long long ngp_mesh_adjacency_bytes(int n_faces) {
    if (n_faces < 1 || 6ll * n_faces > 0x7fffffffll) return -1;
    return sm_workspace(nullptr, 6ll * n_faces).bytes;
}

int ngp_mesh_adjacency_keys(const int32_t* faces, int n_faces, int n_vertices, int64_t* keys, int32_t* counts, void* stream) {
    if (!faces || !keys || !counts || !sm_sizes_ok(n_faces, n_vertices)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(counts, 0, SM_COUNTS * sizeof(int32_t), s);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(sm_edge_keys_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_vertices, (long long*)keys, counts);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_adjacency_build(const float* vertices, int n_faces, int n_vertices, const int64_t* sorted_keys, void* workspace,
                             int32_t* row_start, int32_t* neighbours, uint8_t* multiplicity, uint8_t* vertex_flags, int32_t* counts,
                             void* stream) {
    if (!vertices || !sorted_keys || !workspace || !row_start || !neighbours || !multiplicity || !vertex_flags || !counts ||
        !sm_sizes_ok(n_faces, n_vertices))
        return -1;
    const long long n = 6ll * n_faces;
    const SmWorkspace w = sm_workspace(workspace, n);
    hipStream_t s = (hipStream_t)stream;
    const long long* keys = (const long long*)sorted_keys;
    mesh_number_runs(keys, n, w.heads, w.chunk, w.run, counts + SM_EDGES, s);
    hipLaunchKernelGGL(sm_build_kernel, dim3(mesh_blocks(n, 256)), dim3(256), 0, s, keys, w.heads, w.run, n, n_vertices, neighbours, multiplicity);
    hipLaunchKernelGGL(sm_rows_kernel, dim3(mesh_blocks((long long)n_vertices + 1, 256)), dim3(256), 0, s, keys, w.run, n, n_vertices, counts,
                       row_start);
    hipLaunchKernelGGL(sm_vertex_flags_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, vertices, n_vertices, row_start, multiplicity,
                       n, vertex_flags, counts);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_smooth(float* x_a, float* x_b, const float* x0, const int32_t* row_start, const int32_t* neighbours,
                    const uint8_t* multiplicity, const uint8_t* vertex_flags, const uint8_t* fixed, int n_vertices, long long n_slots,
                    int n_iterations, double lambda, double mu, int boundary_mode, const float* max_move, void* stream) {
    if (!x_a || !x_b || x_a == x_b || !row_start || !neighbours || !multiplicity || !vertex_flags || !max_move) return -1;
    if (n_vertices < 1 || n_slots < 0 || n_slots > 0x7fffffffll || n_iterations < 0) return -1;
    if (!(lambda - lambda == 0.0) || !(mu - mu == 0.0)) return -1;
    if (boundary_mode != NGP_MESH_SMOOTH_FIXED && boundary_mode != NGP_MESH_SMOOTH_CURVE && boundary_mode != NGP_MESH_SMOOTH_FREE) return -1;
    SmMove mm;
    bool clamp = false;
    for (int k = 0; k < 3; ++k) {
        if (!(max_move[k] >= 0.0f)) return -1;                                        // negative or NaN
        mm.v[k] = max_move[k];
        clamp = clamp || max_move[k] < INFINITY;
    }
    if (clamp && (!x0 || x0 == x_a || x0 == x_b)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const int per_iteration = mu == 0.0 ? 1 : 2;
    float *in = x_a, *out = x_b;
    for (long long p = 0; p < (long long)n_iterations * per_iteration; ++p) {
        const double factor = per_iteration == 2 && (p & 1) ? mu : lambda;
        if (clamp)
            hipLaunchKernelGGL(sm_pass_kernel<true>, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, in, x0, row_start, neighbours, multiplicity,
                               vertex_flags, fixed, n_vertices, n_slots, factor, boundary_mode, mm, out);
        else
            hipLaunchKernelGGL(sm_pass_kernel<false>, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, in, x0, row_start, neighbours, multiplicity,
                               vertex_flags, fixed, n_vertices, n_slots, factor, boundary_mode, mm, out);
        float* t = in; in = out; out = t;
    }
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_vertex_normals_keys(const int32_t* faces, int n_faces, int n_vertices, int64_t* keys, void* stream) {
    if (!faces || !keys || !sm_sizes_ok(n_faces, n_vertices)) return -1;
    hipLaunchKernelGGL(sm_normal_keys_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, (hipStream_t)stream, faces, n_faces, n_vertices,
                       (long long*)keys);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_vertex_normals(const float* vertices, const int32_t* faces, int n_faces, int n_vertices, const int64_t* sorted_keys,
                            const int64_t* order, float* normals, void* stream) {
    if (!vertices || !faces || !sorted_keys || !order || !normals || !sm_sizes_ok(n_faces, n_vertices)) return -1;
    hipLaunchKernelGGL(sm_normals_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream, vertices, faces, n_faces,
                       n_vertices, (const long long*)sorted_keys, (const long long*)order, normals);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
