// mesh_simplify.hip -- a smaller mesh by vertex clustering with quadric error metrics, for gfx950 (Rossignac & Borrel's grid, Lindstrom
// 2000's quadric-optimal representative).  The contract is the comment above ngp_mesh_simplify_* in include/ngp_hip.h and DESIGN.md
// section 3, "Simplification"; tests/mesh_simplify_reference.py restates it serially.
//
//   ms_keys_kernel            a lane per vertex: the cell key (f32 subtract, multiply, floorf, clamp; exact int64 after that)
//       torch.sort (stable) of the V keys: plumbing
//   mesh_number_runs, ms_cluster_kernel                    the first slot of every run of equal keys, the run number of every slot
//                             (mesh_edit.h: mesh_run_heads_kernel, mesh_scan<true>), vertex_cluster through the sort's permutation
//   ms_faces_kernel           a lane per face: bad / survives; marks the clusters a surviving face names
//   mesh_scan x 2, ms_vertex_map_kernel                      face_map, the number of every marked cluster, vertex_map
//       ONE host read: {clusters, V', T', bad vertices, bad faces}
//   ms_incidence_keys_kernel  a lane per face: three keys, the corner's cluster or INT64_MAX
//       torch.sort (stable) of the 3 T keys: plumbing
//   ms_vertex_runs_kernel, ms_incidence_runs_kernel          where each cluster's run starts and ends in the two sorted lists
//   ms_solve_kernel           a WAVE per output vertex: lane l adds the terms l, l + 64, ... of the cluster's run in that order (twelve
//                             f64 sums per incidence, three per vertex), an xor tree over the 64 lanes, lane 0 solves the 3 x 3 system
//                             (LDL^T, the matrix is positive definite with condition <= (1 + eps) / eps) and writes position and normal
//   mesh_reindex_faces_kernel a lane per face: the surviving faces through the two maps
//
// From mesh_edit.h: MESH_NO_KEY, mesh_face_indices with mesh_face_in_range (a face that repeats an index is no bad face here: it has no
// area and does not survive), MeshCarve (the workspace, ms_workspace), mesh_wave_count, mesh_run_head / mesh_run_tail, mesh_number_runs,
// mesh_area_vector, mesh_wave_sum, mesh_reindex_faces_kernel, mesh_blocks.
//
// No float atomics: a sum's order depends on the sorted list alone, so two runs write the same bytes and a bad face elsewhere in the list
// moves no bit.  Integer atomics count the bad vertices and faces (one per wave); flag stores of the same value may race.
#include "ngp_device.h"
#include "mesh_edit.h"

namespace ngp {

constexpr int MS_MAX_CELLS = 1 << 21;                      // per axis: three of them fit 63 bits (not all three at once: ms_grid)

struct MsGrid { float lo[3], inv_h[3], h[3]; int n[3]; };
enum { MS_CLUSTERS = 0, MS_OUT_VERTICES = 1, MS_OUT_FACES = 2, MS_BAD_VERTICES = 3, MS_BAD_FACES = 4, MS_COUNTS = 5 };

struct MsWorkspace {
    uint8_t* vertex_flags;    // [V]: over sorted slots the first of a run; later, over cluster numbers, named by a surviving face
    uint8_t* face_flags;      // [T]: survives
    int32_t* chunk;           // [chunks(max(V, T))]
    long long bytes;
};
static MsWorkspace ms_workspace(void* base, long long n_faces, long long n_vertices) {
    MeshCarve c{(char*)base, 0};
    MsWorkspace w;
    w.vertex_flags = c.take<uint8_t>(n_vertices);
    w.face_flags = c.take<uint8_t>(n_faces);
    w.chunk = c.take<int32_t>(mesh_scan_chunks(n_faces > n_vertices ? n_faces : n_vertices));
    w.bytes = c.used;
    return w;
}

__global__ void __launch_bounds__(256) ms_keys_kernel(const float* __restrict__ vertices, int n_vertices, MsGrid g,
                                                      long long* __restrict__ keys, int32_t* counts) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (v < n_vertices) {
        long long q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = vertices[3 * v + k];
            bad = bad || !isfinite(x);
            float c = floorf((x - g.lo[k]) * g.inv_h[k]);                  // one subtraction, one multiplication (-ffp-contract=off)
            const float top = (float)(g.n[k] - 1);
            c = c > 0.0f ? c : 0.0f;                                       // clamped in float, before the conversion
            c = c < top ? c : top;
            q[k] = (long long)c;
        }
        keys[v] = bad ? MESH_NO_KEY : q[0] + (long long)g.n[0] * (q[1] + (long long)g.n[1] * q[2]);
    }
    mesh_wave_count(&counts[MS_BAD_VERTICES], bad, threadIdx.x & 63);
}

__global__ void __launch_bounds__(256) ms_cluster_kernel(const long long* __restrict__ sorted_keys, const long long* __restrict__ order,
                                                         const int32_t* __restrict__ run, int n_vertices,
                                                         int32_t* __restrict__ vertex_cluster) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vertices) return;
    const long long v = order[i];
    if (v >= 0 && v < n_vertices) vertex_cluster[v] = sorted_keys[i] != MESH_NO_KEY ? run[i] : -1;
}

// the clusters of a face's corners; false for a bad face (an index outside [0, V) or a bad vertex)
__device__ __forceinline__ bool ms_face_clusters(const int32_t* __restrict__ faces, long long f, int n_vertices,
                                                 const int32_t* __restrict__ vertex_cluster, int idx[3], int cl[3]) {
    mesh_face_indices(faces, f, idx);
    if (!mesh_face_in_range(idx, n_vertices)) return false;
    cl[0] = vertex_cluster[idx[0]]; cl[1] = vertex_cluster[idx[1]]; cl[2] = vertex_cluster[idx[2]];
    return cl[0] >= 0 && cl[1] >= 0 && cl[2] >= 0;
}

__global__ void __launch_bounds__(256) ms_faces_kernel(const int32_t* __restrict__ faces, int n_faces, int n_vertices,
                                                       const int32_t* __restrict__ vertex_cluster, uint8_t* __restrict__ face_flags,
                                                       uint8_t* cluster_flags, int32_t* counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (f < n_faces) {
        int idx[3], cl[3];
        bad = !ms_face_clusters(faces, f, n_vertices, vertex_cluster, idx, cl);
        const bool survives = !bad && cl[0] != cl[1] && cl[1] != cl[2] && cl[2] != cl[0];
        face_flags[f] = survives ? 1 : 0;
        if (survives) cluster_flags[cl[0]] = cluster_flags[cl[1]] = cluster_flags[cl[2]] = 1;      // cl < clusters <= V
    }
    mesh_wave_count(&counts[MS_BAD_FACES], bad, threadIdx.x & 63);
}

__global__ void __launch_bounds__(256) ms_vertex_map_kernel(const int32_t* __restrict__ vertex_cluster, const int32_t* __restrict__ cluster_out,
                                                            int n_vertices, int32_t* __restrict__ vertex_map) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    const int c = vertex_cluster[v];
    vertex_map[v] = (unsigned)c < (unsigned)n_vertices ? cluster_out[c] : -1;
}

// the keys and the sums decide "the face has area" by the one mesh_area_vector(...) > 0
__global__ void __launch_bounds__(256) ms_incidence_keys_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                int n_faces, int n_vertices, const int32_t* __restrict__ vertex_cluster,
                                                                long long* __restrict__ keys) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    int idx[3], cl[3];
    bool counts = ms_face_clusters(faces, f, n_vertices, vertex_cluster, idx, cl);
    if (counts) {
        double a[3], b[3], c[3], nn[3];
        counts = mesh_area_vector(vertices, idx, a, b, c, nn) > 0.0;
    }
    keys[3 * f] = counts ? (long long)cl[0] : MESH_NO_KEY;
    keys[3 * f + 1] = counts && cl[1] != cl[0] ? (long long)cl[1] : MESH_NO_KEY;
    keys[3 * f + 2] = counts && cl[2] != cl[0] && cl[2] != cl[1] ? (long long)cl[2] : MESH_NO_KEY;
}

// runs: int32 [4 C + V']: vertex run start [C], end [C], incidence run start [C], end [C] (zeroed: a cluster without incidences has the
// empty run), then the cluster of every output vertex [V']
__global__ void __launch_bounds__(256) ms_vertex_runs_kernel(const long long* __restrict__ sorted_keys, const long long* __restrict__ order,
                                                             const int32_t* __restrict__ vertex_cluster,
                                                             const int32_t* __restrict__ cluster_out, int n_vertices, int n_clusters,
                                                             int n_out, int32_t* __restrict__ runs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vertices) return;
    const long long k = sorted_keys[i];
    if (k == MESH_NO_KEY) return;
    const long long v = order[i];
    if (v < 0 || v >= n_vertices) return;
    const int c = vertex_cluster[v];
    if ((unsigned)c >= (unsigned)n_clusters) return;
    if (mesh_run_head(sorted_keys, i)) {
        runs[c] = (int)i;
        const int o = cluster_out[c];
        if ((unsigned)o < (unsigned)n_out) runs[4ll * n_clusters + o] = c;
    }
    if (mesh_run_tail(sorted_keys, i, n_vertices)) runs[(long long)n_clusters + c] = (int)i + 1;
}

__global__ void __launch_bounds__(256) ms_incidence_runs_kernel(const long long* __restrict__ sorted_keys, long long n, int n_clusters,
                                                                int32_t* __restrict__ runs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long k = sorted_keys[i];
    if (k < 0 || k >= n_clusters) return;                                   // MESH_NO_KEY
    if (mesh_run_head(sorted_keys, i)) runs[2ll * n_clusters + k] = (int)i;
    if (mesh_run_tail(sorted_keys, i, n)) runs[3ll * n_clusters + k] = (int)i + 1;
}

constexpr int MS_SUMS = 15;      // A (6: xx xy xz yy yz zz), b (3), area vector (3), sum of v - c (3)

__global__ void __launch_bounds__(256) ms_solve_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int n_faces,
                                                       int n_vertices, MsGrid g, const long long* __restrict__ vertex_keys,
                                                       const long long* __restrict__ vertex_order, const long long* __restrict__ inc_keys,
                                                       const long long* __restrict__ inc_order,
                                                       const int32_t* __restrict__ runs, int n_clusters, int n_out, double regularization,
                                                       float* __restrict__ out_vertices, float* __restrict__ out_normals) {
    const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n_out) return;                                                 // wave-uniform
    const int lane = threadIdx.x & 63;
    const int cl = runs[4ll * n_clusters + o];
    if ((unsigned)cl >= (unsigned)n_clusters) return;
    const int v0 = runs[cl], v1 = runs[(long long)n_clusters + cl], i0 = runs[2ll * n_clusters + cl], i1 = runs[3ll * n_clusters + cl];
    if (v0 < 0 || v1 > n_vertices || v0 >= v1 || i0 < 0 || i1 > 3ll * n_faces) return;
    long long key = vertex_keys[v0];
    double centre[3], half[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long q = k < 2 ? key % g.n[k] : key;
        key /= g.n[k];
        centre[k] = (double)g.lo[k] + ((double)q + 0.5) * (double)g.h[k];
        half[k] = 0.5 * (double)g.h[k];
    }
    double s[MS_SUMS];
#pragma unroll
    for (int j = 0; j < MS_SUMS; ++j) s[j] = 0.0;
    for (long long i = (long long)i0 + lane; i < i1; i += 64) {
        if (inc_keys[i] != cl) continue;
        const long long f = inc_order[i] / 3;
        if (f < 0 || f >= n_faces) continue;
        int idx[3];
        mesh_face_indices(faces, f, idx);
        if (!mesh_face_in_range(idx, n_vertices)) continue;
        double a[3], b[3], c[3], nn[3];
        const double len2 = mesh_area_vector(vertices, idx, a, b, c, nn);
        if (!(len2 > 0.0)) continue;
        const double len = sqrt(len2), w = 0.5 * len;
        const double n[3] = {nn[0] / len, nn[1] / len, nn[2] / len};
        const double d = -((n[0] * (a[0] - centre[0]) + n[1] * (a[1] - centre[1])) + n[2] * (a[2] - centre[2]));
        s[0] += w * n[0] * n[0]; s[1] += w * n[0] * n[1]; s[2] += w * n[0] * n[2];
        s[3] += w * n[1] * n[1]; s[4] += w * n[1] * n[2]; s[5] += w * n[2] * n[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s[6 + k] += w * d * n[k];
            s[9 + k] += 0.5 * nn[k];
        }
    }
    for (long long i = (long long)v0 + lane; i < v1; i += 64) {
        const long long v = vertex_order[i];
        if (v < 0 || v >= n_vertices) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) s[12 + k] += (double)vertices[3 * v + k] - centre[k];
    }
#pragma unroll
    for (int j = 0; j < MS_SUMS; ++j) s[j] = mesh_wave_sum(s[j]);
    if (lane != 0) return;
    const double count = (double)(v1 - v0);
    double y[3] = {s[12] / count, s[13] / count, s[14] / count};           // the mean: the answer without a quadric
    const double trace = (s[0] + s[3]) + s[5];
    if (trace > 0.0 && regularization < INFINITY) {
        // (A + mu I) y = -b + mu mean, mu = regularization tr(A): symmetric positive definite, so LDL^T without pivoting
        const double mu = regularization * trace;
        const double m00 = s[0] + mu, m01 = s[1], m02 = s[2], m11 = s[3] + mu, m12 = s[4], m22 = s[5] + mu;
        const double r0 = mu * y[0] - s[6], r1 = mu * y[1] - s[7], r2 = mu * y[2] - s[8];
        const double l10 = m01 / m00, l20 = m02 / m00;
        const double d1 = m11 - l10 * m01;
        const double t12 = m12 - l20 * m01;
        const double l21 = t12 / d1;
        const double d2 = (m22 - l20 * m02) - l21 * t12;
        const double z0 = r0, z1 = r1 - l10 * z0, z2 = (r2 - l20 * z0) - l21 * z1;
        y[2] = z2 / d2;
        y[1] = z1 / d1 - l21 * y[2];
        y[0] = (z0 / m00 - l10 * y[1]) - l20 * y[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double yk = y[k];
        yk = yk > -half[k] ? yk : -half[k];                                 // the representative stays in its cell
        yk = yk < half[k] ? yk : half[k];
        out_vertices[3 * o + k] = (float)(centre[k] + yk);
    }
    if (out_normals) {
        const double len = sqrt((s[9] * s[9] + s[10] * s[10]) + s[11] * s[11]);
#pragma unroll
        for (int k = 0; k < 3; ++k) out_normals[3 * o + k] = len > 0.0 ? (float)(s[9 + k] / len) : 0.0f;
    }
}

}  // namespace ngp

using namespace ngp;

// the host's grid -> the kernels' argument; false where the contract refuses it
static bool ms_grid(const float* lo, const float* inv_h, const float* h, const int32_t* n, MsGrid* g) {
    if (!lo || !inv_h || !h || !n) return false;
    for (int k = 0; k < 3; ++k) {
        if (!(lo[k] - lo[k] == 0.0f) || !(inv_h[k] > 0.0f) || !(inv_h[k] - inv_h[k] == 0.0f) || !(h[k] > 0.0f) || !(h[k] - h[k] == 0.0f)) return false;
        if (n[k] < 1 || n[k] > MS_MAX_CELLS) return false;
        g->lo[k] = lo[k]; g->inv_h[k] = inv_h[k]; g->h[k] = h[k]; g->n[k] = n[k];
    }
    // the last cell of a grid of 2^21 cells on every axis would have the key INT64_MAX, which is MESH_NO_KEY
    return !(n[0] == MS_MAX_CELLS && n[1] == MS_MAX_CELLS && n[2] == MS_MAX_CELLS);
}

extern "C" {

long long ngp_mesh_simplify_bytes(int n_faces, int n_vertices) {
    if (n_faces < 0 || n_vertices < 1) return -1;
    return ms_workspace(nullptr, n_faces, n_vertices).bytes;
}

int ngp_mesh_simplify_keys(const float* vertices, int n_vertices, const float* lo, const float* inv_h, const float* h, const int32_t* n,
                           int64_t* keys, int32_t* counts, void* stream) {
    MsGrid g;
    if (!vertices || !keys || !counts || n_vertices < 1 || !ms_grid(lo, inv_h, h, n, &g)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(counts, 0, MS_COUNTS * sizeof(int32_t), s);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(ms_keys_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, vertices, n_vertices, g, (long long*)keys, counts);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_simplify_count(const int32_t* faces, int n_faces, int n_vertices, const int64_t* sorted_keys, const int64_t* order,
                            void* workspace, int32_t* vertex_cluster, int32_t* cluster_out, int32_t* vertex_map, int32_t* face_map,
                            int32_t* counts, void* stream) {
    if (!sorted_keys || !order || !workspace || !vertex_cluster || !cluster_out || !vertex_map || !counts) return -1;
    if (n_faces < 0 || n_vertices < 1 || (n_faces > 0 && (!faces || !face_map))) return -1;
    const MsWorkspace w = ms_workspace(workspace, n_faces, n_vertices);
    hipStream_t s = (hipStream_t)stream;
    const unsigned vb = mesh_blocks(n_vertices, 256);
    mesh_number_runs((const long long*)sorted_keys, n_vertices, w.vertex_flags, w.chunk, vertex_map /* scratch until the end */,
                     counts + MS_CLUSTERS, s);
    hipLaunchKernelGGL(ms_cluster_kernel, dim3(vb), dim3(256), 0, s, (const long long*)sorted_keys, (const long long*)order, vertex_map,
                       n_vertices, vertex_cluster);
    const hipError_t e = hipMemsetAsync(w.vertex_flags, 0, (size_t)n_vertices, s);
    if (e != hipSuccess) return -(int)e;
    if (n_faces > 0) {
        hipLaunchKernelGGL(ms_faces_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_vertices, vertex_cluster,
                           w.face_flags, w.vertex_flags, counts);
        mesh_scan<false>(w.face_flags, 1, n_faces, w.chunk, face_map, counts + MS_OUT_FACES, s);
    }
    mesh_scan<false>(w.vertex_flags, 1, n_vertices, w.chunk, cluster_out, counts + MS_OUT_VERTICES, s);
    hipLaunchKernelGGL(ms_vertex_map_kernel, dim3(vb), dim3(256), 0, s, vertex_cluster, cluster_out, n_vertices, vertex_map);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_simplify_incidence_keys(const float* vertices, const int32_t* faces, int n_faces, int n_vertices,
                                     const int32_t* vertex_cluster, int64_t* keys, void* stream) {
    if (!vertices || !faces || !vertex_cluster || !keys || n_faces < 1 || n_vertices < 1) return -1;
    hipLaunchKernelGGL(ms_incidence_keys_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, (hipStream_t)stream, vertices, faces, n_faces,
                       n_vertices, vertex_cluster, (long long*)keys);
    NGP_LAUNCH_CHECK();
    return 0;
}

long long ngp_mesh_simplify_runs_bytes(int n_clusters, int n_out_vertices) {
    if (n_clusters < 1 || n_out_vertices < 1 || n_out_vertices > n_clusters) return -1;
    return 4 * (4ll * n_clusters + n_out_vertices);
}

int ngp_mesh_simplify_emit(const float* vertices, const int32_t* faces, int n_faces, int n_vertices, const float* lo, const float* inv_h,
                           const float* h, const int32_t* n, const int64_t* vertex_keys, const int64_t* vertex_order,
                           const int64_t* incidence_keys, const int64_t* incidence_order, const int32_t* vertex_cluster,
                           const int32_t* cluster_out, const int32_t* vertex_map, const int32_t* face_map, int n_clusters,
                           int n_out_vertices, int n_out_faces, double regularization, void* runs, float* out_vertices,
                           float* out_normals, int32_t* out_faces, void* stream) {
    MsGrid g;
    if (!vertices || !faces || !vertex_keys || !vertex_order || !incidence_keys || !incidence_order || !vertex_cluster || !cluster_out ||
        !vertex_map || !face_map || !runs || !out_vertices || !out_faces)
        return -1;
    if (n_faces < 1 || 3ll * n_faces > 0x7fffffffll || n_vertices < 1 || n_out_faces < 1 || n_out_faces > n_faces || n_clusters > n_vertices ||
        ngp_mesh_simplify_runs_bytes(n_clusters, n_out_vertices) < 0 || !(regularization > 0.0) || !ms_grid(lo, inv_h, h, n, &g))
        return -1;
    hipStream_t s = (hipStream_t)stream;
    int32_t* r = (int32_t*)runs;
    const hipError_t e = hipMemsetAsync(r, 0, (size_t)ngp_mesh_simplify_runs_bytes(n_clusters, n_out_vertices), s);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(ms_vertex_runs_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, (const long long*)vertex_keys,
                       (const long long*)vertex_order, vertex_cluster, cluster_out, n_vertices, n_clusters, n_out_vertices, r);
    hipLaunchKernelGGL(ms_incidence_runs_kernel, dim3(mesh_blocks(3ll * n_faces, 256)), dim3(256), 0, s, (const long long*)incidence_keys,
                       3ll * n_faces, n_clusters, r);
    hipLaunchKernelGGL(ms_solve_kernel, dim3(mesh_blocks(n_out_vertices, 4)), dim3(256), 0, s, vertices, faces, n_faces, n_vertices, g,
                       (const long long*)vertex_keys, (const long long*)vertex_order, (const long long*)incidence_keys,
                       (const long long*)incidence_order, r, n_clusters, n_out_vertices, regularization, out_vertices, out_normals);
    hipLaunchKernelGGL(mesh_reindex_faces_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_vertices, vertex_map, face_map,
                       n_out_faces, out_faces);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
