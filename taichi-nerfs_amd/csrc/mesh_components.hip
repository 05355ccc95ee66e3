// mesh_components.hip -- the pieces of a triangle mesh, for gfx950: a label per vertex and face, a table with one row per piece, and
// the sub-mesh of a set of pieces.  The contract is DESIGN.md section 3, "Connected components"; tests/mesh_components_reference.py
// restates it in numpy.  Two vertices are connected when some face names both (vertex connectivity).
//
// Labelling is a min-index union-find: parent[x] <= x ALWAYS (the start is parent[x] = x, an atomicMin only lowers and a compress
// stores an ancestor), so cc_find walks strictly downwards and ends for any contents of parent[].  A round is two launches:
//
//   cc_hook_kernel      one lane per face: the roots of its three vertices; every root above the smallest gets
//                       atomicMin(&parent[root], smallest) and changed[r] = 1
//   cc_compress_kernel  one lane per vertex: parent[v] = cc_find(v)
//
// No kernel waits for another workgroup's write.  A load may be served stale inside a launch; a stale value is an earlier value of the
// same slot, hence still an ancestor-or-self in the same piece, so a stale walk only ends early, on a vertex that is no root any more,
// and that lane's atomicMin then joins less than it could.  The host loop ends on the first hook pass that set no flag: such a pass ran
// no atomic at all, so parent[] did not move during the launch, every load was exact, and every face found one root for its three
// vertices.  A pass that sets the flag lowers a true root (the first atomic of the launch was issued by a lane that had read only
// unmodified slots), so the number of roots drops by at least one per changed pass: at most V passes in all (the host loop's cap).
// The skip tests (`changed[r - 1] == 0`, `changed[r] == 0`) read flags of EARLIER launches only.
//
//   cc_mark_kernel, cc_root_kernel, mesh_scan (mesh_scan.h), cc_assign_*_kernel   used vertices, root flags, the exclusive scan of the
//                       flags (a wave per 512 slots, one block over the chunk totals, the wave walk again) and the labels; bad faces
//                       and unused vertices are counted by mesh_wave_count
//   cc_edge_keys_kernel, cc_tally_*_kernel, cc_edge_kernel, cc_euler_kernel   the integer columns of the table: integer atomics,
//                       aggregated in the wave: one atomic per distinct component among its lanes (one component usually owns
//                       almost everything)
//   cc_measure_block_kernel, cc_measure_final_kernel   area, volume and box in a fixed order: faces sorted by (component, index) are
//                       cut into blocks of 64 per component, a wave sums a block by an xor tree, a wave sums a component's blocks
//                       (lane l takes l, l + 64, ... in order, then the same tree).  No float atomics: two runs write the same bytes.
//   cc_select_*_kernel, mesh_reindex_faces_kernel   keep flags, the same scan, and the gather through the two maps
//
// From mesh_edit.h: MESH_NO_KEY, mesh_face_indices with mesh_face_in_range (a good face here: a repeated index still joins; only the edge
// keys ask for mesh_face_distinct), MeshCarve (the workspace, cc_workspace), mesh_wave_count, mesh_run_head, mesh_area_vector,
// mesh_wave_sum, mesh_reindex_faces_kernel, mesh_blocks.
//
// Only integer atomicMin / atomicAdd and flag stores cross workgroups; their results do not depend on arrival order.
#include "ngp_device.h"
#include "mesh_edit.h"

namespace ngp {

constexpr int CC_BLOCK = 64;               // faces per block of the float sums: one per lane
constexpr int CC_COLS = 6;                 // int columns of the table: vertices, faces, edges, boundary, non-manifold, euler

struct CcPartial { double area, volume; int32_t lo[3], hi[3]; };         // 40 bytes; lo / hi as ordered keys (cc_key)

struct CcWorkspace {
    uint8_t* flags;       // [max(V, T)]: bit 0 used / kept, bit 1 root
    int32_t* chunk;       // [chunks(max(V, T))]: flagged slots per chunk, after the scan the index the chunk's first one gets
    int32_t* root_id;     // [V]: the number of the component whose root this vertex is, else -1
    long long bytes;
};
static CcWorkspace cc_workspace(void* base, long long n_faces, long long n_vertices) {
    const long long n = n_faces > n_vertices ? n_faces : n_vertices;
    MeshCarve c{(char*)base, 0};
    CcWorkspace w;
    w.flags = c.take<uint8_t>(n);
    w.chunk = c.take<int32_t>(mesh_scan_chunks(n));
    w.root_id = c.take<int32_t>(n_vertices);
    w.bytes = c.used;
    return w;
}

// a float's bits as an int that orders like the float, -0 below +0; its own inverse
__device__ __forceinline__ int32_t cc_key(int32_t bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

// the walk to the root.  Ends for ANY contents of parent[]: it goes on only to a strictly smaller non-negative index.
__device__ __forceinline__ int cc_find(const int32_t* parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)p >= (unsigned)x) return x;
        x = p;
    }
}

__global__ void __launch_bounds__(256) cc_hook_kernel(const int32_t* __restrict__ faces, int n_faces, int n_vertices, int32_t* parent,
                                                      int32_t* changed, int r) {
    if (r > 0 && changed[r - 1] == 0) return;              // the pass before this one (an earlier launch) already changed nothing
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    int idx[3];
    mesh_face_indices(faces, f, idx);
    if (!mesh_face_in_range(idx, n_vertices)) return;
    const int ra = cc_find(parent, idx[0]), rb = cc_find(parent, idx[1]), rc = cc_find(parent, idx[2]);
    const int m = min(ra, min(rb, rc));
    if (ra != m) atomicMin(&parent[ra], m);
    if (rb != m && rb != ra) atomicMin(&parent[rb], m);
    if (rc != m && rc != ra && rc != rb) atomicMin(&parent[rc], m);
    if (ra != m || rb != m || rc != m) changed[r] = 1;
}

__global__ void __launch_bounds__(256) cc_compress_kernel(int n_vertices, int32_t* parent, const int32_t* __restrict__ changed, int r) {
    if (changed[r] == 0) return;                           // this round's hook pass (an earlier launch) moved nothing
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    const int p = parent[v], root = cc_find(parent, (int)v);
    if (root != p) parent[v] = root;
}

__global__ void __launch_bounds__(256) cc_mark_kernel(const int32_t* __restrict__ faces, int n_faces, int n_vertices, uint8_t* flags,
                                                      int32_t* counts) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (f < n_faces) {
        int idx[3];
        mesh_face_indices(faces, f, idx);
        bad = !mesh_face_in_range(idx, n_vertices);
        if (!bad) flags[idx[0]] = flags[idx[1]] = flags[idx[2]] = 1;
    }
    mesh_wave_count(&counts[1], bad, threadIdx.x & 63);
}

__global__ void __launch_bounds__(256) cc_root_kernel(int n_vertices, const int32_t* __restrict__ parent, uint8_t* flags) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    if (flags[v] && parent[v] == (int)v) flags[v] = 3;
}

__global__ void __launch_bounds__(256) cc_assign_vertices_kernel(int n_vertices, const int32_t* __restrict__ parent,
                                                                 const uint8_t* __restrict__ flags, const int32_t* __restrict__ root_id,
                                                                 int32_t* __restrict__ vertex_component, int32_t* counts) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    bool unused = false;
    if (v < n_vertices) {
        unused = flags[v] == 0;
        const int p = parent[v];
        vertex_component[v] = !unused && (unsigned)p <= (unsigned)v ? root_id[p] : -1;
    }
    mesh_wave_count(&counts[2], unused, threadIdx.x & 63);
}

__global__ void __launch_bounds__(256) cc_assign_faces_kernel(const int32_t* __restrict__ faces, int n_faces, int n_vertices,
                                                              const int32_t* __restrict__ vertex_component,
                                                              int32_t* __restrict__ face_component) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    int idx[3];
    mesh_face_indices(faces, f, idx);
    face_component[f] = mesh_face_in_range(idx, n_vertices) ? vertex_component[idx[0]] : -1;
}

// ---- the integer columns of the table --------------------------------------------------------------------------------------------------
// table[comp][col] += 1 for every lane that is `on`, with ONE atomic per distinct component among those lanes: the first of them adds
// the number of lanes that share its component, those lanes leave, and so on -- at most 64 turns, one where a component owns the wave.
// (One atomic per lane made the table of a 2.5 M-face extraction take 27 ms: its floaters sit between the vertices of the large piece,
// so most waves are mixed, and every lane of the large piece hit the same word.)  Every lane of the wave calls it (on = false: no work).
__device__ __forceinline__ void cc_wave_add(int32_t* table, int col, int comp, bool on, int lane) {
    unsigned long long m = __ballot(on);                   // wave-uniform, and so is the loop
    while (m) {
        const int lead = __ffsll((long long)m) - 1;
        const int c0 = __shfl(comp, lead, 64);
        const unsigned long long same = __ballot(on && comp == c0);        // holds `lead`: m shrinks every turn
        if (lane == lead) atomicAdd(&table[(long long)CC_COLS * c0 + col], __popcll(same));
        m &= ~(same | (1ull << lead));
    }
}

__global__ void __launch_bounds__(256) cc_tally_kernel(const int32_t* __restrict__ component, long long n, int n_components, int col,
                                                       int32_t* table) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int comp = i < n ? component[i] : -1;
    cc_wave_add(table, col, comp, (unsigned)comp < (unsigned)n_components, threadIdx.x & 63);
}

// three keys per face, lo V + hi; MESH_NO_KEY for a bad face and for a face that repeats an index
__global__ void __launch_bounds__(256) cc_edge_keys_kernel(const int32_t* __restrict__ faces, int n_faces, int n_vertices,
                                                           long long* __restrict__ keys) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    int u[3];
    mesh_face_indices(faces, f, u);
    const bool counts = mesh_face_distinct(u, n_vertices);
    const int w[3] = {u[1], u[2], u[0]};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        keys[3 * f + k] = counts ? (long long)min(u[k], w[k]) * n_vertices + max(u[k], w[k]) : MESH_NO_KEY;
}

// over the SORTED keys: the first of a run of equal keys is the edge; it looks at most two slots ahead (used once, twice, more)
__global__ void __launch_bounds__(256) cc_edge_kernel(const long long* __restrict__ keys, long long n, int n_vertices, int n_components,
                                                      const int32_t* __restrict__ vertex_component, int32_t* table) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long k = i < n ? keys[i] : MESH_NO_KEY;
    bool head = k != MESH_NO_KEY && k >= 0 && mesh_run_head(keys, i);
    int comp = -1;
    bool twice = false, more = false;
    if (head) {
        const long long lo = k / n_vertices;
        comp = lo < n_vertices ? vertex_component[lo] : -1;
        head = (unsigned)comp < (unsigned)n_components;
        twice = i + 1 < n && keys[i + 1] == k;
        more = twice && i + 2 < n && keys[i + 2] == k;
    }
    const int lane = threadIdx.x & 63;
    cc_wave_add(table, 2, comp, head, lane);
    cc_wave_add(table, 3, comp, head && !twice, lane);
    cc_wave_add(table, 4, comp, head && more, lane);
}

__global__ void __launch_bounds__(256) cc_euler_kernel(int n_components, int32_t* table) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_components) return;
    table[CC_COLS * c + 5] = table[CC_COLS * c] - table[CC_COLS * c + 2] + table[CC_COLS * c + 1];
}

// ---- area, volume, box -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cc_wave_reduce(CcPartial& p) {
    p.area = mesh_wave_sum(p.area);
    p.volume = mesh_wave_sum(p.volume);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p.lo[k] = min(p.lo[k], __shfl_xor(p.lo[k], d, 64));
            p.hi[k] = max(p.hi[k], __shfl_xor(p.hi[k], d, 64));
        }
    }
}
__device__ __forceinline__ CcPartial cc_empty() { return {0.0, 0.0, {0x7fffffff, 0x7fffffff, 0x7fffffff}, {-0x7fffffff - 1, -0x7fffffff - 1, -0x7fffffff - 1}}; }

// a wave per block: block j of component c holds the sorted positions face_start[c] + [64 j, 64 j + 64) below face_start[c + 1]
__global__ void __launch_bounds__(256) cc_measure_block_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                               const long long* __restrict__ order, int n_faces, int n_vertices,
                                                               const int32_t* __restrict__ face_start,
                                                               const int32_t* __restrict__ block_start, int n_components,
                                                               CcPartial* __restrict__ partial) {
    const long long blk = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= block_start[n_components]) return;
    int lo = 0, hi = n_components;                          // the last c with block_start[c] <= blk: at most 31 halvings
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (block_start[mid] <= blk) lo = mid; else hi = mid;
    }
    const int lane = threadIdx.x & 63;
    const long long pos = (long long)face_start[lo] + (blk - block_start[lo]) * CC_BLOCK + lane;
    CcPartial p = cc_empty();
    if (pos < face_start[lo + 1] && pos < n_faces) {
        const long long f = order[pos];
        if (f >= 0 && f < n_faces) {
            int idx[3];
            mesh_face_indices(faces, f, idx);
            if (mesh_face_in_range(idx, n_vertices)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float fa = vertices[3ll * idx[0] + k], fb = vertices[3ll * idx[1] + k], fc = vertices[3ll * idx[2] + k];
                    const int32_t ka = cc_key(__float_as_int(fa)), kb = cc_key(__float_as_int(fb)), kc = cc_key(__float_as_int(fc));
                    p.lo[k] = min(ka, min(kb, kc));
                    p.hi[k] = max(ka, max(kb, kc));
                }
                double a[3], b[3], c[3], nn[3];
                p.area = 0.5 * sqrt(mesh_area_vector(vertices, idx, a, b, c, nn));
                const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
                p.volume = (a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2]) / 6.0;
            }
        }
    }
    cc_wave_reduce(p);
    if (lane == 0) partial[blk] = p;
}

// a wave per component: lane l adds the blocks l, l + 64, ... in that order, then the tree
__global__ void __launch_bounds__(256) cc_measure_final_kernel(const CcPartial* __restrict__ partial, const int32_t* __restrict__ block_start,
                                                               int n_components, double* __restrict__ area, double* __restrict__ volume,
                                                               float* __restrict__ lo, float* __restrict__ hi) {
    const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_components) return;
    const int lane = threadIdx.x & 63;
    CcPartial p = cc_empty();
    for (long long b = (long long)block_start[c] + lane; b < block_start[c + 1]; b += 64) {
        const CcPartial q = partial[b];
        p.area += q.area;
        p.volume += q.volume;
#pragma unroll
        for (int k = 0; k < 3; ++k) { p.lo[k] = min(p.lo[k], q.lo[k]); p.hi[k] = max(p.hi[k], q.hi[k]); }
    }
    cc_wave_reduce(p);
    if (lane == 0) {
        area[c] = p.area;
        volume[c] = p.volume;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[3 * c + k] = __int_as_float(cc_key(p.lo[k]));
            hi[3 * c + k] = __int_as_float(cc_key(p.hi[k]));
        }
    }
}

// ---- selection -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cc_select_flags_kernel(const int32_t* __restrict__ component, long long n,
                                                              const uint8_t* __restrict__ keep, int n_components, uint8_t* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = component[i];
    flags[i] = (unsigned)c < (unsigned)n_components && keep[c] ? 1 : 0;
}

__global__ void __launch_bounds__(256) cc_select_vertices_kernel(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                                 int n_vertices, const int32_t* __restrict__ vertex_map, int n_out,
                                                                 float* __restrict__ out_vertices, float* __restrict__ out_normals) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    const int m = vertex_map[v];
    if ((unsigned)m >= (unsigned)n_out) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_vertices[3ll * m + k] = vertices[3 * v + k];
        if (normals) out_normals[3ll * m + k] = normals[3 * v + k];
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" {

long long ngp_mesh_components_bytes(int n_faces, int n_vertices) {
    if (n_faces < 1 || n_vertices < 1) return -1;
    return cc_workspace(nullptr, n_faces, n_vertices).bytes;
}

int ngp_mesh_components_rounds(const int32_t* faces, int n_faces, int n_vertices, int32_t* parent, int32_t* changed, int n_rounds,
                               void* stream) {
    if (!faces || !parent || !changed || n_faces < 1 || n_vertices < 1 || n_rounds < 1) return -1;
    hipStream_t s = (hipStream_t)stream;
    for (int r = 0; r < n_rounds; ++r) {
        hipLaunchKernelGGL(cc_hook_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_vertices, parent, changed, r);
        hipLaunchKernelGGL(cc_compress_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, n_vertices, parent, changed, r);
    }
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_components_label(const int32_t* faces, int n_faces, int n_vertices, const int32_t* parent, void* workspace,
                              int32_t* vertex_component, int32_t* face_component, int32_t* counts, void* stream) {
    if (!faces || !parent || !workspace || !vertex_component || !face_component || !counts || n_faces < 1 || n_vertices < 1) return -1;
    const CcWorkspace w = cc_workspace(workspace, n_faces, n_vertices);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(w.flags, 0, (size_t)n_vertices, s);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 3 * sizeof(int32_t), s);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(cc_mark_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_vertices, w.flags, counts);
    hipLaunchKernelGGL(cc_root_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, n_vertices, parent, w.flags);
    mesh_scan(w.flags, 2, n_vertices, w.chunk, w.root_id, counts, s);
    hipLaunchKernelGGL(cc_assign_vertices_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, n_vertices, parent, w.flags, w.root_id,
                       vertex_component, counts);
    hipLaunchKernelGGL(cc_assign_faces_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_vertices, vertex_component,
                       face_component);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_components_edge_keys(const int32_t* faces, int n_faces, int n_vertices, int64_t* keys, void* stream) {
    if (!faces || !keys || n_faces < 1 || n_vertices < 1) return -1;
    hipLaunchKernelGGL(cc_edge_keys_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, (hipStream_t)stream, faces, n_faces, n_vertices,
                       (long long*)keys);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_components_table(int n_faces, int n_vertices, const int32_t* vertex_component, const int32_t* face_component,
                              const int64_t* sorted_keys, int n_components, int32_t* table, void* stream) {
    if (!vertex_component || !face_component || !sorted_keys || !table || n_faces < 1 || n_vertices < 1 || n_components < 1) return -1;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(table, 0, (size_t)n_components * CC_COLS * sizeof(int32_t), s);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(cc_tally_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, vertex_component, (long long)n_vertices,
                       n_components, 0, table);
    hipLaunchKernelGGL(cc_tally_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, s, face_component, (long long)n_faces, n_components, 1,
                       table);
    hipLaunchKernelGGL(cc_edge_kernel, dim3(mesh_blocks(3ll * n_faces, 256)), dim3(256), 0, s, (const long long*)sorted_keys, 3ll * n_faces,
                       n_vertices, n_components, vertex_component, table);
    hipLaunchKernelGGL(cc_euler_kernel, dim3(mesh_blocks(n_components, 256)), dim3(256), 0, s, n_components, table);
    NGP_LAUNCH_CHECK();
    return 0;
}

long long ngp_mesh_components_partial_bytes(int n_faces, int n_components) {
    if (n_faces < 1 || n_components < 1 || n_components > n_faces) return -1;
    return (long long)sizeof(CcPartial) * ((long long)n_faces / CC_BLOCK + n_components);
}

int ngp_mesh_components_measure(const float* vertices, const int32_t* faces, const int64_t* order, int n_faces, int n_vertices,
                                const int32_t* face_start, const int32_t* block_start, int n_components, void* partials, double* area,
                                double* volume, float* lo, float* hi, void* stream) {
    if (!vertices || !faces || !order || !face_start || !block_start || !partials || !area || !volume || !lo || !hi) return -1;
    if (ngp_mesh_components_partial_bytes(n_faces, n_components) < 0 || n_vertices < 1) return -1;
    hipStream_t s = (hipStream_t)stream;
    const long long blocks = (long long)n_faces / CC_BLOCK + n_components;            // sum of ceil(n_c / 64) is at most this
    hipLaunchKernelGGL(cc_measure_block_kernel, dim3(mesh_blocks(blocks, 4)), dim3(256), 0, s, vertices, faces, (const long long*)order,
                       n_faces, n_vertices, face_start, block_start, n_components, (CcPartial*)partials);
    hipLaunchKernelGGL(cc_measure_final_kernel, dim3(mesh_blocks(n_components, 4)), dim3(256), 0, s, (const CcPartial*)partials, block_start,
                       n_components, area, volume, lo, hi);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_select_count(int n_faces, int n_vertices, const int32_t* vertex_component, const int32_t* face_component,
                          const uint8_t* keep, int n_components, void* workspace, int32_t* vertex_map, int32_t* face_map,
                          int32_t* counts, void* stream) {
    if (!vertex_component || !face_component || !keep || !workspace || !vertex_map || !face_map || !counts) return -1;
    if (n_faces < 1 || n_vertices < 1 || n_components < 1) return -1;
    const CcWorkspace w = cc_workspace(workspace, n_faces, n_vertices);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_select_flags_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, vertex_component, (long long)n_vertices,
                       keep, n_components, w.flags);
    mesh_scan(w.flags, 1, n_vertices, w.chunk, vertex_map, counts, s);
    hipLaunchKernelGGL(cc_select_flags_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, s, face_component, (long long)n_faces, keep,
                       n_components, w.flags);
    mesh_scan(w.flags, 1, n_faces, w.chunk, face_map, counts + 1, s);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_select_emit(const float* vertices, const float* normals, const int32_t* faces, int n_faces, int n_vertices,
                         const int32_t* vertex_map, const int32_t* face_map, int n_out_vertices, int n_out_faces, float* out_vertices,
                         float* out_normals, int32_t* out_faces, void* stream) {
    if (!vertices || !faces || !vertex_map || !face_map || !out_vertices || !out_faces || (normals && !out_normals)) return -1;
    if (n_faces < 1 || n_vertices < 1 || n_out_vertices < 1 || n_out_faces < 1) return -1;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_select_vertices_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, s, vertices, normals, n_vertices,
                       vertex_map, n_out_vertices, out_vertices, out_normals);
    hipLaunchKernelGGL(mesh_reindex_faces_kernel, dim3(mesh_blocks(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_vertices, vertex_map,
                       face_map, n_out_faces, out_faces);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
