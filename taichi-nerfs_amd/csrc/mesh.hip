// mesh.hip -- isosurface extraction from a sampled scalar field by marching tetrahedra, for gfx950.  The contract (inside rule, vertex
// and face order, winding) is DESIGN.md section 3, "Isosurface extraction"; tests/mesh_reference.py restates it in numpy.
//
// Every cell is split into the six Kuhn tetrahedra, so every mesh vertex lies on an edge p -> p + d, d in {0,1}^3 \ {0}: seven edge
// types e = 4 dx + 2 dy + dz, each owned by its lower grid point p.  That makes an INDEXED mesh possible without a map, a sort or an
// atomic: the id of the vertex on edge e of point q is base(q) + popcount(mask(q) & ((1 << e) - 1)).
//
//   mesh_count_kernel          one lane per grid point, z fastest; a wave walks MESH_CHUNK consecutive points.  Per point: the 7-bit
//                              vertex mask, the triangle count of the cell it is the minimum corner of (<= 12) and the vertex rank
//                              inside the chunk (u16); per chunk: (vertices, triangles).
//   mesh_scan_kernel           one block: exclusive scan of the chunk totals in place, totals to counts[2]
//   mesh_emit_vertices_kernel  one lane per grid point: position (and normal) of each vertex the point owns, at base + rank
//   mesh_emit_faces_kernel     the count kernel's walk again: a wave scans the stored triangle counts and the cells that have any
//                              write their faces at the chunk's base + rank
//
// The eight corner values of a point are read straight from global memory: along z they are the neighbouring lanes' values; the rows
// j + 1, i + 1 are EXPECTED to come back from L2 (a z-y plane of a 513^3 grid is 1 MB), so that HBM sees each value about once -- an
// assumption, no counter run has checked it.  An LDS tile with a halo would have to be three-dimensional, while the vertex order the
// contract asks for is the linear one the wave walk gives for free.
// Workspace: 4 bytes per point (mask 1, triangle count 1, rank 2) + 8 bytes per chunk.  No atomics of any kind: two launches on the same
// input write the same bytes.
#include "ngp_device.h"

namespace ngp {

constexpr int MESH_CHUNK = 512;            // points per wave: 8 rounds of 64 lanes; at most 7 * 512 vertices, so the rank fits 16 bits
constexpr int MESH_SCAN_THREADS = 256;     // the scan block; thread t owns a run of ceil(chunks / 256) consecutive chunk totals

struct MeshGrid {
    int nx, ny, nz, n;
    float iso;
    int sign;
};
struct MeshWorkspace {
    int2* chunk;          // [chunks]: (vertices, triangles) of the chunk, after the scan the ids its first vertex and face get
    uint16_t* rank;       // [n]: vertices owned by earlier points of the same chunk
    uint8_t* mask;        // [n]: bit e = edge type e of this point carries a vertex
    uint8_t* tris;        // [n]: triangles of the cell whose minimum corner this point is
};
__host__ __device__ __forceinline__ long long mesh_chunks(long long n) { return (n + MESH_CHUNK - 1) / MESH_CHUNK; }
__host__ __device__ __forceinline__ long long mesh_align16(long long b) { return (b + 15) & ~15ll; }
__host__ __forceinline__ MeshWorkspace mesh_workspace(void* base, long long n) {
    char* p = (char*)base;
    MeshWorkspace w;
    w.chunk = (int2*)p;      p += mesh_align16(8 * mesh_chunks(n));
    w.rank = (uint16_t*)p;   p += mesh_align16(2 * n);
    w.mask = (uint8_t*)p;    p += mesh_align16(n);
    w.tris = (uint8_t*)p;
    return w;
}

// local corners 0..3 of the tetrahedron of axis permutation pi (lexicographic order) as offset codes 4 dx + 2 dy + dz:
// c, c + e_pi0, c + e_pi0 + e_pi1, c + (1,1,1).  Permutations 1, 2 and 5 are odd: their tetrahedra are mirror images.
__device__ constexpr int MESH_TET[6][4] = {{0, 4, 6, 7}, {0, 4, 5, 7}, {0, 2, 6, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 1, 3, 7}};
// the six edges of a tetrahedron as pairs of local corners, lower first (the lower corner's grid point owns the edge)
__device__ constexpr int MESH_EDGE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// triangles of a tetrahedron of an EVEN permutation by its four inside bits (bit n = local corner n): bits 0-1 the triangle count,
// then up to six 3-bit edge numbers.  One corner apart from the other three: a triangle on its three edges, the others ascending;
// two inside A < B, two outside C < D: (AC, AD, BD), (AC, BD, BC); the second and third vertex swapped where that order is clockwise
// seen from the outside.  An odd permutation swaps them once more.  Purely combinatorial: no geometry decides a winding.
__device__ constexpr uint32_t MESH_CASE[16] = {0x00000, 0x00221, 0x00381, 0x70c46, 0x00565, 0xac2a2, 0x34582, 0x00589,
                                               0x004a9, 0x94522, 0xa83a2, 0x003a5, 0x50c66, 0x00461, 0x00141, 0x00000};

__device__ __forceinline__ bool mesh_inside(float v, const MeshGrid& g) { return g.sign > 0 ? v > g.iso : v < g.iso; }   // NaN: outside
__device__ __forceinline__ void mesh_ijk(int p, const MeshGrid& g, int& i, int& j, int& k) {
    const int r = p / g.nz;
    k = p - r * g.nz;
    i = r / g.ny;
    j = r - i * g.ny;
}
__device__ __forceinline__ int mesh_offset(int code, const MeshGrid& g) {
    return ((code >> 2) & 1) * g.ny * g.nz + ((code >> 1) & 1) * g.nz + (code & 1);
}
// inside bits of the eight corners p + code (bit `code`), zero where the corner is off the grid; on_grid: which corners exist
__device__ __forceinline__ uint32_t mesh_corner_bits(const float* __restrict__ v, int p, const MeshGrid& g, uint32_t& on_grid) {
    int i, j, k;
    mesh_ijk(p, g, i, j, k);
    const bool ok[3] = {i + 1 < g.nx, j + 1 < g.ny, k + 1 < g.nz};
    uint32_t in = 0;
    on_grid = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool here = (!(c & 4) || ok[0]) && (!(c & 2) || ok[1]) && (!(c & 1) || ok[2]);
        if (here) {
            on_grid |= 1u << c;
            if (mesh_inside(v[p + mesh_offset(c, g)], g)) in |= 1u << c;
        }
    }
    return in;
}
__device__ __forceinline__ uint32_t mesh_tet_bits(uint32_t in, int pi) {
    return ((in >> MESH_TET[pi][0]) & 1u) | (((in >> MESH_TET[pi][1]) & 1u) << 1) | (((in >> MESH_TET[pi][2]) & 1u) << 2) |
           (((in >> MESH_TET[pi][3]) & 1u) << 3);
}

__global__ void __launch_bounds__(256) mesh_count_kernel(const float* __restrict__ v, MeshGrid g, MeshWorkspace w) {
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long first = wave * MESH_CHUNK;
    if (first >= g.n) return;
    const int lo = (int)first, hi = (int)min(first + MESH_CHUNK, (long long)g.n), lane = threadIdx.x & 63;
    int v_run = 0, t_run = 0;
    for (int r = 0; r < MESH_CHUNK / 64 && lo + 64 * r < hi; ++r) {         // lo <= 2^31 - 512: lo + 64 r cannot wrap
        const int p0 = lo + 64 * r;
        const bool live = lane < hi - p0;
        const int p = live ? p0 + lane : p0;                       // n can be 2^31 - 1: never form an index past it
        uint32_t mask = 0;
        int tris = 0;
        if (live) {
            uint32_t on_grid;
            const uint32_t in = mesh_corner_bits(v, p, g, on_grid);
            mask = (in ^ ((in & 1u) ? 0xffu : 0u)) & on_grid & 0xfeu;      // edge e: p + e on the grid and on the other side of iso
            if (on_grid == 0xffu) {
#pragma unroll
                for (int pi = 0; pi < 6; ++pi) tris += (int)(MESH_CASE[mesh_tet_bits(in, pi)] & 3u);
            }
            w.mask[p] = (uint8_t)mask;
            w.tris[p] = (uint8_t)tris;
        }
        const int mine = __popc(mask);
        const int incl = wave_scan_add_i(mine, lane);
        if (live) w.rank[p] = (uint16_t)(v_run + incl - mine);
        v_run += __shfl(incl, 63, 64);
        t_run += wave_sum_i(tris);
    }
    if (lane == 0) w.chunk[wave] = make_int2(v_run, t_run);
}

// exclusive scan of the chunk totals, in place.  Thread t sums the run [t R, (t + 1) R) of R = ceil(chunks / 256) totals, the 256 sums
// are scanned across the block, and the thread walks its run again.  64-bit sums: 7 n vertices or 12 n triangles can pass 2^31, and
// then counts = {-1, -1} (the ids of the mesh are int32) instead of a wrapped number.
__global__ void __launch_bounds__(MESH_SCAN_THREADS) mesh_scan_kernel(int2* __restrict__ chunk, long long chunks, int32_t* __restrict__ counts) {
    __shared__ long long part[2][MESH_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long long run = (chunks + MESH_SCAN_THREADS - 1) / MESH_SCAN_THREADS;
    const long long lo = min(t * run, chunks), hi = min(lo + run, chunks);
    long long sv = 0, st = 0;
#pragma unroll 8
    for (long long c = lo; c < hi; ++c) { const int2 x = chunk[c]; sv += x.x; st += x.y; }
    long long iv = sv, it = st;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long uv = __shfl_up(iv, d, 64), ut = __shfl_up(it, d, 64);
        if (lane >= d) { iv += uv; it += ut; }
    }
    if (lane == 63) { part[0][wv] = iv; part[1][wv] = it; }
    __syncthreads();
    long long bv = 0, bt = 0, tv = 0, tt = 0;
#pragma unroll
    for (int k = 0; k < MESH_SCAN_THREADS / 64; ++k) {
        if (k < wv) { bv += part[0][k]; bt += part[1][k]; }
        tv += part[0][k]; tt += part[1][k];
    }
    const bool fits = tv <= 0x7fffffffll && tt <= 0x7fffffffll;
    if (t == 0) { counts[0] = fits ? (int32_t)tv : -1; counts[1] = fits ? (int32_t)tt : -1; }
    if (!fits) return;
    long long av = bv + iv - sv, at = bt + it - st;
    for (long long c = lo; c < hi; ++c) {
        const int2 x = chunk[c];
        chunk[c] = make_int2((int)av, (int)at);
        av += x.x; at += x.y;
    }
}

// gradient of the sampled field at grid point p: central differences, one-sided on the boundary faces
__device__ __forceinline__ void mesh_gradient(const float* __restrict__ v, int p, const MeshGrid& g, const float h[3], float out[3]) {
    int idx[3];
    mesh_ijk(p, g, idx[0], idx[1], idx[2]);
    const int stride[3] = {g.ny * g.nz, g.nz, 1}, size[3] = {g.nx, g.ny, g.nz};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (idx[k] > 0 && idx[k] + 1 < size[k]) out[k] = (v[p + stride[k]] - v[p - stride[k]]) / (2.0f * h[k]);
        else if (idx[k] == 0) out[k] = (v[p + stride[k]] - v[p]) / h[k];
        else out[k] = (v[p] - v[p - stride[k]]) / h[k];
    }
}

struct MeshBox { float lo[3], h[3]; };

__global__ void __launch_bounds__(256) mesh_emit_vertices_kernel(const float* __restrict__ v, MeshGrid g, MeshBox box, MeshWorkspace w,
                                                                 float* __restrict__ vertices, float* __restrict__ normals) {
    const long long pl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pl >= g.n) return;
    const int p = (int)pl;
    const uint32_t mask = w.mask[p];
    if (!mask) return;
    size_t id = (size_t)w.chunk[p / MESH_CHUNK].x + w.rank[p];
    int idx[3];
    mesh_ijk(p, g, idx[0], idx[1], idx[2]);
    const float vp = v[p];
    float gp[3];
    if (normals) mesh_gradient(v, p, g, box.h, gp);
#pragma unroll
    for (int e = 1; e < 8; ++e) {
        if (!(mask >> e & 1u)) continue;
        const int q = p + mesh_offset(e, g);
        float t = (g.iso - vp) / (v[q] - vp);
        if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;                   // only non-finite values get here
        const float d[3] = {(e & 4) ? t : 0.0f, (e & 2) ? t : 0.0f, (e & 1) ? t : 0.0f};
#pragma unroll
        for (int k = 0; k < 3; ++k) vertices[3 * id + k] = box.lo[k] + ((float)idx[k] + d[k]) * box.h[k];
        if (normals) {
            float gq[3], n[3];
            mesh_gradient(v, q, g, box.h, gq);
            const float out = g.sign > 0 ? -1.0f : 1.0f;           // the gradient points towards higher values: inwards for a density
#pragma unroll
            for (int k = 0; k < 3; ++k) n[k] = (gp[k] + t * (gq[k] - gp[k])) * out;
            const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            const float r[3] = {n[0] / len, n[1] / len, n[2] / len};
            const bool good = len > 0.0f && isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) normals[3 * id + k] = good ? r[k] : 0.0f;
        }
        ++id;
    }
}

__device__ __forceinline__ int mesh_pick6(const int x[6], uint32_t k) {
    const int a = k & 1u ? x[1] : x[0], b = k & 1u ? x[3] : x[2], c = k & 1u ? x[5] : x[4];
    return k & 4u ? c : (k & 2u ? b : a);
}

__global__ void __launch_bounds__(256) mesh_emit_faces_kernel(const float* __restrict__ v, MeshGrid g, MeshWorkspace w,
                                                              int32_t* __restrict__ faces) {
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long first = wave * MESH_CHUNK;
    if (first >= g.n) return;
    const int lo = (int)first, hi = (int)min(first + MESH_CHUNK, (long long)g.n), lane = threadIdx.x & 63;
    int t_run = w.chunk[wave].y;
    for (int r = 0; r < MESH_CHUNK / 64 && lo + 64 * r < hi; ++r) {
        const int p0 = lo + 64 * r;
        const bool live = lane < hi - p0;
        const int p = live ? p0 + lane : p0;
        const int tris = live ? (int)w.tris[p] : 0;
        const int incl = wave_scan_add_i(tris, lane);
        size_t f = (size_t)(t_run + incl - tris);
        t_run += __shfl(incl, 63, 64);
        if (tris) {                                                // a guarded body, not `continue`: every lane reaches the next round's scan
            const size_t f_end = f + tris;                             // values that changed since the count must not move a write out of this cell's rows
            uint32_t on_grid;
            const uint32_t in = mesh_corner_bits(v, p, g, on_grid);   // tris > 0: all eight corners are on the grid
            int base[7];
            uint32_t mask[7];
#pragma unroll
            for (int c = 0; c < 7; ++c) {                              // the seven corners that own edges of this cell
                const int q = p + mesh_offset(c, g);
                base[c] = w.chunk[q / MESH_CHUNK].x + (int)w.rank[q];
                mask[c] = w.mask[q];
            }
#pragma unroll
            for (int pi = 0; pi < 6; ++pi) {
                const uint32_t code = MESH_CASE[mesh_tet_bits(in, pi)];
                const int n_tri = (int)(code & 3u);
                if (!n_tri) continue;
                int id[6];                                             // the vertex an edge would carry; used only where it does
#pragma unroll
                for (int e = 0; e < 6; ++e) {
                    const int c = MESH_TET[pi][MESH_EDGE[e][0]], d = MESH_TET[pi][MESH_EDGE[e][1]] ^ c;
                    id[e] = base[c] + __popc(mask[c] & ((1u << d) - 1u));
                }
                const bool odd = pi == 1 || pi == 2 || pi == 5;
                for (int k = 0; k < n_tri; ++k) {
                    const uint32_t tri = code >> (2 + 9 * k);
                    const int a = mesh_pick6(id, tri & 7u), b = mesh_pick6(id, (tri >> 3) & 7u), c = mesh_pick6(id, (tri >> 6) & 7u);
                    if (f < f_end) {
                        faces[3 * f] = a;
                        faces[3 * f + 1] = odd ? c : b;
                        faces[3 * f + 2] = odd ? b : c;
                    }
                    ++f;
                }
            }
        }
    }
}

}  // namespace ngp

using namespace ngp;

static bool mesh_args_ok(const float* values, int nx, int ny, int nz, int sign, const void* workspace) {
    return values && workspace && nx >= 2 && ny >= 2 && nz >= 2 && (sign == 1 || sign == -1) &&
           (long long)nx * ny * nz < (1ll << 31);
}
static MeshGrid mesh_grid(int nx, int ny, int nz, float iso, int sign) { return {nx, ny, nz, nx * ny * nz, iso, sign}; }

extern "C" {

long long ngp_mesh_workspace_bytes(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2 || (long long)nx * ny * nz >= (1ll << 31)) return -1;
    const long long n = (long long)nx * ny * nz;
    return mesh_align16(8 * mesh_chunks(n)) + mesh_align16(2 * n) + 2 * mesh_align16(n);
}

int ngp_mesh_count(const float* values, int nx, int ny, int nz, float iso, int sign, void* workspace, int32_t* counts, void* stream) {
    if (!mesh_args_ok(values, nx, ny, nz, sign, workspace) || !counts) return -1;
    const MeshGrid g = mesh_grid(nx, ny, nz, iso, sign);
    const MeshWorkspace w = mesh_workspace(workspace, g.n);
    const long long chunks = mesh_chunks(g.n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)((chunks + 3) / 4)), dim3(256), 0, s, values, g, w);
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(MESH_SCAN_THREADS), 0, s, w.chunk, chunks, counts);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_emit(const float* values, int nx, int ny, int nz, float iso, int sign, const float* lo, const float* h, const void* workspace,
                  float* vertices, float* normals, int32_t* faces, void* stream) {
    if (!mesh_args_ok(values, nx, ny, nz, sign, workspace) || !lo || !h || !vertices || !faces) return -1;
    if (!(h[0] > 0.0f && h[1] > 0.0f && h[2] > 0.0f)) return -1;
    const MeshGrid g = mesh_grid(nx, ny, nz, iso, sign);
    const MeshWorkspace w = mesh_workspace(const_cast<void*>(workspace), g.n);
    const MeshBox box = {{lo[0], lo[1], lo[2]}, {h[0], h[1], h[2]}};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_emit_vertices_kernel, dim3((unsigned)(((long long)g.n + 255) / 256)), dim3(256), 0, s, values, g, box, w, vertices,
                       normals);
    hipLaunchKernelGGL(mesh_emit_faces_kernel, dim3((unsigned)((mesh_chunks(g.n) + 3) / 4)), dim3(256), 0, s, values, g, w, faces);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
