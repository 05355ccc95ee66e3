// mesh_winding.hip -- the generalized winding number of a triangle mesh at a point (Jacobson et al. 2013), evaluated through the box
// hierarchy of mesh_sdf.hip with a far-field expansion per node (Barill et al. 2018, "Fast winding numbers for soups and clouds"): one
// bottom-up pass for per-node moments and a one-launch query, for gfx950.  The contract is DESIGN.md section 3, "Winding number of a
// triangle mesh"; tests/mesh_winding_reference.py restates the arithmetic in numpy, operation for operation.
//
// DEFINITION.  w(q) = (1 / 4 pi) sum_f Omega_f(q), Omega_f the signed solid angle of face f seen from q.  f32, every operation rounded
// on its own (-ffp-contract=off), dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z (v3_dot), cross(u, v) = (u.y v.z - u.z v.y, u.z v.x - u.x v.z,
// u.x v.y - u.y v.x).  THE EXACT TERM of a face (A, B, C), van Oosterom & Strackee 1983:
//   a = A - q, b = B - q, c = C - q;  la = sqrt(a.a), lb = sqrt(b.b), lc = sqrt(c.c)
//   num = a . cross(b, c);  den = (((la lb) lc + (a.b) lc) + (b.c) la) + (c.a) lb
//   Omega = 2 atan2(num, den), and 0 where num == 0
// num == 0 is the point in the plane of the face: outside the face the angle is 0 anyway, inside it the two one-sided limits are +-2 pi
// and 0 is their mean (atan2(+-0, den < 0) alone would say +-pi by the sign of a zero).  So a point on a vertex (a = 0) and a point on
// the line of a face without area add exactly 0, a face without area seen from elsewhere adds 0 up to the rounding of num (den > 0
// there), and every term is finite.
// ORIENTATION: with cross(B - A, C - A) pointing outward a closed mesh
// gives w = +1 inside and 0 outside -- the orientation for which the pseudonormal sign of mesh_sdf.hip is negative inside.
//
// THE TREE is the one ngp_mesh_bvh_build makes (mesh_sdf.hip, "THE TREE"): the same boxes, order and leaf sizes, read only.
//
// THE MOMENTS.  moments: f32 [2 P - 1, 20], one row of 80 bytes (five aligned 16-byte loads) per node of that tree:
//   0..2   p = the area-weighted centroid of the faces below the node (the box centre 0.5 lo + 0.5 hi when their area sums to 0)
//   3      r = the radius: the distance from p to the farthest corner of the node's box, rounded upwards; -1 marks an EMPTY (padding) node
//   4..6   N = sum_f an_f, an_f = 0.5 cross(B - A, C - A) the area vector of a face
//   7      A = sum_f |an_f|
//   8..16  T = sum_f (c_f - p) (x) an_f, row major (T[i][j] = sum (c_f - p)_i (an_f)_j), c_f the centroid of the face
//   17     1 for a node with faces, 0 for an empty one;  18, 19: 0
//   mesh_winding_leaf_kernel    one lane per leaf, its faces in sorted order j = 0 .. L - 1, all about o = the first corner of its first
//                               face so that nothing cancels far from the origin:  n2 = cross(B - A, C - A), an = 0.5 n2,
//                               area = 0.5 sqrt(n2.n2), c' = (((A - o) + (B - o)) + (C - o)) / 3;  sums A += area, S += area c', N += an,
//                               To[i][j] += c'_i an_j;  then p' = S / A, p = o + p' (A = 0: p = the box centre, p' = p - o) and
//                               T[i][j] = To[i][j] - p'_i N_j
//   mesh_winding_level_kernel   one launch per level, bottom up, one lane per node, the children l and r combined with the parallel-axis
//                               shift:  A = A_l + A_r, p = p_l + (A_r / A) (p_r - p_l) (A = 0: the box centre), N = N_l + N_r,
//                               T[i][j] = (T_l[i][j] + (p_l - p)_i N_l[j]) + (T_r[i][j] + (p_r - p)_i N_r[j]).  One empty child: the
//                               other's p, N, A, T; two: an empty node.
//   r, in both: m = max(p - lo, hi - p) per axis, r = sqrt(m.m) (1 + 2^-21).  The farthest corner bounds the distance from p to every
//   vertex below the node (the leaf boxes are already widened outwards) and needs no pass over vertices; 2^-21 = 8 x 2^-24 holds the
//   three roundings of m, the five of m.m and the one of the root.
// No atomics, every row written by one lane from inputs that are final: the same mesh gives the same bytes.
//
// THE QUERY.  One lane per point, preorder over the implicit tree.  At a node with faces, d = p - q:
//   ACCEPTED iff d.d > (beta r) (beta r).  Its contribution, with l = sqrt(d.d), i3 = 1 / ((d.d) l), i5 = i3 / (d.d):
//     order >= 1   (N.d) i3
//     order 2      + (((T00 + T11) + T22) i3 - (3 (d . (T d))) i5),   (T d)_i = (T[i][0] d.x + T[i][1] d.y) + T[i][2] d.z
//   otherwise the lane goes down; a leaf that is not accepted adds Omega of each of its faces.  beta >= 1 (the entry refuses less), so an
//   accepted node has |d| > r >= 0 and nothing divides by zero; beta = +inf accepts nothing (inf x 0 = NaN compares false as well) and
//   gives the exact sum through the tree.  The sum is plain f32 in walk order, times 1 / 4 pi at the end: a result depends on its point
//   and the tree alone.  A point with a coordinate that is not finite gets NaN without a walk (a finite point so far away that d.d
//   overflows f32, beyond about 1e19 from the mesh, ends in NaN as well: inf x 0).
// THE WALK is stackless and needs not even the trail bits of the two sibling queries, because no node is tested twice: after a node is
// consumed (accepted, empty, or a leaf summed) the lane climbs while the node is a right child (an even index) and then steps to the
// sibling i + 1; from the root it is done.  Floats decide only whether a node is accepted: the walk ends after at most 2 P - 1 nodes for
// any bit pattern.  No per-lane array, nothing in scratch or LDS.
#include "mesh_bvh.h"

namespace ngp {

constexpr int MESH_WINDING_BLOCK = 64;                          // one wave per block, as mesh_sdf_query_kernel
constexpr int MESH_WINDING_ROW = 20;                            // floats per node
constexpr float MESH_WINDING_ROUND_UP = 1.0f + 1.0f / 2097152.0f;      // 1 + 2^-21: on the radius
constexpr float MESH_WINDING_INV_4PI = 0.07957747154594767f;

struct MeshMoments { V3 p; float r; V3 n; float area; float t[9]; };

__device__ __forceinline__ MeshMoments mesh_moments_load(const float* __restrict__ row) {
    MeshMoments m;
    m.p = {row[0], row[1], row[2]};
    m.r = row[3];
    m.n = {row[4], row[5], row[6]};
    m.area = row[7];
#pragma unroll
    for (int k = 0; k < 9; ++k) m.t[k] = row[8 + k];
    return m;
}

__device__ __forceinline__ void mesh_moments_store(float* __restrict__ row, const MeshMoments& m) {
    row[0] = m.p.x; row[1] = m.p.y; row[2] = m.p.z; row[3] = m.r;
    row[4] = m.n.x; row[5] = m.n.y; row[6] = m.n.z; row[7] = m.area;
#pragma unroll
    for (int k = 0; k < 9; ++k) row[8 + k] = m.t[k];
    row[17] = 1.0f; row[18] = 0.0f; row[19] = 0.0f;
}

__device__ __forceinline__ void mesh_moments_store_empty(float* __restrict__ row) {
#pragma unroll
    for (int k = 0; k < MESH_WINDING_ROW; ++k) row[k] = 0.0f;
    row[3] = -1.0f;
}

__device__ __forceinline__ V3 mesh_box_centre(const float* __restrict__ box) {
    return {0.5f * box[0] + 0.5f * box[3], 0.5f * box[1] + 0.5f * box[4], 0.5f * box[2] + 0.5f * box[5]};
}

// the header comment's r: from p to the farthest corner of the box, rounded upwards
__device__ __forceinline__ float mesh_box_radius(const float* __restrict__ box, V3 p) {
    const V3 m = {fmaxf(p.x - box[0], box[3] - p.x), fmaxf(p.y - box[1], box[4] - p.y), fmaxf(p.z - box[2], box[5] - p.z)};
    return sqrtf(v3_dot(m, m)) * MESH_WINDING_ROUND_UP;
}

__global__ void __launch_bounds__(MESH_SWEEP_BLOCK) mesh_winding_leaf_kernel(MeshGeometry g, const float* __restrict__ boxes,
                                                                             float* __restrict__ moments) {
    const long long k = (long long)blockIdx.x * MESH_SWEEP_BLOCK + threadIdx.x;
    if (k >= g.padded) return;
    const long long node = (long long)g.padded - 1 + k;
    float* row = moments + MESH_WINDING_ROW * node;
    const long long first = k * g.leaf_size;
    if (first >= g.n_faces) { mesh_moments_store_empty(row); return; }
    const V3 o = v3_load(g.vertices, g.faces[3 * (long long)g.order[first]]);
    MeshMoments m;
    m.area = 0.0f;
    m.n = {0.0f, 0.0f, 0.0f};
    V3 s = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 9; ++i) m.t[i] = 0.0f;
    mesh_leaf_faces(g, k, [&](long long, long long f) {
        V3 a, b, c;
        mesh_face_corners(g, f, a, b, c);
        const V3 n2 = v3_cross(v3_sub(b, a), v3_sub(c, a));
        const V3 an = v3_scale(n2, 0.5f);
        const float area = 0.5f * sqrtf(v3_dot(n2, n2));
        const V3 ca = v3_sub(a, o), cb = v3_sub(b, o), cc = v3_sub(c, o);
        const V3 cf = {((ca.x + cb.x) + cc.x) / 3.0f, ((ca.y + cb.y) + cc.y) / 3.0f, ((ca.z + cb.z) + cc.z) / 3.0f};
        m.area += area;
        s = v3_add(s, v3_scale(cf, area));
        m.n = v3_add(m.n, an);
        m.t[0] += cf.x * an.x; m.t[1] += cf.x * an.y; m.t[2] += cf.x * an.z;
        m.t[3] += cf.y * an.x; m.t[4] += cf.y * an.y; m.t[5] += cf.y * an.z;
        m.t[6] += cf.z * an.x; m.t[7] += cf.z * an.y; m.t[8] += cf.z * an.z;
    });
    const float* box = boxes + 6 * node;
    V3 pl;
    if (m.area > 0.0f) {
        pl = {s.x / m.area, s.y / m.area, s.z / m.area};
        m.p = v3_add(o, pl);
    } else {
        m.p = mesh_box_centre(box);
        pl = v3_sub(m.p, o);
    }
    m.t[0] -= pl.x * m.n.x; m.t[1] -= pl.x * m.n.y; m.t[2] -= pl.x * m.n.z;
    m.t[3] -= pl.y * m.n.x; m.t[4] -= pl.y * m.n.y; m.t[5] -= pl.y * m.n.z;
    m.t[6] -= pl.z * m.n.x; m.t[7] -= pl.z * m.n.y; m.t[8] -= pl.z * m.n.z;
    m.r = mesh_box_radius(box, m.p);
    mesh_moments_store(row, m);
}

// nodes [first, first + count) of one level: the children's moments moved to the common centroid and added
__global__ void __launch_bounds__(MESH_SWEEP_BLOCK) mesh_winding_level_kernel(const float* __restrict__ boxes, float* moments, int first,
                                                                              int count) {
    const long long t = (long long)blockIdx.x * MESH_SWEEP_BLOCK + threadIdx.x;
    if (t >= count) return;
    const long long i = first + t;
    float* row = moments + MESH_WINDING_ROW * i;
    const MeshMoments l = mesh_moments_load(moments + MESH_WINDING_ROW * (2 * i + 1));
    const MeshMoments r = mesh_moments_load(moments + MESH_WINDING_ROW * (2 * i + 2));
    const float* box = boxes + 6 * i;
    const bool l_empty = l.r < 0.0f, r_empty = r.r < 0.0f;
    if (l_empty && r_empty) { mesh_moments_store_empty(row); return; }
    MeshMoments m;
    if (l_empty || r_empty) {
        m = l_empty ? r : l;
    } else {
        m.area = l.area + r.area;
        if (m.area > 0.0f) {
            const float w = r.area / m.area;
            m.p = v3_add(l.p, v3_scale(v3_sub(r.p, l.p), w));
        } else {
            m.p = mesh_box_centre(box);
        }
        const V3 sl = v3_sub(l.p, m.p), sr = v3_sub(r.p, m.p);
        m.n = v3_add(l.n, r.n);
        m.t[0] = (l.t[0] + sl.x * l.n.x) + (r.t[0] + sr.x * r.n.x);
        m.t[1] = (l.t[1] + sl.x * l.n.y) + (r.t[1] + sr.x * r.n.y);
        m.t[2] = (l.t[2] + sl.x * l.n.z) + (r.t[2] + sr.x * r.n.z);
        m.t[3] = (l.t[3] + sl.y * l.n.x) + (r.t[3] + sr.y * r.n.x);
        m.t[4] = (l.t[4] + sl.y * l.n.y) + (r.t[4] + sr.y * r.n.y);
        m.t[5] = (l.t[5] + sl.y * l.n.z) + (r.t[5] + sr.y * r.n.z);
        m.t[6] = (l.t[6] + sl.z * l.n.x) + (r.t[6] + sr.z * r.n.x);
        m.t[7] = (l.t[7] + sl.z * l.n.y) + (r.t[7] + sr.z * r.n.y);
        m.t[8] = (l.t[8] + sl.z * l.n.z) + (r.t[8] + sr.z * r.n.z);
    }
    m.r = mesh_box_radius(box, m.p);
    mesh_moments_store(row, m);
}

// the header comment's exact term
__device__ __forceinline__ float mesh_solid_angle(V3 q, V3 A, V3 B, V3 C) {
    const V3 a = v3_sub(A, q), b = v3_sub(B, q), c = v3_sub(C, q);
    const float la = sqrtf(v3_dot(a, a)), lb = sqrtf(v3_dot(b, b)), lc = sqrtf(v3_dot(c, c));
    const float num = v3_dot(a, v3_cross(b, c));
    const float den = (((la * lb) * lc + v3_dot(a, b) * lc) + v3_dot(b, c) * la) + v3_dot(c, a) * lb;
    return num == 0.0f ? 0.0f : 2.0f * atan2f(num, den);
}

// the header comment's far-field term of an accepted node: d = p - q, d2 = d.d > 0
template <int ORDER>
__device__ __forceinline__ float mesh_far_field(const float4* __restrict__ row, V3 d, float d2) {
    const float4 m1 = row[1];
    const float i3 = 1.0f / (d2 * sqrtf(d2));
    float term = v3_dot(V3{m1.x, m1.y, m1.z}, d) * i3;
    if (ORDER >= 2) {
        const float4 m2 = row[2], m3 = row[3], m4 = row[4];            // T00 T01 T02 T10 | T11 T12 T20 T21 | T22 flag 0 0
        const V3 td = {v3_dot(V3{m2.x, m2.y, m2.z}, d), v3_dot(V3{m2.w, m3.x, m3.y}, d), v3_dot(V3{m3.z, m3.w, m4.x}, d)};
        const float trace = (m2.x + m3.x) + m4.x;
        const float i5 = i3 / d2;
        term += trace * i3 - (3.0f * v3_dot(d, td)) * i5;
    }
    return term;
}

template <int ORDER>
__global__ void __launch_bounds__(MESH_WINDING_BLOCK) mesh_winding_query_kernel(const float* __restrict__ points, int n, MeshGeometry g,
                                                                                const float4* __restrict__ moments, float beta,
                                                                                float* __restrict__ winding) {
    const long long i = (long long)blockIdx.x * MESH_WINDING_BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3 q = v3_load(points, i);
    const float big = 3.402823466e+38f;
    if (!(fabsf(q.x) <= big && fabsf(q.y) <= big && fabsf(q.z) <= big)) { winding[i] = NAN; return; }
    const int first_leaf = g.padded - 1;
    float sum = 0.0f;
    int node = 0;
    MeshTally<3> tally;                                               // nodes tested, nodes accepted, faces evaluated
    for (;;) {
        const float4* row = moments + 5 * (long long)node;
        const float4 m0 = row[0];                                     // p, r
        tally.add(0);
        if (m0.w >= 0.0f) {                                           // a node with faces
            const V3 d = v3_sub(V3{m0.x, m0.y, m0.z}, q);
            const float d2 = v3_dot(d, d), br = beta * m0.w;
            if (d2 > br * br) {
                sum += mesh_far_field<ORDER>(row, d, d2);
                tally.add(1);
            } else if (node >= first_leaf) {
                mesh_leaf_faces(g, node - first_leaf, [&](long long, long long f) {
                    V3 a, b, c;
                    mesh_face_corners(g, f, a, b, c);
                    sum += mesh_solid_angle(q, a, b, c);
                    tally.add(2);
                });
            } else {
                node = 2 * node + 1;
                continue;
            }
        }
        while (node > 0 && !(node & 1)) node = (node - 1) >> 1;        // a right child: up
        if (node == 0) break;
        ++node;                                                       // a left child: across to the sibling
    }
    tally.flush();
    winding[i] = sum * MESH_WINDING_INV_4PI;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

long long ngp_mesh_winding_bytes(long long n_faces, int leaf_size) {
    MeshTree t;
    if (!mesh_tree(n_faces, leaf_size, t)) return -1;
    return 4ll * MESH_WINDING_ROW * (2 * t.padded - 1);
}

int ngp_mesh_winding_build(const float* vertices, const int32_t* faces, const int32_t* order, const float* boxes, int n_faces,
                           int leaf_size, float* moments, void* stream) {
    MeshGeometry g;
    MeshTree t;
    if (!boxes || !moments || !mesh_geometry(vertices, faces, order, n_faces, leaf_size, g, t)) return -1;
    mesh_tree_sweep(
        t, (hipStream_t)stream,
        [&](dim3 grid, dim3 block, hipStream_t s) { hipLaunchKernelGGL(mesh_winding_leaf_kernel, grid, block, 0, s, g, boxes, moments); },
        [&](dim3 grid, dim3 block, hipStream_t s, int first, int count) {
            hipLaunchKernelGGL(mesh_winding_level_kernel, grid, block, 0, s, boxes, moments, first, count);
        });
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_winding_query(const float* points, int n, const float* vertices, const int32_t* faces, const int32_t* order,
                           const float* moments, int n_faces, int leaf_size, float beta, int order_terms, float* winding, void* stream) {
    MeshGeometry g;
    MeshTree t;
    if (!moments || n < 0 || !mesh_geometry(vertices, faces, order, n_faces, leaf_size, g, t)) return -1;
    if (!(beta >= 1.0f) || (order_terms != 1 && order_terms != 2)) return -1;      // a NaN beta fails the comparison too
    if (n == 0) return 0;                    // an empty batch has no points and no output: their pointers may be null
    if (!points || !winding) return -1;
    const dim3 grid((unsigned)(((long long)n + MESH_WINDING_BLOCK - 1) / MESH_WINDING_BLOCK)), block(MESH_WINDING_BLOCK);
    const float4* rows = (const float4*)moments;
    if (order_terms == 1)
        hipLaunchKernelGGL(mesh_winding_query_kernel<1>, grid, block, 0, (hipStream_t)stream, points, n, g, rows, beta, winding);
    else
        hipLaunchKernelGGL(mesh_winding_query_kernel<2>, grid, block, 0, (hipStream_t)stream, points, n, g, rows, beta, winding);
    NGP_LAUNCH_CHECK();
    return 0;
}

// the microbenchmark's build only (profiles/microbench/mesh_winding.py binds it by hand): read and clear the three tallies
NGP_MESH_TALLY_ENTRY(ngp_mesh_winding_counters, 3)

}  // extern "C"

