// mesh_sdf.hip -- signed distance from points to a triangle mesh: a bounding-volume hierarchy built on the device and a one-launch
// nearest-face query, for gfx950.  The contract is DESIGN.md section 3, "Distance to a triangle mesh"; tests/mesh_sdf_reference.py
// restates the arithmetic in numpy, operation for operation.
//
// THE TREE.  The caller sorts the faces (order[s] = the caller's index of the face at sorted position s; the package sorts by the
// Morton code of the centroid).  Leaf k holds the sorted positions [k L, min((k + 1) L, n_faces)), L = leaf_size; the leaves are padded
// to P = the next power of two >= ceil(n_faces / L), and the tree is the implicit complete binary tree over them: 2 P - 1 nodes, node i
// has the children 2 i + 1 and 2 i + 2, leaf k is node P - 1 + k.  boxes: f32 [2 P - 1, 6] = (lo xyz, hi xyz).
//   mesh_sdf_leaf_kernel    one lane per leaf: min / max of the vertices of its faces (exact in f32), widened (below); an empty leaf
//                           gets the inverted box lo = +inf, hi = -inf
//   mesh_sdf_level_kernel   one launch per level, bottom up, one lane per node: the union of the two children's boxes (min / max: exact;
//                           the union with an inverted box is the other box, two inverted boxes give an inverted box)
// No atomics, every node written by one lane from inputs that are final: the same mesh gives the same bytes.
//
// THE CLOSEST POINT on a face (a, b, c) for a point p: the Voronoi-region test of Ericson, Real-Time Collision Detection, 5.1.5, in
// f32, every operation rounded on its own (-ffp-contract=off), dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z:
//   ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c
//   d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp
//   vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4
//   the first rule that holds gives the feature and the barycentrics (v, w) of the closest point a + v ab + w ac:
//     d1 <= 0 and d2 <= 0                         vertex a (4)   v = 0, w = 0
//     d3 >= 0 and d4 <= d3                        vertex b (5)   v = 1, w = 0
//     vc <= 0 and d1 >= 0 and d3 <= 0             edge ab  (1)   v = d1 / (d1 - d3), w = 0
//     d6 >= 0 and d5 <= d6                        vertex c (6)   v = 0, w = 1
//     vb <= 0 and d2 >= 0 and d6 <= 0             edge ca  (3)   v = 0, w = d2 / (d2 - d6)
//     va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0   edge bc  (2)   w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
//     otherwise                                   interior (0)   den = 1 / (va + vb + vc), v = vb den, w = vc den
//   per component:  closest = (a + ab v) + ac w,   r = ap - (ab v + ac w),   dist2 = r.r
//   n = cross(ab, ac) = (ab.y ac.z - ab.z ac.y, ab.z ac.x - ab.x ac.z, ab.x ac.y - ab.y ac.x); if n = (0, 0, 0), dist2 = NaN: a face
//   without area in f32 (collinear or coincident corners) has no normal and is no face, though its rules would still measure a segment
// r is x - closest formed in the face's own frame: its error is relative to |ap|, |ab| and |ac| and does not grow with the distance of
// the mesh from the origin (closest, an output, does carry the rounding of the coordinates).  dist2 and the sign both use r.
// A face wins with dist2 < best, strictly: a NaN (a zero-area face, or a rule that divides 0 by 0) never wins, and of two equal distances
// the face met first in the walk stays -- the walk is a function of the point and the tree, so is the result.
//
// PRUNING.  lb(box, p) = (gx gx + gy gy) + gz gz with g = max(max(lo - p, p - hi), 0) per axis, times (1 - 2^-18); a node is entered
// iff lb < best.  The guarantee that no face is pruned whose computed dist2 would have won:
//   * every leaf box is widened outwards by m = 2^-18 x (its longest side) and then one more ulp (nextafter), so the widening survives
//     the rounding of lo - m at any distance from the origin.  A computed r differs from the vector to a true point of the face by at
//     most about 10 ulp-fractions (2^-24) of the face's diameter <= sqrt(3) x the longest side: well below m = 64 x 2^-24 x side.  So
//     the computed distance of any face below a node is at least the true distance to the node's (widened) box, times 1 - 3 x 2^-24.
//   * the lower bound itself has five roundings, each relative (at most 5 x 2^-24 too large); the factor 1 - 2^-18 = 1 - 64 x 2^-24
//     takes out these, the 2 x 3 x 2^-24 of the face's side of the comparison and the three roundings of r.r.
// An inverted box gives lb = +inf, which is never < best (best starts at +inf): padding is never entered.
//
// THE WALK is the one of mesh_bvh.h ("THE WALK" and "TERMINATION") with key = lb and limit = best: the nearer child first.  The root is
// entered without a test: a tree has at least one face.
//
// THE SIGN (signed mode: both normal arrays given): s = +1 if n.r >= 0 else -1, n by the feature of the winning face f -- interior:
// cross(ab, ac), unnormalised; edge e: edge_normals[f, e]; vertex k: vertex_normals[faces[f, k]] (the angle-weighted pseudonormals of
// Baerentzen & Aanaes 2005, made by the caller).  sdf = s sqrt(dist2).  Unsigned mode: sdf = sqrt(dist2).
#include "mesh_bvh.h"

namespace ngp {

constexpr int MESH_SDF_QUERY_BLOCK = 64;                        // one wave per block: a walk is as long as its slowest lane, and a small batch
                                                               // (16 384 points = 256 waves) then reaches every CU
constexpr float MESH_SDF_WIDEN = 1.0f / 262144.0f;             // 2^-18: of the leaf box's longest side
constexpr float MESH_SDF_DEFLATE = 1.0f - 1.0f / 262144.0f;    // 1 - 2^-18: on the squared lower bound

__global__ void __launch_bounds__(MESH_SWEEP_BLOCK) mesh_sdf_leaf_kernel(MeshGeometry g, float* __restrict__ boxes) {
    const long long k = (long long)blockIdx.x * MESH_SWEEP_BLOCK + threadIdx.x;
    if (k >= g.padded) return;
    V3 lo = {INFINITY, INFINITY, INFINITY}, hi = {-INFINITY, -INFINITY, -INFINITY};
    const auto grow = [&](V3 v) {
        lo = {fminf(lo.x, v.x), fminf(lo.y, v.y), fminf(lo.z, v.z)};
        hi = {fmaxf(hi.x, v.x), fmaxf(hi.y, v.y), fmaxf(hi.z, v.z)};
    };
    mesh_leaf_faces(g, k, [&](long long, long long f) {
        V3 a, b, c;
        mesh_face_corners(g, f, a, b, c);
        grow(a); grow(b); grow(c);
    });
    if (k * g.leaf_size < g.n_faces) {
        const float m = fmaxf(fmaxf(hi.x - lo.x, hi.y - lo.y), hi.z - lo.z) * MESH_SDF_WIDEN;
        lo = {nextafterf(lo.x - m, -INFINITY), nextafterf(lo.y - m, -INFINITY), nextafterf(lo.z - m, -INFINITY)};
        hi = {nextafterf(hi.x + m, INFINITY), nextafterf(hi.y + m, INFINITY), nextafterf(hi.z + m, INFINITY)};
    }
    float* out = boxes + 6 * ((long long)g.padded - 1 + k);
    out[0] = lo.x; out[1] = lo.y; out[2] = lo.z;
    out[3] = hi.x; out[4] = hi.y; out[5] = hi.z;
}

// nodes [first, first + count) of one level: the union of the children
__global__ void __launch_bounds__(MESH_SWEEP_BLOCK) mesh_sdf_level_kernel(float* __restrict__ boxes, int first, int count) {
    const long long t = (long long)blockIdx.x * MESH_SWEEP_BLOCK + threadIdx.x;
    if (t >= count) return;
    const long long i = first + t;
    const float* l = boxes + 6 * (2 * i + 1);
    const float* r = l + 6;
    float* out = boxes + 6 * i;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[a] = fminf(l[a], r[a]);
        out[3 + a] = fmaxf(l[3 + a], r[3 + a]);
    }
}

struct MeshHit { float d2; int feature; V3 closest, r, n; };

// the header comment's formula; every rule is evaluated and the first that holds is selected, so the lanes of a wave stay together
__device__ __forceinline__ MeshHit mesh_closest(V3 p, V3 a, V3 b, V3 c) {
    MeshHit h;
    const V3 ab = v3_sub(b, a), ac = v3_sub(c, a);
    const V3 ap = v3_sub(p, a), bp = v3_sub(p, b), cp = v3_sub(p, c);
    const float d1 = v3_dot(ab, ap), d2 = v3_dot(ac, ap), d3 = v3_dot(ab, bp), d4 = v3_dot(ac, bp), d5 = v3_dot(ab, cp),
                d6 = v3_dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float den = 1.0f / ((va + vb) + vc);
    float v = vb * den, w = vc * den;
    int feature = 0;
    const float e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) { w = e43 / (e43 + e56); v = 1.0f - w; feature = 2; }
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { v = 0.0f; w = d2 / (d2 - d6); feature = 3; }
    if (d6 >= 0.0f && d5 <= d6) { v = 0.0f; w = 1.0f; feature = 6; }
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { v = d1 / (d1 - d3); w = 0.0f; feature = 1; }
    if (d3 >= 0.0f && d4 <= d3) { v = 1.0f; w = 0.0f; feature = 5; }
    if (d1 <= 0.0f && d2 <= 0.0f) { v = 0.0f; w = 0.0f; feature = 4; }
    h.feature = feature;
    h.closest = {(a.x + ab.x * v) + ac.x * w, (a.y + ab.y * v) + ac.y * w, (a.z + ab.z * v) + ac.z * w};
    h.r = {ap.x - (ab.x * v + ac.x * w), ap.y - (ab.y * v + ac.y * w), ap.z - (ab.z * v + ac.z * w)};
    h.n = v3_cross(ab, ac);
    h.d2 = (h.n.x != 0.0f || h.n.y != 0.0f || h.n.z != 0.0f) ? v3_dot(h.r, h.r) : NAN;       // no area, no normal: not a face
    return h;
}

__device__ __forceinline__ float mesh_box_bound(const float* __restrict__ boxes, long long node, V3 p) {
    const float* b = boxes + 6 * node;
    const float gx = fmaxf(fmaxf(b[0] - p.x, p.x - b[3]), 0.0f), gy = fmaxf(fmaxf(b[1] - p.y, p.y - b[4]), 0.0f),
                gz = fmaxf(fmaxf(b[2] - p.z, p.z - b[5]), 0.0f);
    return ((gx * gx + gy * gy) + gz * gz) * MESH_SDF_DEFLATE;
}

// (vertices, faces) loose, not a MeshGeometry, and the corner loads spelled out: mesh_sdf_query_kernel keeps the parent's parameters and
// text so that it compiles to the same instructions (profiles/mesh_tree_refactor.md)
__device__ __forceinline__ MeshHit mesh_face_hit(const float* __restrict__ vertices, const int32_t* __restrict__ faces, long long f, V3 p) {
    return mesh_closest(p, v3_load(vertices, faces[3 * f]), v3_load(vertices, faces[3 * f + 1]), v3_load(vertices, faces[3 * f + 2]));
}

__global__ void __launch_bounds__(MESH_SDF_QUERY_BLOCK) mesh_sdf_query_kernel(const float* __restrict__ points, int n, const float* __restrict__ vertices,
                                                             const int32_t* __restrict__ faces, const int32_t* __restrict__ order,
                                                             const float* __restrict__ boxes, int n_faces, int leaf_size, int padded,
                                                             const float* __restrict__ edge_normals, const float* __restrict__ vertex_normals,
                                                             float* __restrict__ sdf, float* __restrict__ closest, int32_t* __restrict__ face,
                                                             int32_t* __restrict__ feature) {
    const long long i = (long long)blockIdx.x * MESH_SDF_QUERY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const V3 p = v3_load(points, i);
    const int first_leaf = padded - 1;
    float best = INFINITY;
    int best_pos = -1;
    MeshTally<2> tally;                      // boxes tested, faces evaluated
    int node = 0, depth = 0;
    uint32_t trail = 0;
    bool down = true;                        // the root is entered without a test: a tree has at least one face
    for (;;) {                               // mesh_bvh.h, "THE WALK": keep this and mesh_raycast_kernel's alike, state for state
        if (down) {
            if (node >= first_leaf) {
                const long long s0 = (long long)(node - first_leaf) * leaf_size;
                for (int j = 0; j < leaf_size && s0 + j < n_faces; ++j) {
                    const MeshHit h = mesh_face_hit(vertices, faces, order[s0 + j], p);
                    if (h.d2 < best) { best = h.d2; best_pos = (int)(s0 + j); }
                    tally.add(1);
                }
                down = false;
            } else {
                const int c0 = 2 * node + 1;
                const float l0 = mesh_box_bound(boxes, c0, p), l1 = mesh_box_bound(boxes, c0 + 1, p);
                tally.add(0, 2);
                if (fminf(l0, l1) < best) {
                    node = l1 < l0 ? c0 + 1 : c0;
                    ++depth;
                    trail &= ~(1u << depth);         // the sibling is still to come
                } else {
                    down = false;
                }
            }
        } else {
            if (depth == 0) break;
            if (!((trail >> depth) & 1u)) {
                trail |= 1u << depth;
                node = ((node - 1) ^ 1) + 1;
                tally.add(0);
                down = mesh_box_bound(boxes, node, p) < best;
            } else {
                node = (node - 1) >> 1;
                --depth;
            }
        }
    }
    tally.flush();
    if (best_pos < 0) {                      // every face evaluated to NaN: no nearest face
        sdf[i] = INFINITY;
        if (closest) { closest[3 * i] = p.x; closest[3 * i + 1] = p.y; closest[3 * i + 2] = p.z; }
        if (face) face[i] = -1;
        if (feature) feature[i] = 0;
        return;
    }
    const long long f = order[best_pos];
    const MeshHit h = mesh_face_hit(vertices, faces, f, p);                    // the same bits as in the walk
    float s = 1.0f;
    if (edge_normals) {
        V3 nrm = h.n;
        if (h.feature >= 4) nrm = v3_load(vertex_normals, faces[3 * f + (h.feature - 4)]);
        else if (h.feature >= 1) nrm = v3_load(edge_normals, 3 * f + (h.feature - 1));
        s = v3_dot(nrm, h.r) >= 0.0f ? 1.0f : -1.0f;
    }
    sdf[i] = s * sqrtf(h.d2);
    if (closest) { closest[3 * i] = h.closest.x; closest[3 * i + 1] = h.closest.y; closest[3 * i + 2] = h.closest.z; }
    if (face) face[i] = (int32_t)f;
    if (feature) feature[i] = h.feature;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

long long ngp_mesh_bvh_bytes(long long n_faces, int leaf_size) {
    MeshTree t;
    if (!mesh_tree(n_faces, leaf_size, t)) return -1;
    return 24 * (2 * t.padded - 1);
}

int ngp_mesh_bvh_build(const float* vertices, const int32_t* faces, const int32_t* order, int n_faces, int leaf_size, float* boxes,
                       void* stream) {
    MeshGeometry g;
    MeshTree t;
    if (!boxes || !mesh_geometry(vertices, faces, order, n_faces, leaf_size, g, t)) return -1;
    mesh_tree_sweep(
        t, (hipStream_t)stream,
        [&](dim3 grid, dim3 block, hipStream_t s) { hipLaunchKernelGGL(mesh_sdf_leaf_kernel, grid, block, 0, s, g, boxes); },
        [&](dim3 grid, dim3 block, hipStream_t s, int first, int count) {
            hipLaunchKernelGGL(mesh_sdf_level_kernel, grid, block, 0, s, boxes, first, count);
        });
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_sdf_query(const float* points, int n, const float* vertices, const int32_t* faces, const int32_t* order, const float* boxes,
                       int n_faces, int leaf_size, const float* edge_normals, const float* vertex_normals, float* sdf, float* closest,
                       int32_t* face, int32_t* feature, void* stream) {
    MeshGeometry g;
    MeshTree t;
    if (!boxes || n < 0 || !mesh_geometry(vertices, faces, order, n_faces, leaf_size, g, t)) return -1;
    if ((edge_normals == nullptr) != (vertex_normals == nullptr)) return -1;
    if (n == 0) return 0;                    // an empty batch has no points and no outputs: their pointers may be null
    if (!points || !sdf) return -1;
    hipLaunchKernelGGL(mesh_sdf_query_kernel, dim3((unsigned)(((long long)n + MESH_SDF_QUERY_BLOCK - 1) / MESH_SDF_QUERY_BLOCK)),
                       dim3(MESH_SDF_QUERY_BLOCK), 0, (hipStream_t)stream, points, n, g.vertices, g.faces, g.order, boxes, g.n_faces,
                       g.leaf_size, g.padded, edge_normals, vertex_normals, sdf, closest, face, feature);
    NGP_LAUNCH_CHECK();
    return 0;
}

// the microbenchmark's build only (profiles/microbench/mesh_sdf.py binds it by hand): read and clear the two tallies
NGP_MESH_TALLY_ENTRY(ngp_mesh_sdf_counters, 2)

}  // extern "C"
