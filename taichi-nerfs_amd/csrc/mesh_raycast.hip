// mesh_raycast.hip -- where a ray meets a triangle mesh: the first face along the ray (or any face: the occlusion query) found in the box
// hierarchy of mesh_sdf.hip, one launch, one lane per ray, for gfx950.  The contract is DESIGN.md section 3, "Ray casting against a
// triangle mesh"; tests/mesh_raycast_reference.py restates the ray / face arithmetic in numpy, operation for operation.
//
// THE TREE is the one ngp_mesh_bvh_build makes (mesh_sdf.hip, "THE TREE"): the same boxes, order and leaf sizes.  Nothing is rebuilt and
// the boxes are read only.
//
// THE RAY / FACE TEST is the watertight test of Woop, Benthin & Wald (JCGT 2013) in f32, every operation rounded on its own
// (-ffp-contract=off).  Per ray o + t d, once:
//   kz = the axis of the largest |d| (the first of equal ones, x before y before z), kx = (kz + 1) mod 3, ky = (kx + 1) mod 3, kx and ky
//   exchanged if d[kz] < 0 (the winding survives);   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]
// Per face (a, b, c):
//   A = a - o, B = b - o, C = c - o                                       per component
//   Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], Az = Sz A[kz]           likewise B, C: the corners sheared so that the ray is the z axis
//   U = Cx By - Cy Bx,  V = Ax Cy - Ay Cx,  W = Bx Ay - By Ax             the 2-D edge functions; two products, one difference each
//   if U == 0 or V == 0 or W == 0: all three again as (float)((double)Cx (double)By - (double)Cy (double)Bx) etc. -- the products of
//     f32 operands are exact in f64, the difference keeps its sign -- so a sign is lost only where the f64 value itself rounds to 0
//   reject if (U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0)     the origin of the sheared plane is outside
//   det = (U + V) + W;  reject if det == 0                                on edge in all three, or no area
//   T = (U Az + V Bz) + W Cz;  t = T / det                                one IEEE division
//   accept iff t_min <= t and t <= t_max; first-hit mode: the face wins iff also t < best, strictly
//   bary (v, w) = (V / det, W / det): the hit point is a + v (b - a) + w (c - a);  side = +1 if det > 0 (front: d . cross(b - a, c - a)
//   < 0) else -1;  NGP_RAYCAST_CULL_BACK rejects det < 0, NGP_RAYCAST_CULL_FRONT rejects det > 0
// A difference of two rounded products never has the wrong sign (rounding is monotone), only possibly 0, and then f64 decides: the signs
// of U, V, W are those of the EXACT edge functions of the computed 2-D corners.  A corner is sheared the same way for every face that
// uses it, so two faces that share an edge see the same two 2-D points and opposite edge functions: the ray cannot be outside both,
// at any distance of o from the mesh.  A zero-area face has det == 0 and never wins; a NaN makes every comparison of the acceptance
// false and never wins; t = +inf (an overflow) is not < best.  Of equal t the face met first in the walk stays.
//
// PRUNING.  enter(box) for the interval [t_min, hi], hi = min(t_max, best): not at all if lo.x <= hi.x fails (padding: lo = +inf,
// hi = -inf; any NaN).  Else per axis k: p0 = lo[k] - o[k], p1 = hi[k] - o[k]; m = the largest of the six |p|; delta = m 2^-19;
// s0 = (p0 - delta) inv[k], s1 = (p1 + delta) inv[k] with inv[k] = 1 / d[k] (inv[kz] IS Sz: the same division); near = the largest of
// the three min(s0, s1), far = the smallest of the three max(s0, s1) (fminf / fmaxf: a NaN from 0 x inf leaves its axis out, which
// only lets more in); tn = near - |near| 2^-21, tf = far + |far| 2^-21; enter iff tn <= tf and tn <= hi and tf >= t_min.
// The guarantee -- NO FACE IS PRUNED WHOSE COMPUTED TEST WOULD HAVE BEEN ACCEPTED WITH t < best:
//   * by the above an accepted face is hit exactly by the sheared ray in its computed 2-D corners.  A computed corner differs from the
//     true one by the roundings of A (|A[k]| 2^-24 per component), of Sx (relative 2^-24), of Sx A[kz] and of the difference: at most
//     (|A[kx]| + 3 |A[kz]|) 2^-24 <= 4 m 2^-24 sideways, for m of any box that holds the corner.  So the true ray passes within
//     4 m 2^-24 of the face, hence through the box grown by that much on kx and ky, at a parameter t* inside the kz slab.  These errors
//     are relative to |a - o|, not to the leaf's side the boxes were widened by: hence delta, 32 m 2^-24, a pad that scales with the
//     distance.  The boxes themselves are not changed.
//   * the computed t is T / det, a mean of Az, Bz, Cz with weights of one sign: within 6 x 2^-24 x max |Az| <= 6 m |Sz| 2^-24 of t*
//     (three products, two sums of T, two of det, the division), and Az itself is the kz slab's own formula on a corner between
//     lo[kz] and hi[kz] (monotone roundings: inside the slab before the pad is applied).
//   * of delta's 32 units 4 are used sideways; the other 28, divided by |d[k]| <= |d[kz]|, move each slab's ends by at least
//     28 m |Sz| 2^-24 in t, which holds the 6 of the computed t and the rounding of p -+ delta.  What is left are the three relative
//     roundings of a slab end (p, inv, the product); 2^-21 = 8 x 2^-24 on tn and tf takes them out.
// An inverted box fails the first comparison: padding is never entered.
//
// THE WALK is the one of mesh_bvh.h ("THE WALK" and "TERMINATION") with key = enter(box) for hi = min(t_max, best) and limit = +inf: the
// child with the smaller tn first.  Its leaf loop is spelled out too, not a call of mesh_leaf_faces: through that helper (as through a
// walk template) the compiler nests the leaf loop in another loop of the walk and 800 x 800 primary rays take a third longer
// (profiles/mesh_tree_refactor.md).  The root is entered after its own box test.  A ray without a dominant axis (a zero direction, or
// a component that is not finite) and a ray with t_min <= t_max false is a miss, written without a walk.  NGP_RAYCAST_ANY_HIT leaves
// the walk after the first leaf with an accepted face.
#include "mesh_bvh.h"

namespace ngp {

constexpr int MESH_RAYCAST_BLOCK = 64;                          // one wave per block, as mesh_sdf_query_kernel
constexpr float MESH_RAYCAST_PAD = 1.0f / 524288.0f;            // 2^-19: of the largest |box - origin| component, on every slab
constexpr float MESH_RAYCAST_GROW = 1.0f / 2097152.0f;          // 2^-21: of |tn| and |tf|
constexpr int MESH_RAYCAST_FLAGS = NGP_RAYCAST_ANY_HIT | NGP_RAYCAST_CULL_BACK | NGP_RAYCAST_CULL_FRONT;

struct MeshRay { V3 o, inv; float sx, sy; int kx, ky, kz; };
struct MeshRayFace { float t, v, w, det; };

__device__ __forceinline__ float v3_axis(V3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }       // selects: no indexed array

// the header comment's per-ray constants; false: no dominant axis
__device__ __forceinline__ bool mesh_ray_setup(V3 o, V3 d, MeshRay& r) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const float big = 3.402823466e+38f;
    if (!(ax <= big && ay <= big && az <= big)) return false;
    int kz = 0;
    if (ay > ax) kz = 1;
    if (az > fmaxf(ax, ay)) kz = 2;
    const float dz = v3_axis(d, kz);
    if (!(fabsf(dz) > 0.0f)) return false;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    if (dz < 0.0f) { const int s = kx; kx = ky; ky = s; }
    r.o = o;
    r.inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    r.sx = v3_axis(d, kx) / dz;
    r.sy = v3_axis(d, ky) / dz;
    r.kx = kx; r.ky = ky; r.kz = kz;
    return true;
}

// the header comment's per-face formula; t = NaN where the face is rejected (a NaN is never accepted)
__device__ __forceinline__ MeshRayFace mesh_ray_face(const MeshRay& r, V3 a, V3 b, V3 c, int flags) {
    const V3 A = v3_sub(a, r.o), B = v3_sub(b, r.o), C = v3_sub(c, r.o);
    const float akz = v3_axis(A, r.kz), bkz = v3_axis(B, r.kz), ckz = v3_axis(C, r.kz);
    const float ax = v3_axis(A, r.kx) - r.sx * akz, ay = v3_axis(A, r.ky) - r.sy * akz;
    const float bx = v3_axis(B, r.kx) - r.sx * bkz, by = v3_axis(B, r.ky) - r.sy * bkz;
    const float cx = v3_axis(C, r.kx) - r.sx * ckz, cy = v3_axis(C, r.ky) - r.sy * ckz;
    float U = cx * by - cy * bx, V = ax * cy - ay * cx, W = bx * ay - by * ax;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {
        U = (float)((double)cx * (double)by - (double)cy * (double)bx);
        V = (float)((double)ax * (double)cy - (double)ay * (double)cx);
        W = (float)((double)bx * (double)ay - (double)by * (double)ax);
    }
    const float det = (U + V) + W;
    const float sz = v3_axis(r.inv, r.kz);
    const float T = (U * (sz * akz) + V * (sz * bkz)) + W * (sz * ckz);
    MeshRayFace h;
    h.t = T / det;
    h.v = V / det;
    h.w = W / det;
    h.det = det;
    const bool mixed = (U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f);
    const bool culled = ((flags & NGP_RAYCAST_CULL_BACK) && det < 0.0f) || ((flags & NGP_RAYCAST_CULL_FRONT) && det > 0.0f);
    if (mixed || det == 0.0f || culled) h.t = NAN;
    return h;
}

// the header comment's enter(box): tn if the node is to be entered for [t_lo, t_hi], else +inf
__device__ __forceinline__ float mesh_ray_box(const float* __restrict__ boxes, long long node, const MeshRay& r, float t_lo, float t_hi) {
    const float* b = boxes + 6 * node;
    const float px0 = b[0] - r.o.x, py0 = b[1] - r.o.y, pz0 = b[2] - r.o.z, px1 = b[3] - r.o.x, py1 = b[4] - r.o.y, pz1 = b[5] - r.o.z;
    const float m = fmaxf(fmaxf(fmaxf(fabsf(px0), fabsf(px1)), fmaxf(fabsf(py0), fabsf(py1))), fmaxf(fabsf(pz0), fabsf(pz1)));
    const float delta = m * MESH_RAYCAST_PAD;
    const float x0 = (px0 - delta) * r.inv.x, x1 = (px1 + delta) * r.inv.x;
    const float y0 = (py0 - delta) * r.inv.y, y1 = (py1 + delta) * r.inv.y;
    const float z0 = (pz0 - delta) * r.inv.z, z1 = (pz1 + delta) * r.inv.z;
    const float near = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    const float far = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    const float tn = near - fabsf(near) * MESH_RAYCAST_GROW, tf = far + fabsf(far) * MESH_RAYCAST_GROW;
    return (b[0] <= b[3] && tn <= tf && tn <= t_hi && tf >= t_lo) ? tn : INFINITY;
}

__device__ __forceinline__ MeshRayFace mesh_ray_face_at(const MeshGeometry& g, long long f, const MeshRay& r, int flags) {
    V3 a, b, c;
    mesh_face_corners(g, f, a, b, c);
    return mesh_ray_face(r, a, b, c, flags);
}

__global__ void __launch_bounds__(MESH_RAYCAST_BLOCK) mesh_raycast_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int n,
                                                                          MeshGeometry g, const float* __restrict__ boxes, float t_min,
                                                                          float t_max, int flags, float* __restrict__ t_out,
                                                                          int32_t* __restrict__ face_out, float* __restrict__ bary,
                                                                          int32_t* __restrict__ side) {
    const long long i = (long long)blockIdx.x * MESH_RAYCAST_BLOCK + threadIdx.x;
    if (i >= n) return;
    MeshRay ray;
    float best = INFINITY;
    int best_pos = -1;
    MeshTally<2> tally;                      // boxes tested, faces tested
    if (mesh_ray_setup(v3_load(rays_o, i), v3_load(rays_d, i), ray) && t_min <= t_max) {
        // mesh_bvh.h, "THE WALK": keep this and mesh_sdf_query_kernel's alike, state for state
        const int first_leaf = g.padded - 1;
        const bool any_hit = (flags & NGP_RAYCAST_ANY_HIT) != 0;
        int node = 0, depth = 0;
        uint32_t trail = 0;
        bool down = mesh_ray_box(boxes, 0, ray, t_min, t_max) < INFINITY;
        tally.add(0);
        for (;;) {
            if (down) {
                if (node >= first_leaf) {
                    const long long s0 = (long long)(node - first_leaf) * g.leaf_size;
                    for (int j = 0; j < g.leaf_size && s0 + j < g.n_faces; ++j) {
                        const float t = mesh_ray_face_at(g, g.order[s0 + j], ray, flags).t;
                        if (t_min <= t && t <= t_max && t < best) { best = t; best_pos = (int)(s0 + j); }
                        tally.add(1);
                    }
                    if (any_hit && best_pos >= 0) break;
                    down = false;
                } else {
                    const int c0 = 2 * node + 1;
                    const float hi = fminf(t_max, best);
                    const float e0 = mesh_ray_box(boxes, c0, ray, t_min, hi), e1 = mesh_ray_box(boxes, c0 + 1, ray, t_min, hi);
                    tally.add(0, 2);
                    if (fminf(e0, e1) < INFINITY) {
                        node = e1 < e0 ? c0 + 1 : c0;
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
                    down = mesh_ray_box(boxes, node, ray, t_min, fminf(t_max, best)) < INFINITY;
                } else {
                    node = (node - 1) >> 1;
                    --depth;
                }
            }
        }
    }
    tally.flush();
    t_out[i] = best;
    if (best_pos < 0) {
        if (face_out) face_out[i] = -1;
        if (bary) { bary[2 * i] = 0.0f; bary[2 * i + 1] = 0.0f; }
        if (side) side[i] = 0;
        return;
    }
    if (!face_out && !bary && !side) return;
    const long long f = g.order[best_pos];
    const MeshRayFace h = mesh_ray_face_at(g, f, ray, flags);       // the same bits as in the walk
    if (face_out) face_out[i] = (int32_t)f;
    if (bary) { bary[2 * i] = h.v; bary[2 * i + 1] = h.w; }
    if (side) side[i] = h.det > 0.0f ? 1 : -1;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_mesh_raycast(const float* rays_o, const float* rays_d, int n, const float* vertices, const int32_t* faces, const int32_t* order,
                     const float* boxes, int n_faces, int leaf_size, float t_min, float t_max, int flags, float* t, int32_t* face,
                     float* bary, int32_t* side, void* stream) {
    MeshGeometry g;
    MeshTree tree;
    if (!boxes || n < 0 || (flags & ~MESH_RAYCAST_FLAGS) || !mesh_geometry(vertices, faces, order, n_faces, leaf_size, g, tree)) return -1;
    if (n == 0) return 0;                    // an empty batch has no rays and no outputs: their pointers may be null
    if (!rays_o || !rays_d || !t) return -1;
    hipLaunchKernelGGL(mesh_raycast_kernel, dim3((unsigned)(((long long)n + MESH_RAYCAST_BLOCK - 1) / MESH_RAYCAST_BLOCK)),
                       dim3(MESH_RAYCAST_BLOCK), 0, (hipStream_t)stream, rays_o, rays_d, n, g, boxes, t_min, t_max, flags, t, face, bary,
                       side);
    NGP_LAUNCH_CHECK();
    return 0;
}

// the microbenchmark's build only (profiles/microbench/mesh_raycast.py binds it by hand): read and clear the two tallies of MeshRayFirst
NGP_MESH_TALLY_ENTRY(ngp_mesh_raycast_counters, 2)

}  // extern "C"

