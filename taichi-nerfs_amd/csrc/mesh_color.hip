// mesh_color.hip -- vertex colours of a triangle mesh from posed images: every vertex projected into every view, the occlusion segment of
// each (vertex, camera) pair written for ngp_mesh_raycast (mesh_raycast.hip, called by the package between the two launches: nothing of
// the walk or of the ray / face test is repeated here), what the views show blended per vertex, and the vertices no view shows filled in
// from their neighbours, for gfx950.  The contract is the comment above ngp_mesh_color_* in include/ngp_hip.h and DESIGN.md section 3,
// "Vertex colours"; tests/mesh_color_reference.py restates it serially.
//
//   mc_project_kernel         a lane per (camera j of the chunk, vertex v) pair, pair = j V + v (camera-major: a wave holds neighbouring
//                             vertices seen from one camera, so its occlusion rays run side by side): the four tests in f32, the
//                             segment, the sample position, cos and the weight cos^2
//       ngp_mesh_raycast over the chunk's pairs, NGP_RAYCAST_ANY_HIT, t in [0, 1]: the package
//   mc_accumulate_kernel<MODE> a lane per vertex: the chunk's cameras in ascending index, four texels and the bilinear mean in f64,
//                             w rgb and w added into the persistent f64 accumulator (BLEND) or kept for the largest cos alone (BEST)
//   mc_finish_kernel          a lane per vertex: sum w rgb / sum w, one rounding to f32
//   mc_fill_kernel            a lane per vertex, one Jacobi round over the CSR of mesh_smooth.hip: the f64 mean of the coloured
//                             neighbours in ascending neighbour order
//
// The f32 expressions of the projection and the f64 expressions of the sums are evaluated as written: the library is compiled with
// -ffp-contract=off, so a product and the sum it feeds are two roundings, never an fma; no fast-math flag is given, so divisions and
// square roots are the correctly rounded ones.  No float atomics and no atomics at all: a vertex is one lane's, its cameras come in
// ascending index whatever the chunk size, so two runs -- and two chunk sizes -- write the same bytes.
#include "ngp_device.h"
#include "mesh_bvh.h"
#include "mesh_edit.h"

namespace ngp {

constexpr int MC_UNCOLOURED = 255;                          // `filled` of a vertex without a colour; a round number stays below it

struct McCamera { V3 right, down, front, centre; float fx, fy, cx, cy; };

// c2w [3,4] row-major = (right, down, front | position): the columns; K [3,3] row-major
__device__ __forceinline__ McCamera mc_camera(const float* __restrict__ K, const float* __restrict__ c2w) {
    McCamera m;
    m.right = {c2w[0], c2w[4], c2w[8]};
    m.down = {c2w[1], c2w[5], c2w[9]};
    m.front = {c2w[2], c2w[6], c2w[10]};
    m.centre = {c2w[3], c2w[7], c2w[11]};
    m.fx = K[0]; m.cx = K[2]; m.fy = K[4]; m.cy = K[5];
    return m;
}

__device__ __forceinline__ bool v3_finite(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ __forceinline__ void v3_store(float* __restrict__ p, long long i, V3 a) { p[3 * i] = a.x; p[3 * i + 1] = a.y; p[3 * i + 2] = a.z; }

__global__ void __launch_bounds__(256) mc_project_kernel(const float* __restrict__ vertices, const float* __restrict__ normals, int n_vertices,
                                                         const float* __restrict__ K, int k_per_camera, const float* __restrict__ c2w,
                                                         int n_cameras, float w_max, float h_max, const float* __restrict__ eps_ptr,
                                                         float cos_min, float near, int two_sided, float* __restrict__ rays_o,
                                                         float* __restrict__ rays_d, float* __restrict__ sample, float* __restrict__ weight,
                                                         float* __restrict__ cosv) {
    const long long pair = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pair >= (long long)n_vertices * n_cameras) return;
    const int j = (int)(pair / n_vertices);
    const long long v = pair - (long long)j * n_vertices;
    const McCamera cam = mc_camera(K + (k_per_camera ? 9ll * j : 0), c2w + 12ll * j);
    const V3 x = v3_load(vertices, v);
    V3 n = v3_load(normals, v);
    V3 o = {0.0f, 0.0f, 0.0f}, dir = {0.0f, 0.0f, 0.0f};              // a zero direction: ngp_mesh_raycast writes a miss without a walk
    float su = 0.0f, sw = 0.0f, w = 0.0f, cs = 0.0f;
    if (v3_finite(x) && v3_finite(n)) {
        const V3 d = v3_sub(cam.centre, x);
        float nd = v3_dot(n, d);
        if (two_sided && nd < 0.0f) { n = {-n.x, -n.y, -n.z}; nd = -nd; }
        const float c = nd / sqrtf(v3_dot(d, d));
        const V3 q = v3_sub(x, cam.centre);
        const float px = v3_dot(cam.right, q), py = v3_dot(cam.down, q), pz = v3_dot(cam.front, q);
        const float u = cam.fx * px / pz + cam.cx, t = cam.fy * py / pz + cam.cy;
        const float a = u - 0.5f, b = t - 0.5f;
        if (c > cos_min && pz > near && a >= 0.0f && a <= w_max && b >= 0.0f && b <= h_max) {          // a NaN fails its comparison
            o = v3_add(x, v3_scale(n, eps_ptr[0]));
            dir = v3_sub(cam.centre, o);
            su = a; sw = b; cs = c; w = c * c;
        }
    }
    v3_store(rays_o, pair, o);
    v3_store(rays_d, pair, dir);
    sample[2 * pair] = su;
    sample[2 * pair + 1] = sw;
    weight[pair] = w;
    cosv[pair] = cs;
}

// the bilinear mean of channel c at (x0 + fx, y0 + fy) in f64: the two rows first, then between them
__device__ __forceinline__ double mc_bilinear(const float* __restrict__ r0, const float* __restrict__ r1, long long i0, long long i1, int c,
                                              double fx, double fy) {
    const double top = (1.0 - fx) * (double)r0[i0 + c] + fx * (double)r0[i1 + c];
    const double bottom = (1.0 - fx) * (double)r1[i0 + c] + fx * (double)r1[i1 + c];
    return (1.0 - fy) * top + fy * bottom;
}

template <int MODE>
__global__ void __launch_bounds__(256) mc_accumulate_kernel(const float* __restrict__ images, int n_cameras, int height, int width, int channels,
                                                            int n_vertices, const float* __restrict__ sample, const float* __restrict__ weight,
                                                            const float* __restrict__ cosv, const float* __restrict__ t,
                                                            double* __restrict__ accum, int32_t* __restrict__ views,
                                                            float* __restrict__ best_cos) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    double s[4] = {accum[4 * v], accum[4 * v + 1], accum[4 * v + 2], accum[4 * v + 3]};
    int count = views[v];
    float best = MODE == NGP_MESH_COLOR_BEST ? best_cos[v] : 0.0f;
    for (int j = 0; j < n_cameras; ++j) {                               // ascending camera index
        const long long pair = (long long)j * n_vertices + v;
        const float w = weight[pair];
        if (!(w > 0.0f) || t[pair] < INFINITY) continue;                // rejected, or something of the mesh between the vertex and the camera
        const float c = cosv[pair];
        if (MODE == NGP_MESH_COLOR_BEST && !(c > best)) continue;       // strictly: of equal cos the lower index stays
        const float a = sample[2 * pair], b = sample[2 * pair + 1];
        int x0 = (int)floorf(a), y0 = (int)floorf(b);
        x0 = x0 < 0 ? 0 : (x0 > width - 1 ? width - 1 : x0);           // the projection has tested both; an index is clamped all the same
        y0 = y0 < 0 ? 0 : (y0 > height - 1 ? height - 1 : y0);
        const int x1 = x0 + 1 > width - 1 ? width - 1 : x0 + 1, y1 = y0 + 1 > height - 1 ? height - 1 : y0 + 1;
        const double fx = (double)(a - (float)x0), fy = (double)(b - (float)y0);
        const float* r0 = images + ((long long)j * height + y0) * width * channels;
        const float* r1 = images + ((long long)j * height + y1) * width * channels;
        const long long i0 = (long long)x0 * channels, i1 = (long long)x1 * channels;
        const double dw = (double)w;
        if (MODE == NGP_MESH_COLOR_BEST) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = dw * mc_bilinear(r0, r1, i0, i1, k, fx, fy);
            s[3] = dw;
            count = 1;
            best = c;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] += dw * mc_bilinear(r0, r1, i0, i1, k, fx, fy);
            s[3] += dw;
            ++count;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) accum[4 * v + k] = s[k];
    views[v] = count;
    if (MODE == NGP_MESH_COLOR_BEST) best_cos[v] = best;
}

__global__ void __launch_bounds__(256) mc_finish_kernel(const double* __restrict__ accum, const int32_t* __restrict__ views, int n_vertices,
                                                        float* __restrict__ colors, float* __restrict__ weight, uint8_t* __restrict__ filled) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    const bool seen = views[v] > 0;
    const double sw = accum[4 * v + 3];
#pragma unroll
    for (int k = 0; k < 3; ++k) colors[3 * v + k] = seen ? (float)(accum[4 * v + k] / sw) : 0.0f;
    weight[v] = seen ? (float)sw : 0.0f;
    filled[v] = seen ? 0 : MC_UNCOLOURED;
}

// colours are written in place: a round writes only vertices that were uncoloured when it began and reads only vertices that were not
__global__ void __launch_bounds__(256) mc_fill_kernel(float* colors, const uint8_t* __restrict__ filled_in, uint8_t* __restrict__ filled_out,
                                                      const int32_t* __restrict__ row_start, const int32_t* __restrict__ neighbours,
                                                      int n_vertices, long long n_slots, int round) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    int state = filled_in[v];
    if (state == MC_UNCOLOURED) {
        long long e0 = row_start[v], e1 = row_start[v + 1];
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > n_slots ? n_slots : e1;
        double s[3] = {0.0, 0.0, 0.0};
        int count = 0;
        for (long long e = e0; e < e1; ++e) {                           // ascending neighbour index: the row's order
            const int j = neighbours[e];
            if ((unsigned)j >= (unsigned)n_vertices || filled_in[j] == MC_UNCOLOURED) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] += (double)colors[3ll * j + k];
            ++count;
        }
        if (count > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) colors[3 * v + k] = (float)(s[k] / (double)count);
            state = round;
        }
    }
    filled_out[v] = (uint8_t)state;
}

}  // namespace ngp

using namespace ngp;

extern "C" {

int ngp_mesh_color_project(const float* vertices, const float* normals, int n_vertices, const float* K, int k_per_camera, const float* c2w,
                           int n_cameras, int width, int height, const float* eps, float cos_min, float near, int two_sided, float* rays_o,
                           float* rays_d, float* sample, float* weight, float* cosv, void* stream) {
    if (!vertices || !normals || !K || !c2w || !eps || !rays_o || !rays_d || !sample || !weight || !cosv) return -1;
    if (n_vertices < 1 || n_cameras < 1 || width < 1 || height < 1 || (long long)n_vertices * n_cameras > 0x7fffffffll) return -1;
    if (!(cos_min >= 0.0f) || !(near >= 0.0f)) return -1;                              // negative or NaN
    const long long pairs = (long long)n_vertices * n_cameras;
    hipLaunchKernelGGL(mc_project_kernel, dim3(mesh_blocks(pairs, 256)), dim3(256), 0, (hipStream_t)stream, vertices, normals, n_vertices, K,
                       k_per_camera ? 1 : 0, c2w, n_cameras, (float)(width - 1), (float)(height - 1), eps, cos_min, near, two_sided ? 1 : 0,
                       rays_o, rays_d, sample, weight, cosv);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_color_accumulate(const float* images, int n_cameras, int height, int width, int channels, int n_vertices, const float* sample,
                              const float* weight, const float* cosv, const float* t, int mode, double* accum, int32_t* views,
                              float* best_cos, void* stream) {
    if (!images || !sample || !weight || !cosv || !t || !accum || !views) return -1;
    if (n_vertices < 1 || n_cameras < 1 || width < 1 || height < 1 || channels < 3 || (long long)n_vertices * n_cameras > 0x7fffffffll) return -1;
    if (mode != NGP_MESH_COLOR_BLEND && mode != NGP_MESH_COLOR_BEST) return -1;
    if (mode == NGP_MESH_COLOR_BEST && !best_cos) return -1;
    const dim3 grid(mesh_blocks(n_vertices, 256)), block(256);
    if (mode == NGP_MESH_COLOR_BEST)
        hipLaunchKernelGGL(mc_accumulate_kernel<NGP_MESH_COLOR_BEST>, grid, block, 0, (hipStream_t)stream, images, n_cameras, height, width,
                           channels, n_vertices, sample, weight, cosv, t, accum, views, best_cos);
    else
        hipLaunchKernelGGL(mc_accumulate_kernel<NGP_MESH_COLOR_BLEND>, grid, block, 0, (hipStream_t)stream, images, n_cameras, height, width,
                           channels, n_vertices, sample, weight, cosv, t, accum, views, best_cos);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_color_finish(const double* accum, const int32_t* views, int n_vertices, float* colors, float* weight, uint8_t* filled,
                          void* stream) {
    if (!accum || !views || !colors || !weight || !filled || n_vertices < 1) return -1;
    hipLaunchKernelGGL(mc_finish_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream, accum, views, n_vertices, colors,
                       weight, filled);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mesh_color_fill(float* colors, const uint8_t* filled_in, uint8_t* filled_out, const int32_t* row_start, const int32_t* neighbours,
                        int n_vertices, long long n_slots, int round, void* stream) {
    if (!colors || !filled_in || !filled_out || filled_in == filled_out || !row_start || !neighbours) return -1;
    if (n_vertices < 1 || n_slots < 0 || n_slots > 0x7fffffffll || round < 1 || round >= MC_UNCOLOURED) return -1;
    hipLaunchKernelGGL(mc_fill_kernel, dim3(mesh_blocks(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream, colors, filled_in, filled_out,
                       row_start, neighbours, n_vertices, n_slots, round);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
