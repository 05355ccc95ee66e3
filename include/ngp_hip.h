/*
 * ngp_hip.h -- C ABI of libngp_hip.so: the MI355X (gfx950) Instant-NGP training hot path.
 *
 * This is the drop-in boundary under the Python surface of the reference's `modules/` package
 * (taichi-dev/taichi-nerfs).  Every entry point replaces ONE Taichi kernel launch of the reference;
 * the reference file:line each one stands in for is cited next to it.  The reference binds its kernels
 * through Taichi's torch zero-copy interop (tensor -> raw device pointer); the binding a maintainer adds
 * instead is the ctypes stub shown in INTEGRATION.md (taichi-nerfs_amd/ngp_hip/lib.py derives it from this file).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers + explicit sizes; no torch types; no allocation; no host sync
 *     (the only exception is ngp_march_train_total, which is an explicit D2H read).
 *   - every function returns 0 on success, or the negated hipError_t of the failing launch.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - all geometric data is f32, `rays_a` is i32, alive/ray indices are i64 -- as in the reference.
 *   - arrays are dense row-major ("contiguous" in torch terms); the reference wrappers call
 *     .contiguous() before every launch (hash_encoder.py:283, volume_train.py:188, rendering.py:34).
 */
#ifndef NGP_HIP_H
#define NGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGP_MAX_LEVELS 16
#define NGP_ABI_VERSION 3

/* Multiresolution level table.  Built ONCE on the host (ngp_hash_levels_init) in the arithmetic of
 * modules/hash_encoder.py:183-205 + modules/utils.py:19-42 (f64 sizes) and of the in-kernel
 * grid_scale/grid_resolution (hash_encoder.py:73-80, f32) and handed to every hash kernel by value, so
 * the CPU oracle and the HIP kernels index with the very same numbers. */
typedef struct ngp_hash_levels {
    int32_t  n_levels;                 /* L, <= NGP_MAX_LEVELS                                  */
    int32_t  n_features;               /* F, features per entry (2)                             */
    int32_t  begin_fast_hash_level;    /* first level that uses the xor-prime hash              */
    int32_t  total_entries;            /* sum of map_size                                       */
    float    scale[NGP_MAX_LEVELS];    /* base*exp(l*log_b)-1, f32                              */
    uint32_t resolution[NGP_MAX_LEVELS]; /* ceil(scale)+1                                       */
    uint32_t map_size[NGP_MAX_LEVELS]; /* entries in level l                                    */
    uint32_t offset[NGP_MAX_LEVELS];   /* first entry of level l                                */
    uint32_t bwd_plan;                 /* NGP_BWD_PLAN_* bits: task plan of the LDS-sliced scatter-add over this table
                                          (ngp_hash_bwd_sliced_*); 0 after ngp_hash_levels_init; every other entry point ignores it */
} ngp_hash_levels;

/* Task-plan modes of the LDS-sliced scatter-add (ngp_hash_levels.bwd_plan).  They are part of the level table the caller hands to
 * EVERY ngp_hash_bwd_sliced_* call of one step (prep, main*, adam_prefix, plan must see the same bits): the library keeps no mode
 * state of its own (until ABI version 1 these were per-thread switches, ngp_hash_bwd_sliced_deterministic / _concentrated).
 * DETERMINISTIC: the default plan replicates the coarse levels over sample ranges whose owners meet in dtable with float atomics
 *   (order-dependent at ~1e-7) and pre-sums equal-cell runs in groups that depend on which wave took which piece of the sample list.
 *   With this bit every slice has ONE owner (no float atomics; with _main_adam the optimizer runs in the flush of EVERY level,
 *   _adam_prefix = 0) and a pre-summing group never spans two pieces: the result is a function of the inputs.  Slower on the coarse
 *   levels; bench.py conditions its model in this mode so that two processes reach the same state.
 * CONCENTRATED: for scenes that fill a small part of the box (multi-cascade scenes) the coarse hashed levels (resolution <= 256) get
 *   sample-range replicas like the dense ones -- a few hot cells otherwise load a handful of slice owners with several times the mean
 *   (C3: the launch 2.2 ms with the XCDs busy 55 % of it; 1.7 ms in this mode).  The levels that get replicas leave the set
 *   ngp_hash_bwd_sliced_main_adam updates in its flush (ngp_hash_bwd_sliced_adam_prefix says where that set starts). */
#define NGP_BWD_PLAN_DETERMINISTIC 1u
#define NGP_BWD_PLAN_CONCENTRATED  2u

int ngp_abi_version(void);

/* Entry points that NO default path of the package calls (earlier rounds' forms kept for A/B runs, the overlapped-exchange experiment, host-side
 * introspection and diagnostics) are declared in ngp_hip_experimental.h; the library exports both sets. */

/* Host-only helper: fills `lv` like HashEncoder.__init__ (hash_encoder.py:183-205). Returns 0. */
int ngp_hash_levels_init(ngp_hash_levels* lv, double max_params, int levels, double base_res,
                         double max_res, int features);

/* ---- a-1  ray_aabb_intersect (modules/intersection.py:8-37) ---------------------------------- */
int ngp_ray_aabb(const float* rays_o, const float* rays_d, float scale, int n_rays,
                 float* hits_t /*[n,2]*/, void* stream);

/* ---- a-2  raymarching_train_kernel (modules/ray_march.py:8-123) ------------------------------
 * The reference's single kernel (count pass, two global atomics per ray, write pass) is split into
 * three deterministic launches:
 *   count : one lane per ray walks the f32 orbit once, stores every emitted (t,dt) into the ray's
 *           private staging row stage[r*max_samples + k] and its sample count into counts[r];
 *   scan  : exclusive prefix sum over counts -> rays_a[r] = (r, start, count) IN RAY ORDER and
 *           total[0] = number of samples (replaces counter[0]/counter[1] atomics, ray_march.py:76-81);
 *   write : sample-parallel expansion of the staged (t,dt) into xyzs/dirs/deltas/ts.            */
/* (hits_t may be NULL in the _ex form below: the slab test of ngp_ray_aabb is then evaluated inline.) */
/* Optional acceleration of `count`: coarse[k] bit = any occupied cell among the 512 Morton codes of 8^3-cell block k
 * (built by ngp_bitfield_coarsen whenever the bitfield changes; cascades*grid^3/512 bits).  Purely a shortcut for
 * provably empty cells -- results are bit-identical with coarse == NULL. */
int ngp_bitfield_coarsen(const uint8_t* density_bitfield, int cascades, int grid_size, uint32_t* coarse,
                         void* stream);
int ngp_march_train_count_ex(const float* rays_o, const float* rays_d, const float* hits_t,
                             const uint8_t* density_bitfield, const uint32_t* coarse, const float* noise,
                             int cascades, int grid_size, float scale, float exp_step_factor, int max_samples,
                             int n_rays, float* stage, int32_t* counts, void* stream);
/* The whole training march in ONE launch (count + allocation + expansion): a 16-wave block marches 32 rays, takes its output
 * range from ctr[0] with one atomic add and writes its rays' samples itself.  Per ray the samples are those of the chain above
 * (bit for bit, contiguous, in march order); the rays follow each other in the order their blocks finished, as in the reference
 * (ray_march.py:76-80: N_eff_samples / counter atomic adds) -- rays_a[r] = (r, start, count) says where.  ctr = [2] int32 scratch,
 * zero before the FIRST launch only (the kernel leaves it zero); total[0] = number of samples.  hits_t / coarse nullable as in
 * ngp_march_train_count_ex; stage = [n_rays * max_samples * 2] scratch. */
int ngp_march_train_fused(const float* rays_o, const float* rays_d, const float* hits_t,
                          const uint8_t* density_bitfield, const uint32_t* coarse, const float* noise, int cascades,
                          int grid_size, float scale, float exp_step_factor, int max_samples, int n_rays,
                          float* stage, int32_t* ctr, int32_t* rays_a, int32_t* total, float* xyzs, float* dirs,
                          float* deltas, float* ts, void* stream);
/* ngp_march_train_fused writes start + k for every emitted sample: xyzs / dirs / deltas / ts must have n_rays * max_samples rows.
 * With smaller arrays use this form: samples at or beyond `capacity` rows are dropped, total[0] still counts them. */
int ngp_march_train_fused_cap(const float* rays_o, const float* rays_d, const float* hits_t, const uint8_t* density_bitfield,
                              const uint32_t* coarse, const float* noise, int cascades, int grid_size, float scale,
                              float exp_step_factor, int max_samples, int n_rays, long long capacity, float* stage, int32_t* ctr,
                              int32_t* rays_a, int32_t* total, float* xyzs, float* dirs, float* deltas, float* ts, void* stream);
/* The same with the jitter drawn in the kernel: ray r gets rng_uniform(seed, r) (splitmix64 -> 24-bit uniform in [0, 1); the
 * reference draws torch.rand_like, ray_march.py:138).  ngp_rng_uniform writes those values out (tests / callers wanting a tensor). */
int ngp_march_train_fused_rng(const float* rays_o, const float* rays_d, const float* hits_t, const uint8_t* density_bitfield,
                              const uint32_t* coarse, unsigned long long seed, int cascades, int grid_size, float scale,
                              float exp_step_factor, int max_samples, int n_rays, float* stage, int32_t* ctr, int32_t* rays_a,
                              int32_t* total, float* xyzs, float* dirs, float* deltas, float* ts, void* stream);
/* Round 5: the same launch with its SHAPE chosen by the caller (the side-stream prefetch of FusedTrainer puts the march underneath
 * other kernels of the step): block_waves in {4, 8, 16} waves per block (16 = the entry points above), lds_pad_bytes of dynamic
 * LDS the kernel never touches (caps the blocks one CU takes at a time; 0 = none).  noise == NULL: jitter rng_uniform(seed, r),
 * else the vector (seed ignored).  Per ray the samples are bit for bit those of every other form (ray_march.py:8-123). */
int ngp_march_train_fused_shaped(const float* rays_o, const float* rays_d, const float* hits_t, const uint8_t* density_bitfield,
                                 const uint32_t* coarse, const float* noise, unsigned long long seed, int cascades, int grid_size,
                                 float scale, float exp_step_factor, int max_samples, int n_rays, int block_waves, int lds_pad_bytes,
                                 float* stage, int32_t* ctr, int32_t* rays_a, int32_t* total, float* xyzs, float* dirs, float* deltas,
                                 float* ts, void* stream);
int ngp_rng_uniform(unsigned long long seed, int n, float* out, void* stream);
int ngp_march_train_scan(const int32_t* counts, int n_rays, int32_t* rays_a /*[n,3]*/,
                         int32_t* total /*[1]*/, void* stream);
int ngp_march_train_write(const float* rays_o, const float* rays_d, const int32_t* rays_a,
                          const float* stage, int max_samples, int n_rays,
                          float* xyzs, float* dirs, float* deltas, float* ts, void* stream);

/* ---- a-3  raymarching_test_kernel (modules/ray_march.py:197-268) ----------------------------- */
int ngp_march_test(const float* rays_o, const float* rays_d, float* hits_t /*in-out*/,
                   const int64_t* alive_indices, const uint8_t* density_bitfield,
                   int cascades, int grid_size, float scale, float exp_step_factor,
                   int max_samples, int n_alive,
                   int64_t* ray_indices, uint8_t* valid_mask, float* deltas, float* ts,
                   int32_t* samples_counter, void* stream);

/* ---- a-4  hash_encoder_kernel fp32 + its autodiff backward (modules/hash_encoder.py:89-143,269) */
int ngp_hash_fwd_f32(const float* xyzs /*[n,3] in [0,1]*/, const float* table,
                     const ngp_hash_levels* lv, int n, float* out /*[n, L*F]*/, void* stream);
/* dtable must be zero-filled by the caller (or hold a gradient to accumulate into). */
int ngp_hash_bwd_f32(const float* xyzs, const float* dout /*[n, L*F]*/,
                     const ngp_hash_levels* lv, int n, float* dtable, void* stream);

/* ---- a-4x  gradient of the encoding with respect to the sample POSITION (csrc/hash_grad_input.hip; not in the reference, whose
 * backward returns None for the positions, hash_encoder.py:277).  dxyzs [n,3] is WRITTEN, every element, never accumulated:
 *   dx_k = sum_l scale_l * sum_f denc[l,f] * sum_c s_k(c) * prod_{j != k} w_j(c) * T[off_l + idx_c, f]
 * with s_k(c) = +1 where corner c lies on the far side along axis k and -1 otherwise, w_j(c) = fr_j on the far side and 1 - fr_j
 * otherwise: the derivative of the forward as the forward evaluates it (its f32 cell and fraction, d fr / d pos = 1).
 * Face rule: on a cell face (fr == 0) it is the derivative of the cell floorf selects, i.e. the one-sided derivative towards larger
 * coordinates.  Positions outside [0, 1] and NaN positions take the cell the forward gives them; no read leaves the table (a NaN
 * position yields a NaN row and touches no other row).  Products and sums are f32; the sum over levels is a fixed shuffle tree (no
 * atomics): two runs on the same input are bit-identical.  denc is the natural [n, L*F] layout.  n == 0 returns 0 without a launch.
 * These entries are first order; the double backward through dx is ngp_hash_bwd2_* below.
 * ngp_hash_bwd_input_f32 differentiates ngp_hash_fwd_f32: same (L, F) domain (1 <= L <= 16, F in {1, 2, 4, 8}), -1 outside it. */
int ngp_hash_bwd_input_f32 (const float* xyzs, const float* table, const float* denc /*[n, L*F]*/, const ngp_hash_levels* lv, int n,
                            float* dxyzs /*[n,3]*/, void* stream);
/* Differentiates ngp_hash_fwd_bf16_ex (normalize = 0, natural layout): the bf16 storage copy the forward read (F = 2), widened
 * exactly; same face rule.  Equals ngp_hash_bwd_input_f32 on the bf16-rounded table, bit for bit. */
int ngp_hash_bwd_input_bf16(const float* xyzs, const uint16_t* table, const float* denc /*[n, L*2]*/, const ngp_hash_levels* lv, int n,
                            float* dxyzs /*[n,3]*/, void* stream);
/* Differentiates ngp_hash_fwd_f16 (the half2 encoder, F = 2): f16 table entries and f16 denc, widened exactly, and the forward's
 * f16-rounded cell in the fraction; same face rule.  The forward's f16 roundings of its products and sums are not differentiated. */
int ngp_hash_bwd_input_f16 (const float* xyzs, const uint16_t* table, const uint16_t* denc /*[n,L,2] f16*/, const ngp_hash_levels* lv,
                            int n, float* dxyzs /*[n,3]*/, void* stream);

/* ---- a-4xx  double backward through dxyzs (csrc/hash_grad_input2.hip): for ddx [n,3] the gradient of a loss with respect to the dxyzs
 * of ngp_hash_bwd_input_*, and A_c = sum_k ddx_k * s_k(c) * prod_{j != k} w_j(c),
 *   d_denc[l,f]            = scale_l * sum_c A_c * T[off_l + idx_c, f]
 *   d_xyzs[m]              = sum_l scale_l^2 * sum_{k != m} ddx_k * M_km,
 *                            M_km = sum_b w_j(b) * (t[1_k,1_m,b] - t[0_k,1_m,b] - t[1_k,0_m,b] + t[0_k,0_m,b]),  t_c = denc[l,:] . T_c
 *   dtable[off_l + idx_c,f] += scale_l * A_c * denc[l,f]
 * (j the third axis; the diagonal M_kk is exactly 0).  Same cell, fraction, face rule and (L, F) domain as the first backward; no
 * access leaves the table for any input.  The gather entries WRITE d_denc [n, L*F] and d_xyzs [n,3], every element, without atomics
 * (bit-identical from run to run); either pointer may be NULL and that output is skipped.  ngp_hash_bwd2_gather_bf16 reads the bf16
 * storage copy (F = 2) and equals the f32 entry on the bf16-rounded table bit for bit.  ngp_hash_bwd2_table_f32 ACCUMULATES into
 * dtable with float atomics like ngp_hash_bwd_f32 (summation order not deterministic) and skips contributions that are exactly 0;
 * it does not read the table, so it serves both encoders (the bf16-copy encoder's gradient goes to the fp32 master).
 * n <= 0 returns 0 without a launch; an (L, F) outside the forward's domain returns -1. */
int ngp_hash_bwd2_gather_f32 (const float* xyzs, const float* table, const float* denc /*[n, L*F]*/, const float* ddx /*[n,3]*/,
                              const ngp_hash_levels* lv, int n, float* d_denc /*[n, L*F] or NULL*/, float* d_xyzs /*[n,3] or NULL*/,
                              void* stream);
int ngp_hash_bwd2_gather_bf16(const float* xyzs, const uint16_t* table, const float* denc /*[n, L*2]*/, const float* ddx /*[n,3]*/,
                              const ngp_hash_levels* lv, int n, float* d_denc /*[n, L*2] or NULL*/, float* d_xyzs /*[n,3] or NULL*/,
                              void* stream);
int ngp_hash_bwd2_table_f32  (const float* xyzs, const float* denc /*[n, L*F]*/, const float* ddx /*[n,3]*/, const ngp_hash_levels* lv,
                              int n, float* dtable /* += */, void* stream);

/* Sync-free forms used by the fused training step: the sample count is read ON THE DEVICE from n_dev[0] (the
 * `total` written by ngp_march_train_scan; NULL = use n_max), buffers are sized for n_max, and `normalize` fuses the
 * caller-side position normalisation (x - lo) / (hi - lo) of modules/networks.py:144 (same two f32 operations).
 * enc_pairs = 1 (L = 16, F = 2 only) selects the PAIR-MAJOR encoding layout of the fused path:
 *     enc[(p * n_max + i) * 4 + slot],  plane p = min(l, 15 - l),  slot = 2 * (l >= 8) + f
 * i.e. eight [n_max, 4] planes, each written by the workgroups of one XCD (16 contiguous bytes per sample). */
int ngp_hash_fwd_f32_ex(const float* xyzs, const float* table, const ngp_hash_levels* lv, int n_max,
                        const int32_t* n_dev, int normalize, float lo, float hi, int enc_pairs, float* out,
                        void* stream);
/* bf16-stored table (F = 2; entries packed as bf16 pairs): f32 interpolation and f32 output, i.e. bit-identical to
 * ngp_hash_fwd_f32_ex on the bf16-rounded table at half the gather bytes (588 B/sample algorithmic).  The gradient of the
 * encoding w.r.t. the table does not depend on the table values: the backward is ngp_hash_bwd_f32_ex into the fp32 master
 * gradient. */
int ngp_hash_fwd_bf16_ex(const float* xyzs, const uint16_t* table, const ngp_hash_levels* lv, int n_max,
                         const int32_t* n_dev, int normalize, float lo, float hi, int enc_pairs, float* out,
                         void* stream);
/* Round 5 -- the same encoder over a LIST of samples (the chunked forward below): rows list[0 .. *n_list) of xyzs are encoded into
 * the same rows of out (16 levels x 2 features; pair-major planes of stride n_max when enc_pairs).  table_kind 0: fp32 table,
 * 1: its bf16 storage copy.  Bit-identical per row to ngp_hash_fwd_f32_ex / _bf16_ex (hash_encoder.py:89-143).  Returns -2 where
 * the specialised kernel does not apply (other table shapes; tables of 4 GB and more): the caller encodes every row instead. */
int ngp_hash_fwd_list(const float* xyzs, const void* table, int table_kind, const ngp_hash_levels* lv, int n_max,
                      const int32_t* n_list, const int32_t* list, int normalize, float lo, float hi, int enc_pairs, float* out,
                      void* stream);
/* found_inf (nullable): set to 1 when a non-finite incoming gradient is seen -- GradScaler's inf/nan check
 * (train.py:199) done where the data passes instead of in an extra pass over the 45.7 MB gradient. */

/* ---- a-4t  triplane_encoder_kernel fp32 + its autodiff backward (modules/triplane.py:35-98, glue :103-204) --------
 * Level table of the tri-plane encoder (TriPlaneEncoder.__init__, triplane.py:103-160): the same f32 grid_scale / grid_resolution
 * arithmetic as ngp_hash_levels (triplane.py:27-33), plus the full resolution every level's corners are mapped to.  Built on the
 * host by ngp_triplane_levels_init and passed by pointer; the kernels copy what they need. */
typedef struct ngp_triplane_levels {
    int32_t  n_levels;                   /* L, <= NGP_MAX_LEVELS (the reference's NGP: 8)                        */
    int32_t  n_features;                 /* F, features per entry (the reference's NGP: 4; the kernels take 4)   */
    int32_t  max_res;                    /* side of each of the three planes, <= 16384                           */
    int32_t  reserved;                   /* 0                                                                    */
    float    scale[NGP_MAX_LEVELS];      /* base*exp(l*log_b)-1, f32                                             */
    uint32_t resolution[NGP_MAX_LEVELS]; /* ceil(scale)+1                                                        */
} ngp_triplane_levels;

/* Host-only helper: fills `lv` like TriPlaneEncoder.__init__ (log_b = ln(max_res/base_res)/(L-1)). Returns 0, or -1 for bad arguments. */
int ngp_triplane_levels_init(ngp_triplane_levels* lv, double base_res, double max_res, int levels, int features);
/* Forward: replaces one launch of the reference's triplane_encoder_kernel (triplane.py:35-98, launched at :170).
 * table = [3, max_res^2, F] f32 (planes (x,y), (y,z), (z,x)); out = [n, L*F] f32, FEATURE-major (column j*L + level).
 * `normalize` fuses (x - lo) / (hi - lo) (networks.py:144) like ngp_hash_fwd_f32_ex; positions are then clamped to [0, 1]
 * (the reference indexes out of bounds outside it).  Bit-exact to the reference's f32 arithmetic. */
int ngp_triplane_fwd_f32(const float* xyzs /*[n,3]*/, const float* table, const ngp_triplane_levels* lv, int n, int normalize,
                         float lo, float hi, float* out /*[n, L*F]*/, void* stream);
/* Backward: replaces the Taichi-autodiff launch `_encode_kernel.grad` (triplane.py:186-198).  dtable += d out / d table for
 * dout = d loss / d out: the TRUE gradient (the reference's glue returns the leaf's own .grad, which autograd adds a second time:
 * 2x).  The gradient depends on the table values, which are read again here.  dtable must be zero-filled by the caller (or hold a
 * gradient to accumulate into); float atomics: the summation order is not fixed. */
int ngp_triplane_bwd_f32(const float* xyzs, const float* dout /*[n, L*F]*/, const float* table, const ngp_triplane_levels* lv,
                         int n, int normalize, float lo, float hi, float* dtable, void* stream);

/* ---- a-4v  VoxelGrid.forward / query_grids + sh_utils.eval_sh and their backward (modules/networks.py:382-575, sh_utils.py:58-113)
 * The reference's svox model never ran (its forward names undefined variables); these entry points are the lookup its helpers
 * describe: normalize_samples (:521-522), query_grids(use_trilinear=False) (:546-559) with out_of_grid (:491-508), eval_sh of degree
 * 0-4 per colour channel (:572-574), and the PlenOctrees activations sigma = relu(density), rgb = sigmoid(SH) (voxel grid).
 * sh = [G, G, G, 3*D] f32 with D = (sh_degree+1)^2, channel-major (R's D coefficients, then G's, then B's); density = [G, G, G] f32;
 * (x, y, z) 'ij' order.  Sample p reads row (ix*G + iy)*G + iz, i = rint((p - grid_min) / grid_radius) per axis (f32, IEEE divide,
 * half-to-even like torch.round); an axis outside [0, G) gives the all-zero row: sigma = 0, rgb = sigmoid(0) = 0.5, no gradient.
 * grid_min = f32(1 - ceil(G/2)) * f32(grid_radius) (grid_normalized_coords.min(0), :470-478).  G <= 1024, 64-bit row offsets. */
int ngp_voxel_fwd(const float* xyzs /*[n,3]*/, const float* dirs /*[n,3], any length*/, const float* sh, const float* density, int n,
                  int grid_size, int sh_degree, float grid_min, float grid_radius, float* sigmas /*[n]*/, float* rgbs /*[n,3]*/,
                  void* stream);
/* Density only (the occupancy update's query, networks.py:255-290 on VoxelGrid.density). */
int ngp_voxel_density(const float* xyzs, const float* density, int n, int grid_size, float grid_min, float grid_radius,
                      float* sigmas, void* stream);
/* Backward of ngp_voxel_fwd: dsh += d loss / d sh, ddensity += d loss / d density, from the saved sigmas / rgbs (the relu passes the
 * gradient where sigma > 0, the sigmoid's derivative is rgb (1 - rgb)); the row is recomputed from xyzs, the field is not read.
 * dsh / ddensity must be zero-filled by the caller (or hold a gradient to accumulate into); float atomics: the order is not fixed. */
int ngp_voxel_bwd(const float* xyzs, const float* dirs, const float* sigmas, const float* rgbs, const float* dsigmas /*[n]*/,
                  const float* drgbs /*[n,3]*/, int n, int grid_size, int sh_degree, float grid_min, float grid_radius, float* dsh,
                  float* ddensity, void* stream);
/* Trilinear form of the three calls above: query_grids(use_trilinear=True) (:546-561) with trilinear_interpolation (:524-533) and
 * out_of_grid (:489-508); upstream's arithmetic behind that switch cannot run, so the contract is stated here (voxel grid).
 * u = (p - grid_min) / grid_radius per axis (f32, IEEE divide), b = floor(u), f = u - b; the corners are b + (i, j, k), i, j, k in
 * {0, 1}.  A corner with a coordinate outside [0, G) reads the all-zero row and gets no gradient, without renormalisation (grid_sample's
 * zero padding with align_corners); a sample with any u < -1, u >= G or NaN gives sigma = 0, rgb = 0.5 and no gradient.  The raw row
 * (3*D SH coefficients and the density) is interpolated by nested lerps a + t (b - a), z first, then y, then x -- this form returns a
 * constant field exactly -- and then activated: sigma = relu(density), rgb_c = sigmoid(sum_k Y_k sh_{c,k}) (the three dot products
 * are formed per corner and interpolated: eval_sh is linear). */
int ngp_voxel_trilinear_fwd(const float* xyzs /*[n,3]*/, const float* dirs /*[n,3], any length*/, const float* sh, const float* density,
                            int n, int grid_size, int sh_degree, float grid_min, float grid_radius, float* sigmas /*[n]*/,
                            float* rgbs /*[n,3]*/, void* stream);
/* Density only, bit for bit the sigmas of ngp_voxel_trilinear_fwd (the occupancy update's query, networks.py:255-290). */
int ngp_voxel_trilinear_density(const float* xyzs, const float* density, int n, int grid_size, float grid_min, float grid_radius,
                                float* sigmas, void* stream);
/* Backward of ngp_voxel_trilinear_fwd from the saved sigmas / rgbs: with w the product of the corner's per-axis factors (1 - f or f),
 * ddensity[corner] += w [sigma > 0] dsigma and dsh[corner, c, k] += w drgb_c rgb_c (1 - rgb_c) Y_k; the fields are not read.  dsh /
 * ddensity must be zero-filled by the caller (or hold a gradient to accumulate into); float atomics: the order is not fixed. */
int ngp_voxel_trilinear_bwd(const float* xyzs, const float* dirs, const float* sigmas, const float* rgbs, const float* dsigmas /*[n]*/,
                            const float* drgbs /*[n,3]*/, int n, int grid_size, int sh_degree, float grid_min, float grid_radius,
                            float* dsh, float* ddensity, void* stream);
/* packbits (utils.py:157-169) of VoxelGrid.update_density_grid: bit = density >= threshold and density > 0, threshold =
 * min(mean of the positive cells, density_threshold), the mean summed in f64 in a fixed order.  NGP's packbits (`>` against an f32
 * mean) marks none or all cells of a fresh grid that holds one value everywhere, depending on how the mean rounds.
 * scratch: ngp_voxel_occ_scratch_doubles() doubles; n_bytes = cells / 8. */
int ngp_voxel_occ_scratch_doubles(void);
int ngp_voxel_occ_pack(const float* density_grid, long long n_bytes, double density_threshold, double* scratch, uint8_t* bitfield,
                       void* stream);

/* ---- a-5  half2 encoder fwd / explicit bwd (modules/hash_encoder_half.py:112-161,164-213) ----
 * table/out/dout/dtable are IEEE binary16 pairs (uint16_t storage). */
int ngp_hash_fwd_f16(const float* xyzs, const uint16_t* table, const ngp_hash_levels* lv, int n,
                     uint16_t* out /*[n, L, 2]*/, void* stream);
int ngp_hash_bwd_f16(const float* xyzs, const uint16_t* dout, const ngp_hash_levels* lv, int n,
                     uint16_t* dtable /*[entries,2] f16*/, void* stream);

/* Fused-path forms of the half2 encoder (same arithmetic, the buffers of the fp32 fused path): the forward widens its f16
 * result to f32 (exact) into the natural [n,32] or the pair-major layout; the backward takes the fp32 d_enc of the fused MLP
 * backward, rounds it to f16 like the reference's fp16 output gradient, merges equal-cell runs of consecutive samples before
 * the packed f16 atomic (so the f16 accumulation order differs from a serial run: tolerance-checked), and flags non-finite
 * incoming gradients.  ngp_check_finite_f16 scans the ACCUMULATED f16 gradient (n % 8 == 0) for inf / nan. */
int ngp_hash_fwd_f16_ex(const float* xyzs, const uint16_t* table, const ngp_hash_levels* lv, int n_max,
                        const int32_t* n_dev, int normalize, float lo, float hi, int enc_pairs, float* out,
                        void* stream);
int ngp_check_finite_f16(const uint16_t* g, long long n, int32_t* found_inf, void* stream);

/* ---- a-6  dir_encoder (modules/spherical_harmonics.py:7-42) + analytic backward -------------- */
int ngp_sh16_fwd(const float* dirs /*[n,3]*/, int n, float* out /*[n,16]*/, void* stream);
int ngp_sh16_bwd(const float* dirs, const float* dout /*[n,16]*/, int n, float* ddirs /*[n,3]*/,
                 void* stream);

/* ---- a-7  volume_rendering_kernel + closed-form backward (modules/volume_train.py:6-48,160) ---
 * rgbs_is_half selects fp16 (autocast) or fp32 `rgbs`; the gradient is written in the same dtype.
 * Outputs are indexed by ray_idx = rays_a[n,0] like the reference. dL_dopacity / dL_ddepth / dL_dws may
 * be NULL (== zeros); opacity/depth/rgb/ws are the forward outputs. */
int ngp_composite_train_fwd(const float* sigmas, const void* rgbs, int rgbs_is_half,
                            const float* deltas, const float* ts, const int32_t* rays_a,
                            float T_threshold, int n_rays,
                            int32_t* total_samples /*[n]*/, float* opacity, float* depth,
                            float* rgb /*[n,3]*/, float* ws /*[S]*/, void* stream);
int ngp_composite_train_bwd(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb,
                            const float* dL_dws, const float* sigmas, const void* rgbs,
                            int rgbs_is_half, const float* deltas, const float* ts,
                            const int32_t* rays_a, const float* opacity, const float* depth,
                            const float* rgb, const float* ws, float T_threshold, int n_rays,
                            float* dL_dsigmas, void* dL_drgbs, void* stream);
/* ... with the background blend of rendering.py:219-226 (results['rgb'] = rgb + rgb_bg * (1 - opacity), rgb_bg = ones behind
 * synthetic scenes) inside the two launches: _fwd_bg also writes rgb_out[n,3] = rgb + bg (1 - opacity) (nullable; `rgb` stays the
 * unblended colour the backward reads); _bwd_bg takes dL_drgb as the gradient of the BLENDED colour and adds the blend's share,
 * -bg sum_c dL_drgb, to d opacity.  bg == 0: the two entries above. */
int ngp_composite_train_fwd_bg(const float* sigmas, const void* rgbs, int rgbs_is_half, const float* deltas, const float* ts,
                               const int32_t* rays_a, float T_threshold, int n_rays, int32_t* total_samples, float* opacity,
                               float* depth, float* rgb, float* ws, float* rgb_out, float bg, void* stream);
int ngp_composite_train_bwd_bg(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb, const float* dL_dws,
                               const float* sigmas, const void* rgbs, int rgbs_is_half, const float* deltas, const float* ts,
                               const int32_t* rays_a, const float* opacity, const float* depth, const float* rgb, const float* ws,
                               float T_threshold, int n_rays, float* dL_dsigmas, void* dL_drgbs, float bg, void* stream);

/* Round 5 -- chunked forward: do not shade what compositing will never read.  The reference shades every marched sample and then
 * ignores those behind T <= T_threshold (volume_train.py:38); its evaluation loop (rendering.py:62-158) already shades in rounds
 * and drops finished rays.  One call per round: samples [begin, begin + len) of every ray still alive are appended to `list`
 * (count[0] += their number; count_zero, nullable, is set to 0 for a later round's counter).  begin > 0: the ray's transmittance
 * state T_state[row of rays_a] (n_rays floats) is first advanced over [prev_begin, begin) -- which must have been shaded -- as
 * T *= exp(-sum sigma delta), and the ray is retired when T <= thr_stop; begin == 0 initialises the state.  begin / len / prev_begin
 * must be multiples of 64 and thr_stop at most half the compositing threshold: ngp_composite_train_* read a ray 64 samples at a
 * time and skip a group when T <= threshold at its start, so every group they read has then been shaded.  Per ray rgb / opacity /
 * depth / ws / vr and every gradient are those of shading everything (tests/test_gpu_chunked.py). */
int ngp_chunk_schedule(const int32_t* rays_a, const float* sigmas, const float* deltas, int n_rays, int begin, int len,
                       int prev_begin, float thr_stop, float* T_state, int32_t* list, int32_t* count, int32_t* count_zero,
                       void* stream);
/* The list of ngp_live_compact in block-completion order (each ray's samples contiguous; the *_live kernels do not depend on the
 * order) from one launch with one atomic per 64 rays: live_total[0] must be 0 at launch, live_zero (nullable) is cleared. */
int ngp_live_list(const int32_t* rays_a, const int32_t* vr_per_ray /*[n], by ray index*/, int n_rays, int32_t* live_idx,
                  int32_t* live_total, int32_t* live_zero, void* stream);
/* The same launch, and the compacted live-sample list of ngp_live_compact as a by-product: every 16-ray block appends its rays'
 * first vr[r] samples to live_idx at an offset it takes from live_total with ONE atomic add, so the list is in block-completion
 * order (each ray contiguous) -- the *_live kernels do not depend on the order.  live_total[0] must be 0 at launch; live_zero
 * (nullable) is set to 0 by the kernel: a caller alternating two counters gets the next step's counter cleared for free.
 * live_idx == NULL: plain ngp_composite_train_fused. */
int ngp_composite_train_fused_live(const float* sigmas, const void* rgbs, int rgbs_is_half, const float* deltas,
                                   const float* ts, const int32_t* rays_a, const float* target, float bg,
                                   const float* loss_scale, float T_threshold, int n_rays, int32_t* vr_per_ray,
                                   float* opacity, float* depth, float* rgb, float* ws, float* d_sigmas, void* d_rgbs,
                                   float* sq_err, int32_t* live_idx, int32_t* live_total, int32_t* live_zero,
                                   void* stream);

/* Live-sample list for the backward pass: the first vr_per_ray[r] samples of ray r (those in front of the early-termination
 * point, volume_train.py:31-47) are the only ones with a non-zero gradient.  live_idx[j] = sample index of the j-th live
 * sample (ray order), live_total[0] = their number, live_off = [n_rays] scratch.  ngp_mlp_bwd_live / ngp_hash_bwd_*_live run
 * on that list: position j reads sample live_idx[j] (enc, dirs, gradients, xyzs) and d_enc is written / read at position j. */
int ngp_live_compact(const int32_t* rays_a, const int32_t* vr_per_ray /*[n], by ray index*/, int n_rays, int32_t* live_off,
                     int32_t* live_idx, int32_t* live_total, void* stream);
int ngp_mlp_bwd_live(const float* enc, const float* dirs, const uint16_t* wpack, const float* dsigmas, const uint16_t* drgbs,
                     int n_max, const int32_t* n_dev, const int32_t* live_idx, int enc_pairs, float* d_enc, float* dW,
                     int32_t* found_inf, void* stream);
/* The same backward with the weight gradients left as PER-BLOCK SLABS instead of float atomics on dW: block b of the launch
 * writes its sums of all 9408 weights to dW_parts[b * 9408 ...] with plain stores (256 blocks x 9408 same-address atomics were
 * 13 us of a 72 us launch).  dW_parts: ngp_mlp_dw_parts_max() * 9408 floats, no initialisation needed.  Returns the number of
 * slabs written (>= 1; 0 for n_max <= 0; < 0 on error).  ngp_mlp_dw_reduce ADDS the slabs to dW [9408] -- or the trainer's
 * ngp_train_prologue_reduce does, in the launch it needs anyway. */
int ngp_mlp_dw_parts_max(void);
int ngp_mlp_bwd_live_parts(const float* enc, const float* dirs, const uint16_t* wpack, const float* dsigmas,
                           const uint16_t* drgbs, int n_max, const int32_t* n_dev, const int32_t* live_idx, int enc_pairs,
                           float* d_enc, float* dW_parts, int32_t* found_inf, void* stream);
int ngp_mlp_dw_reduce(const float* dW_parts, int n_parts, float* dW, void* stream);
int ngp_hash_bwd_f32_live(const float* xyzs, const float* dout, const ngp_hash_levels* lv, int n_max, const int32_t* n_dev,
                          const int32_t* live_idx, int normalize, float lo, float hi, int enc_pairs, float* dtable,
                          int32_t* found_inf, void* stream);
int ngp_hash_bwd_f16_live(const float* xyzs, const float* dout, const ngp_hash_levels* lv, int n_max, const int32_t* n_dev,
                          const int32_t* live_idx, int normalize, float lo, float hi, int enc_pairs, uint16_t* dtable,
                          int32_t* found_inf, void* stream);
/* The same scatter-add (autodiff backward of modules/hash_encoder.py:89-143, call site :269; F = 2) WITHOUT global float
 * atomics: the gradient table is cut into slices of 8192 entries (128 KB of f64 pairs), each owned by one workgroup that
 * accumulates in its LDS and adds the slice to the table once (csrc/hash_bwd_lds.hip).  Same arguments and semantics as
 * ngp_hash_bwd_f32_live (dtable is accumulated into) plus a caller-owned scratch buffer of
 * ngp_hash_bwd_sliced_workspace(lv, n_max) bytes: compact positions + one hit BIT per (level, slice, sample) + the queue heads
 * of the persistent workgroups.  Returns -2 when the level table does not fit the formulation (F != 2, a level of more than
 * 64 slices = 2^19 entries, an odd level size): the caller then uses ngp_hash_bwd_f32_live.
 * The workspace belongs to ONE call sequence at a time: prep -> main of one backward must not be interleaved with another
 * backward's on another stream using the same buffer (the bitmaps and the queue heads live in it). */
long long ngp_hash_bwd_sliced_workspace(const ngp_hash_levels* lv, int n_max);
/* The two halves as separate entry points: the prepass (compact positions + hit bitmaps) needs only positions and live list, so it
 * can be issued before the MLP backward that produces `dout`; `main` consumes the workspace it filled. */
int ngp_hash_bwd_sliced_prep(const float* xyzs, const ngp_hash_levels* lv, int n_max, const int32_t* n_dev,
                             const int32_t* live_idx, int normalize, float lo, float hi, void* workspace,
                             long long workspace_bytes, void* stream);
int ngp_hash_bwd_sliced_main(const float* dout, const ngp_hash_levels* lv, int n_max, const int32_t* n_dev, int enc_pairs,
                             float* dtable, int32_t* found_inf, const void* workspace, long long workspace_bytes,
                             void* stream);
/* ngp_hash_bwd_sliced_main / _main_f16 (table_is_f16) whose first workgroups ALSO finish the MLP backward: dW[9408] += the sum of
 * the n_parts weight-gradient slabs ngp_mlp_bwd_live_parts left (= ngp_mlp_dw_reduce, without a launch of its own: in a 200 us
 * launch of persistent workgroups the ~2 us are invisible; the trainer's single-GPU step). */
int ngp_hash_bwd_sliced_main_slabs(const float* dout, const ngp_hash_levels* lv, int n_max, const int32_t* n_dev, int enc_pairs,
                                   void* dtable, int table_is_f16, int32_t* found_inf, const void* workspace,
                                   long long workspace_bytes, const float* mlp_dw_parts, int n_parts, float* mlp_dw, void* stream);
/* Round 5 -- scatter-add WITH the optimizer (replaces train.py:197-201 on the path modules/hash_encoder.py:269 feeds; one GPU).
 * The owner of a slice that is not replicated over sample ranges (every level of 64 slices = 2^19 entries: the hashed levels)
 * holds that slice's complete gradient in LDS when its task ends; instead of adding it to dtable for ngp_adam_all_ex to read
 * back, it applies the same torch.optim.Adam update (eps as given, unscale by state_f[1], skip when state_i[4]) to EVERY entry of
 * its slice of table / table_m / table_v and refreshes table_bf16 (nullable): 24 B per parameter instead of 40.  The remaining
 * (coarse, replicated) levels still accumulate into dtable; they occupy table floats [0, ngp_hash_bwd_sliced_adam_prefix(lv)),
 * and the caller runs ngp_adam_all_ex over exactly that range afterwards.  Results are bit-identical to
 * ngp_hash_bwd_sliced_main + ngp_adam_all_ex over the whole table (tests/test_gpu_flush_adam.py).
 * state_f / state_i must hold THIS step's decision already: run ngp_train_prologue before this call; the inf flag it consumes comes
 * from ngp_mlp_bwd_live[_parts], which checks the d_enc values this kernel reads (this entry point does not write found_inf).
 * mlp_dw_parts / n_parts / mlp_dw: the optional slab sum of ngp_hash_bwd_sliced_main_slabs (NULL / 0: none).
 * _adam_prefix returns -2 (and _main_adam -2) when the level table has no non-replicated levels. */
long long ngp_hash_bwd_sliced_adam_prefix(const ngp_hash_levels* lv);
/* The same launch with the step's scalar bookkeeping inside it (ngp_train_prologue's arguments; train.py:197-201): every workgroup
 * evaluates the GradScaler / schedule decision on a private copy of state_f / state_i when it starts (as the previous step left
 * them + this step's inf flag from the MLP backward), its flushes use that copy, and the last workgroup out stores it -- after the
 * launch state_f / state_i are exactly what ngp_train_prologue would have left, and no one-thread launch sits in front of the
 * scatter-add.  Bit-identical to ngp_train_prologue + ngp_hash_bwd_sliced_main_adam (tests/test_gpu_flush_adam.py). */
int ngp_hash_bwd_sliced_main_adam_step(const float* dout, const ngp_hash_levels* lv, int n_max, const int32_t* n_dev, int enc_pairs,
                                       float* dtable, const void* workspace, long long workspace_bytes, const float* mlp_dw_parts,
                                       int n_parts, float* mlp_dw, float* table, float* table_m, float* table_v, uint16_t* table_bf16,
                                       float* state_f, int32_t* state_i, float lr0, float eta_min, int t_max, float beta1, float beta2,
                                       float eps, float growth, float backoff, int growth_interval, void* stream);
/* the half2 encoder's backward (hash_encoder_half.py:163-213) over the same prepass: dtable_f16 = fp16 pairs [entries][2]; the
 * encoder's fp16 arithmetic per contribution (cell cast to f16, w * g rounded to f16), the owner's f64 sum rounded to fp16 once */
int ngp_hash_bwd_sliced_main_f16(const float* dout, const ngp_hash_levels* lv, int n_max, const int32_t* n_dev, int enc_pairs,
                                 uint16_t* dtable_f16, int32_t* found_inf, const void* workspace, long long workspace_bytes,
                                 void* stream);
int ngp_hash_bwd_f32_sliced(const float* xyzs, const float* dout, const ngp_hash_levels* lv, int n_max, const int32_t* n_dev,
                            const int32_t* live_idx, int normalize, float lo, float hi, int enc_pairs, float* dtable,
                            int32_t* found_inf, void* workspace, long long workspace_bytes, void* stream);

/* ---- a-8  composite_test (modules/volume_render_test.py:4-54) -------------------------------- */
int ngp_composite_test(const float* sigmas, const void* rgbs, int rgbs_is_half, const float* deltas,
                       const float* ts, const int64_t* pack_info /*[n,2]*/,
                       int64_t* alive_indices /*in-out*/, float T_threshold, int n_alive,
                       float* opacity, float* depth, float* rgb, void* stream);

/* ---- a-9  the two MLPs + TruncExp + direction glue, fused (modules/networks.py:18-30,111-132,136-166,293-380
 * under torch.autocast(fp16), train.py:177).  Default architecture only: xyz_encoder 32->64->16, rgb_net
 * [SH16|h16]->64->64->3, bias-free.  Weights are the fp32 master tensors in nn.Linear layout [out][in];
 * ngp_mlp_pack rounds them to fp16 and lays them out as MFMA fragments (ngp_mlp_wpack_halfs() uint16 elements).
 *   fwd : enc [n,32] f32 (hash-grid output), dirs [n,3] f32 (raw ray directions; normalisation, (d+1)/2 and SH16
 *         happen inside) -> sigmas [n] f32, rgbs [n,3] f16.  dirs == NULL or rgbs == NULL: density only.
 *   bwd : recomputes the forward, consumes dL/dsigmas [n] f32 and dL/drgbs [n,3] f16, writes dL/denc [n,32] f32 and
 *         ACCUMULATES the weight gradients into dW [9408] f32 = W1|W2|W3|W4|W5 row-major (caller zero-fills). */
int ngp_mlp_wpack_halfs(void);
int ngp_mlp_pack(const float* W1, const float* W2, const float* W3, const float* W4, const float* W5,
                 int enc_pairs, uint16_t* wpack, void* stream);      /* enc_pairs: which enc layout the image is for */
int ngp_mlp_fwd(const float* enc, const float* dirs, const uint16_t* wpack, int n, float* sigmas,
                uint16_t* rgbs, void* stream);
int ngp_mlp_bwd(const float* enc, const float* dirs, const uint16_t* wpack, const float* dsigmas,
                const uint16_t* drgbs, int n, float* d_enc, float* dW, void* stream);

int ngp_mlp_fwd_ex(const float* enc, const float* dirs, const uint16_t* wpack, int n_max, const int32_t* n_dev,
                   int enc_pairs, float* sigmas, uint16_t* rgbs, void* stream);
/* Round 5 -- the forward over a LIST of samples: position j < *n_list shades sample list[j] (reads its enc row and direction, writes
 * its sigma / rgb; networks.py:136-166).  Bit-identical per sample to ngp_mlp_fwd_ex. */
int ngp_mlp_fwd_list(const float* enc, const float* dirs, const uint16_t* wpack, int n_max, const int32_t* n_list,
                     const int32_t* list, int enc_pairs, float* sigmas, uint16_t* rgbs, void* stream);

/* Stream plumbing for a caller that runs the march of the NEXT batch on a second stream (FusedTrainer): events that order two
 * streams of THIS device without the system-scope cache write-back + invalidate a default HIP event performs when it is recorded
 * (hipEventDisableTiming | hipEventDisableSystemFence).  Not for host-visible results. */
int ngp_event_create(void** event);
int ngp_event_record(void* event, void* stream);
int ngp_stream_wait_event(void* stream, void* event);
int ngp_event_destroy(void* event);
/* ... and the host-side wait for one (round 6): returns when the work recorded in front of the event has completed.  FusedTrainer can wait
 * this way (NGP_EXPERIMENT prefetch_host_wait=1) for a prefetched march that was issued a whole step earlier: a stream-side wait for an
 * event of another queue costs the waiting stream ~10 us even when the event completed long ago. */
int ngp_event_synchronize(void* event);
/* A non-blocking stream of the lowest priority the device offers (for the prefetched march: it should take only the CUs the step's
 * own kernels leave free); *least / *greatest (nullable) = hipDeviceGetStreamPriorityRange. */
int ngp_stream_create_low_priority(void** stream, int* least, int* greatest);
int ngp_stream_destroy(void* stream);
/* Pinned host memory + an asynchronous device-to-host copy on a stream of the caller's choice: a word the device reports into
 * without anybody waiting for it (FusedTrainer: the sample count of each prefetched march, read by later steps to place the next
 * one).  The caller frees the memory after synchronising the streams it copied on. */
int ngp_host_alloc(void** host, long long bytes);
int ngp_host_free(void* host);
int ngp_copy_to_host_async(void* host, const void* dev, long long bytes, void* stream);

/* ---- the fused training render as ONE entry per direction (round 5; replaces the launch sequence of reference
 * modules/rendering.py:161-228 + modules/networks.py:152-166 and their autograd backward for one batch of rays).  The caller keeps
 * one argument block per sample arena and patches the per-call pointers; every buffer is caller-owned device memory.
 * _fwd: [coarse occupancy table when rebuild_coarse] -> ngp_march_train_fused -> ngp_hash_fwd_{f32,bf16,f16}_ex -> ngp_mlp_pack ->
 *       ngp_mlp_fwd_ex -> ngp_composite_train_fwd.
 * _bwd: ngp_composite_train_bwd -> ngp_live_compact -> ngp_mlp_bwd_live -> ngp_hash_bwd_f32_sliced into dW / dtable, which the caller
 *       hands over CLEARED (or the
 *       float-atomic kernel when the level table does not fit it / force_atomic; table_kind 2: the half2 encoder's fp16 forms).
 * Same kernels, same results as the individual entry points in that order (tests/test_gpu_fused.py). */
typedef struct ngp_render_args {
    const float* rays_o; const float* rays_d; const float* hits_t /*nullable: slab test inline*/; const float* noise /*[n_rays] jitter*/;
    int32_t n_rays, max_samples;
    const uint8_t* bitfield; uint32_t* coarse; int32_t rebuild_coarse, cascades, grid_size;
    float scale, exp_step_factor, T_threshold;
    const void* table; int32_t table_kind /*0 fp32, 1 bf16 copy, 2 f16 copy (half2 encoder)*/, enc_pairs;
    const ngp_hash_levels* levels; float lo, hi;
    const float* w[5]; uint16_t* wpack;
    long long cap;                                   /* rows of the per-sample buffers below (n_rays * max_samples) */
    float* stage; int32_t* march_ctr; float* xyzs; float* dirs; float* deltas; float* ts; float* enc; float* sigmas; uint16_t* rgbs; float* ws;
    int32_t* rays_a; int32_t* total; int32_t* vr_per_ray; float* opacity; float* depth; float* rgb;          /* per-ray outputs */
    const float* g_opacity; const float* g_depth; const float* g_rgb; const float* g_ws;                    /* backward: nullable but g_rgb */
    float* d_sigmas; uint16_t* d_rgbs; float* d_enc; int32_t* live_off; int32_t* live_idx; int32_t* live_total;
    void* workspace; long long workspace_bytes;      /* ngp_hash_bwd_sliced_workspace(levels, cap) bytes */
    int32_t force_atomic, reserved;
    /* round 6 (both nullable: NULL = round 5's launches).  dW_parts: ngp_mlp_dw_parts_max() * 9408 floats -- the MLP backward leaves its
     * weight gradients as per-block slabs and the head of the scatter-add launch adds them to dW (ngp_hash_bwd_sliced_main_slabs) instead of
     * 256 x 9408 same-address float atomics.  live_zero: a second counter that is 0 at launch; the live list is then built by ngp_live_list
     * (one atomic per 64 rays, block-completion order) into live_total -- WHICH MUST BE 0 AT LAUNCH -- and live_zero is what the launch clears
     * for the next call (a caller alternating the two never clears one itself). */
    float* dW_parts; int32_t* live_zero;
    float* dW /*[9408], cleared by the caller*/; void* dtable /*f32 [entries * 2]; table_kind 2: f16; cleared by the caller*/; long long dtable_bytes;
    /* ABI 3.  bg: the background the composited colour is blended over (rendering.py:219-226: 1 behind synthetic scenes, 0 behind real
     * ones).  rgb_out (nullable, [n_rays,3]): _fwd also writes rgb + bg (1 - opacity) there -- what the loss sees; `rgb` stays the
     * unblended colour the backward reads.  _bwd takes g_rgb as the gradient of the BLENDED colour when bg != 0 (adds -bg sum_c g_rgb to
     * d opacity).  clear_grads != 0: _bwd clears dW and dtable itself (one fill launch behind the compositing backward; dtable_bytes % 16
     * == 0) instead of expecting them cleared. */
    float bg; int32_t clear_grads; float* rgb_out;
} ngp_render_args;
int ngp_render_train_fwd(const ngp_render_args* args, void* stream);
int ngp_render_train_bwd(const ngp_render_args* args, void* stream);

/* ---- f-2  device-resident optimisation-step epilogue (reference train.py:193-201: mse_loss, GradScaler,
 * Adam(eps=1e-15), CosineAnnealingLR, zero_grad) -- see csrc/optim.hip.
 * state_f[8] f32: [0] loss scale, [1] 1/scale of this step, [2] lr, [3] 1-beta1^t, [4] sqrt(1-beta2^t), [5] last loss
 * state_i[8] i32: [0] iteration, [1] optimizer steps taken, [2] growth tracker, [3] found_inf (set by the backward
 *                 kernels, consumed + cleared by the prologue), [4] skip flag of this step, [5] skipped steps so far */
int ngp_mse_loss_grad(const float* rgb, const float* opacity, const float* target, float bg, int n_rays,
                      float* state_f, float* g_rgb, float* g_opacity, void* stream);
/* ... per ray, from as many blocks as the batch needs: the same g_rgb / g_opacity (loss-scaled by state_f[0]) and, instead of the
 * reduced loss, the per-ray squared error sq_err[r] (nullable) for whoever logs it (train.py:193). */
int ngp_mse_loss_grad_rays(const float* rgb, const float* opacity, const float* target, float bg, int n_rays,
                           const float* state_f, float* g_rgb, float* g_opacity, float* sq_err, void* stream);
int ngp_train_prologue(float* state_f, int32_t* state_i, float lr0, float eta_min, int t_max, float beta1,
                       float beta2, float growth, float backoff, int growth_interval, void* stream);
/* The prologue and, in the same launch, ngp_mlp_dw_reduce(dW_parts, n_parts, dW). */
int ngp_train_prologue_reduce(float* state_f, int32_t* state_i, float lr0, float eta_min, int t_max, float beta1,
                              float beta2, float growth, float backoff, int growth_interval, const float* dW_parts,
                              int n_parts, float* dW, void* stream);
/* Prologue for an optimizer driven by torch.cuda.amp.GradScaler (train.py:143-149,198-201 with apex.optimizers.FusedAdam =
 * compat/apex): grad_scale / found_inf are the scaler's device tensors (NULL: scale 1 / never skip), lr the host-side scheduler's
 * value; fills state_f[1..4] and state_i[1,4] for ngp_adam_step; the bias-correction step count advances on non-skipped steps. */
int ngp_adam_amp_prologue(float* state_f, int32_t* state_i, const float* grad_scale, const float* found_inf, float lr,
                          float beta1, float beta2, void* stream);
/* p, g, m, v: n floats each (n % 4 == 0, 16-byte aligned); g is unscaled on the fly and zero-filled. */
/* The same pass over up to NGP_ADAM_MULTI_MAX tensors in ONE launch (host arrays of device pointers and element counts, read at
 * call time): what an optimizer over model.parameters() -- the table and the five weight matrices, train.py:143-149 -- needs per
 * step instead of one launch per tensor. */
#define NGP_ADAM_MULTI_MAX 16
int ngp_adam_multi(int n_tensors, float* const* p, float* const* g, float* const* m, float* const* v, const long long* n,
                   const float* state_f, const int32_t* state_i, float beta1, float beta2, float eps, void* stream);
/* GradScaler's inf / nan check (train.py:199, torch.amp.GradScaler._check_inf_per_device) over the same tensor list, read-only:
 * found_inf[0] (a float32 device scalar, cleared by the caller) becomes 1.0f when any gradient value is not finite. */
int ngp_check_finite_multi(int n_tensors, const float* const* g, const long long* n, float* found_inf, void* stream);
/* ... and ngp_adam_amp_prologue in the same launch (one parameter group of <= NGP_ADAM_MULTI_MAX tensors): the last block out runs the
 * prologue on the finished flag.  found_inf must be 0 at launch; clear_next (nullable) is a second flag this launch clears for the
 * caller's NEXT step -- GradScaler.update() (train.py:200) reads found_inf after step() returns, so a caller alternating two flags never
 * issues a fill.  done: 17 x 32 uint32 of device memory (arrival counters 128 bytes apart), 0 between launches. */
int ngp_adam_amp_check_prologue(int n_tensors, const float* const* g, const long long* n, float* found_inf, float* clear_next,
                                uint32_t* done, float* state_f, int32_t* state_i, const float* grad_scale, float lr, float beta1,
                                float beta2, void* stream);
/* dst[i] = bf16(src[i]), round-to-nearest-even; n % 4 == 0 (the per-forward cast of hash_encoder_half.py:367, in bf16). */
int ngp_cast_f32_bf16(const float* src, uint16_t* dst, long long n, void* stream);
/* General form: table_g is fp32 or (grad_is_f16) the half2 encoder's f16 gradient buffer, widened to fp32 on the fly;
 * copy_kind 0 = no storage copy, 1 = bf16, 2 = f16 (the table the f16 forward gathers from, hash_encoder_half.py:367). */
int ngp_adam_all_ex(float* table, void* table_g, int grad_is_f16, float* table_m, float* table_v, long long n,
                    uint16_t* table_16, int copy_kind, float* mlp, float* mlp_g, float* mlp_m, float* mlp_v,
                    const float* state_f, const int32_t* state_i, float beta1, float beta2, float eps, int enc_pairs,
                    uint16_t* wpack, void* stream);
/* Adam on the 9 408 flat MLP weights (W1|W2|W3|W4|W5) + the fp16 fragment repack for the next step, one launch. */
int ngp_adam_mlp_pack(float* p, float* g, float* m, float* v, const float* state_f, const int32_t* state_i,
                      float beta1, float beta2, float eps, int enc_pairs, uint16_t* wpack, void* stream);

/* ---- a-10 morton3D / morton3D_invert / packbits (modules/utils.py:120-169) -------------------- */
int ngp_morton3d(const int32_t* coords /*[m,3]*/, int m, int32_t* indices, void* stream);
int ngp_morton3d_invert(const int32_t* indices, int m, int32_t* coords /*[m,3]*/, void* stream);
int ngp_packbits(const float* density_grid /*[8k]*/, float threshold, int n_bytes,
                 uint8_t* bitfield, void* stream);

/* ---- f-1  distortion loss (modules/distortion.py:15-119): per-ray loss[N] (indexed by ray_idx) and the inclusive
 * scans the backward needs; backward writes dL/dws for the live samples addressed by rays_a. */
int ngp_distortion_fwd(const float* ws, const float* deltas, const float* ts, const int32_t* rays_a, int n_rays,
                       float* loss, float* ws_inc, float* wts_inc, void* stream);
int ngp_distortion_bwd(const float* dL_dloss, const float* ws, const float* deltas, const float* ts,
                       const float* ws_inc, const float* wts_inc, const int32_t* rays_a, int n_rays,
                       float* dL_dws, void* stream);

/* ---- f-4  camera rays and training-batch sampling (datasets/ray_utils.py:51-80, datasets/base.py:34-61, train.py:171-184)
 * get_rays:    rays_d[k,i] = sum_j directions[k,j] * c2w[i,j], rays_o[k] = c2w[:,3]; poses = [n,3,4] (per_ray_pose = 1, the
 *              training batch) or one [3,4] pose for all rays (per_ray_pose = 0, an evaluation image).
 * sample_rays: for sample k: image i = img_idx[k] (img0 when img_idx is NULL = 'same_image' sampling), pixel p = pix_idx[k];
 *              pose = poses[i], direction = directions[p], rgb[k] = rays[i, p, 0:3] (rays = [n_img, hw, ray_c] f32, rgb nullable). */
int ngp_get_rays(const float* directions /*[n,3]*/, const float* poses, int per_ray_pose, int n, float* rays_o,
                 float* rays_d, void* stream);
/* up to three n-float copies in one launch (src NULL = slot unused): stages a batch into the static buffers of a captured step */
int ngp_stage_batch(const float* a, float* da, const float* b, float* db, const float* c, float* dc, int n, void* stream);
int ngp_sample_rays(const float* poses /*[n_img,3,4]*/, const float* directions /*[hw,3]*/, const float* rays, int ray_c,
                    long long hw, const int64_t* img_idx, long long img0, const int64_t* pix_idx, int n, float* rays_o,
                    float* rays_d, float* rgb, void* stream);

/* ---- f-5  ray and camera-pose gradients (pose refinement; csrc/ray_grad.hip).  First order; sums in a fixed
 * order without float atomics: two launches give the same bytes, and a NaN stays inside its ray / image.
 * march_train_bwd: adjoint of the sample write of ngp_march_train_write / ngp_march_train_fused (xyzs = o + t d, dirs = d), t held
 *   constant.  Row m of rays_a is (ray_idx, start, N): d_rays_o[ray_idx] = sum_{j<N} d_xyzs[start+j],
 *   d_rays_d[ray_idx] = sum_{j<N} ((ts[start+j] * d_xyzs[start+j]) + d_dirs[start+j]).  A NULL d_xyzs / d_dirs counts as zeros; N == 0
 *   writes zeros; every output row named by a rays_a row is written, never accumulated (rows with ray_idx outside [0, n_rays) are
 *   skipped).  Stated on rays_a rows: holds for the ray-ordered and the block-completion-ordered packing alike.
 * sample_rays_bwd: adjoint of ngp_sample_rays / the one-pose form of ngp_get_rays, per image: d_poses[i][r][c] = sum_{k: img(k)=i}
 *   d_rays_d[k][r] directions[pix(k)][c] (c < 3), d_poses[i][r][3] = sum_{k: img(k)=i} d_rays_o[k][r]; img(k) = img_idx[k] (img0 when
 *   NULL), pix(k) = pix_idx[k] (k when NULL).  All 12 n_img entries are written (an image without rays: zeros); a ray whose image lies
 *   outside [0, n_img) is skipped.  A NULL d_rays_o / d_rays_d counts as zeros.  n == 0 is valid (all zeros).
 * get_rays_bwd: the per-ray-pose form of ngp_get_rays (poses [n,3,4]): the outer product per ray, d_rays_o into column 3. */
int ngp_march_train_bwd(const float* d_xyzs /*[S,3] | NULL*/, const float* d_dirs /*[S,3] | NULL*/, const float* ts /*[S]*/,
                        const int32_t* rays_a /*[n,3]*/, int n_rays, float* d_rays_o /*[n,3]*/, float* d_rays_d /*[n,3]*/, void* stream);
int ngp_sample_rays_bwd(const float* directions /*[hw,3]*/, const int64_t* img_idx /*[n] | NULL -> img0*/, long long img0,
                        const int64_t* pix_idx /*[n] | NULL -> k*/, const float* d_rays_o /*[n,3] | NULL*/, const float* d_rays_d /*[n,3] | NULL*/,
                        int n, int n_img, float* d_poses /*[n_img,3,4]*/, void* stream);
int ngp_get_rays_bwd(const float* directions /*[n,3]*/, const float* d_rays_o, const float* d_rays_d, int n, float* d_poses /*[n,3,4]*/, void* stream);

/* ---- f-3  occupancy-grid update without host round trips (modules/networks.py:181-209,255-290).
 * compact : list[0..count) = cells of ONE cascade with density > threshold, in cell order (deterministic); count is written
 * sample  : m uniform cells (u_cell [m] in [0,1) -> Morton code) + m picks from the list (u_pick [m]) -> Morton indices [2m] and jittered
 *           world positions [2m,3] (u_jit [2m,3]); s = min(2^(c-1), scale), half_grid = s / grid_size
 * all_cells: warm-up variant, cell i = Morton code i
 * scatter : tmp[indices[i]] = sigmas[i] (indices == NULL: identity); a cell drawn twice keeps whichever write lands last, like the
 *           reference's fresh[c, indices] = density.  scatter_max: the largest of them wins (the same one on every run; sigmas > 0)
 * merge   : grid = grid < 0 ? grid : max(grid*decay, tmp); the sum and count of the positive cells leave as per-block partials in
 *           stats[2..] (stats: ngp_occ_stats_floats() floats, no initialisation needed; round 5: no float atomics -- the mean is the
 *           occupancy threshold and must not depend on the order blocks finish in)
 * pack    : every block adds the partials up in one fixed order (stats[0] = sum, stats[1] = count are written for the caller);
 *           bitfield bit = grid > min(stats[0]/stats[1], density_threshold).  n_bytes must be the merge's n / 8. */
int ngp_occ_compact(const float* density_grid, float threshold, int n_cells, int32_t* list, int32_t* count,
                    int32_t* scratch /*[1024]*/, void* stream);
/* m ascending U(0,1) values per set without sorting (normalised partial sums of m + 1 unit exponentials: the order statistics
 * of m iid uniforms, exact in distribution); u: sets * rows * 1024 uniforms (rows = (m + 1 + 1023) / 1024), work: sets * (rows *
 * 1024 + rows) floats, out: [sets][m].  Feeds ngp_occ_sample: ascending uniforms -> ascending cells -> coherent encoder queries. */
int ngp_sorted_uniforms(const float* u, int m, int sets, float* work, float* out, void* stream);
int ngp_occ_sample(const float* u_cell, const float* u_pick, const float* u_jit, const int32_t* list, const int32_t* count,
                   int m, int grid_size, float s, float half_grid, int32_t* indices, float* xyzs, void* stream);
int ngp_occ_all_cells(const float* u_jit, int n_cells, int grid_size, float s, float half_grid, float* xyzs, void* stream);
int ngp_occ_scatter(const int32_t* indices, const float* sigmas, int n, float* tmp, void* stream);
int ngp_occ_scatter_max(const int32_t* indices, const float* sigmas, int n, float* tmp, void* stream);
int ngp_occ_stats_floats(void);
int ngp_occ_merge(float* density_grid, const float* tmp, float decay, int n, float* stats, void* stream);
int ngp_occ_pack(const float* density_grid, float* stats, float density_threshold, int n_bytes, uint8_t* bitfield,
                 void* stream);

/* ---- deployment model (train.py --deployment; csrc/deploy.hip) --------------------------------------------------------------------
 * Shading of the exported 4-level, 4-feature dense grid with 16-wide MLPs, all fp32, one launch: xyzs [n,3] world positions in
 * [-0.5, 0.5] (x01 = xyz + 0.5), dirs [n,3] of any length.  table: the fp32 hash table [total_entries, 4], 16-byte aligned; lv: the
 * level table of ngp_hash_levels_init(2^21, 4, 32, 128, 4) (4 levels, 4 features, every level dense: anything else is -1).
 * sigma_w [512] = W1 [16][16] | W2 [16][16], rgb_w [768] = W3 [16][32] | W4 [16][16] whose first 3 rows are the colour rows, both
 * row-major [out][in] as save_deployment_model writes them.  sigma = exp(W2 relu(W1 enc))[0], rgb = sigmoid(W4 relu(W3 [SH16 | 16])).
 * The dense index is taken modulo the level's entry count like the training encoder, so no position reads out of bounds.
 * enc_out (nullable, [n,16], 16-byte aligned): the embedding, bit-identical to ngp_hash_fwd_f32 on x01 (tests only). */
int ngp_deploy_shade(const float* xyzs, const float* dirs, const float* table, const ngp_hash_levels* lv, const float* sigma_w,
                     const float* rgb_w, int n, float* sigmas /*[n]*/, float* rgbs /*[n,3]*/, float* enc_out, void* stream);

/* A whole image of the deployment model in ONE launch: per ray the slab test of ngp_ray_aabb (scale 0.5, near plane 0.01), the sample
 * sequence of ngp_march_train with zero noise on one 128^3 cascade at exp_step_factor 0 (at most max_samples samples), the shading of
 * ngp_deploy_shade at xyz = o + t d, and the serial front-to-back composite of ngp_composite_train_fwd over black: before each sample
 * stop unless T > T_threshold; a = 1 - exp(-sigma dt), w = a T, rgb += w c, depth += w t, opacity += w, T *= 1 - a.  The march of a
 * ray ends with its composite: nothing behind the termination point is marched or shaded.  rays_o, rays_d: [n_rays,3] (ngp_get_rays);
 * density_bitfield: the 262 144 bytes of the cascade; coarse (nullable): ngp_bitfield_coarsen of it, 128 words, built once per model;
 * table, lv, sigma_w, rgb_w: as for ngp_deploy_shade.  Outputs, every ray written (a miss: zeros): rgb [n_rays,3], opacity, depth
 * [n_rays], n_samples [n_rays] int32 = composited samples, t_last [n_rays] = t of the last composited sample (0 if none).  Every output
 * is a function of its ray alone (no atomics, no dependence on launch geometry or ray order); no per-sample data is written, nothing
 * is allocated or read back.  A ray with an all-zero direction is a miss.  -1 without a launch: a null pointer other than coarse, a
 * level table that is not ngp_deploy_shade's, a table not 16-byte aligned, max_samples < 1. */
int ngp_deploy_render(const float* rays_o, const float* rays_d, const uint8_t* density_bitfield, const uint32_t* coarse /* may be NULL */,
                      const float* table, const ngp_hash_levels* lv, const float* sigma_w, const float* rgb_w, int n_rays,
                      int max_samples, float T_threshold, float* rgb, float* opacity, float* depth, int32_t* n_samples, float* t_last,
                      void* stream);

/* ---- isosurface extraction: marching tetrahedra on a sampled scalar field (csrc/mesh.hip; contract: DESIGN.md section 3) ----------
 * values: f32 [nx, ny, nz], z fastest, every n >= 2, nx ny nz < 2^31; grid point (i, j, k) sits at lo + (i, j, k) h.  A point is inside
 * iff sign v > sign iso in f32 (sign +1: a density, -1: a signed distance; NaN and v == iso are outside).  Each cell is split into the six
 * Kuhn tetrahedra; a vertex lies on each lattice edge p -> p + d, d in {0,1}^3 \ {0}, whose ends differ, at t = (iso - v_p) / (v_q - v_p)
 * (0.5 where that is not in [0, 1]), position lo + (float(i) + t d) h per axis.  Vertices are ordered by owner p, then by edge type
 * 4 dx + 2 dy + dz; faces by cell, tetrahedron (axis permutations, lexicographic) and the listed order, counter-clockwise seen from the
 * outside.  No atomics: the same input gives the same bytes.
 * workspace_bytes: the size of `workspace` for this grid (about 4 bytes per point), -1 for a grid the other two refuse
 * count : fills the workspace and writes counts[2] = {vertices, faces} on the device ({-1, -1} if either passes 2^31 - 1)
 * emit  : after count on the same values, iso, sign and workspace: vertices f32 [V,3], faces int32 [T,3] and, unless NULL, normals f32
 *         [V,3]: the central-difference gradient of the grid (one-sided on the boundary faces), interpolated along the edge with the same
 *         t, times -sign, normalised; (0, 0, 0) where it is zero or not finite.  lo, h: three HOST floats each, h > 0.
 * Both return -1 without a launch for a null required pointer, an n < 2, a sign other than +1 / -1, nx ny nz >= 2^31 or an h <= 0. */
long long ngp_mesh_workspace_bytes(int nx, int ny, int nz);
int ngp_mesh_count(const float* values, int nx, int ny, int nz, float iso, int sign, void* workspace, int32_t* counts /*[2]*/,
                   void* stream);
int ngp_mesh_emit(const float* values, int nx, int ny, int nz, float iso, int sign, const float* lo /*[3], host*/,
                  const float* h /*[3], host*/, const void* workspace, float* vertices, float* normals /* may be NULL */, int32_t* faces,
                  void* stream);

/* ---- distance to a triangle mesh: a bounding-volume hierarchy and a nearest-face query (csrc/mesh_sdf.hip) ----
 * vertices f32 [V,3], faces int32 [*,3] (indices trusted: the caller checks their range), order int32 [n_faces]: the faces the tree
 * holds, in the order it holds them (any permutation of a subset of the rows of `faces`; the package sorts by the Morton code of the
 * centroid).  Leaf k = sorted positions [k leaf_size, (k + 1) leaf_size), padded to P = a power of two leaves; node i of the implicit
 * complete binary tree has the children 2 i + 1 and 2 i + 2, leaf k is node P - 1 + k.  boxes: f32 [2 P - 1, 6] = (lo xyz, hi xyz),
 * every leaf box widened outwards by 2^-18 of its longest side and one ulp; a node without faces has lo = +inf, hi = -inf.
 * bvh_bytes : the size of `boxes`; -1 for n_faces < 1, n_faces >= 2^31, a leaf_size outside 1..NGP_MESH_SDF_MAX_LEAF or more than
 *             2^24 leaves (the walk keeps one bit per level)
 * bvh_build : fills boxes, one launch per level, no atomics: the same mesh and order give the same bytes
 * sdf_query : one launch, one lane per point.  Per point the face that minimises the squared distance in f32 (closest point by the
 *             Voronoi regions of Ericson 5.1.5, the formula in csrc/mesh_sdf.hip; a face whose distance is NaN never wins), written as
 *             sdf [n] = s sqrt(dist2), closest [n,3], face [n] (a row of `faces`, i.e. the caller's numbering), feature [n]: 0 interior,
 *             1 / 2 / 3 edge ab / bc / ca, 4 / 5 / 6 vertex a / b / c.  closest, face, feature may be NULL.  edge_normals f32 [*,3,3]
 *             (per row of `faces`, per edge) and vertex_normals f32 [V,3]: the pseudonormals; s = +1 if n . (x - closest) >= 0 else -1
 *             with n = cross(b - a, c - a), the edge's or the vertex's by the feature.  Both NULL: unsigned, s = +1.  A result depends
 *             on its point and the mesh alone.  If no face has a distance (all NaN): sdf +inf, closest = the point, face -1.
 * All return -1 without a launch for a null required pointer, a size bvh_bytes refuses, n < 0 or exactly one of the two normal
 * arrays; sdf_query returns 0 without a launch for n = 0 (points and sdf may then be null: an empty tensor has no address). */
#define NGP_MESH_SDF_MAX_LEAF 8
long long ngp_mesh_bvh_bytes(long long n_faces, int leaf_size);
int ngp_mesh_bvh_build(const float* vertices, const int32_t* faces, const int32_t* order, int n_faces, int leaf_size, float* boxes,
                       void* stream);
int ngp_mesh_sdf_query(const float* points, int n, const float* vertices, const int32_t* faces, const int32_t* order, const float* boxes,
                       int n_faces, int leaf_size, const float* edge_normals /* may be NULL */, const float* vertex_normals /* may be NULL */,
                       float* sdf, float* closest /* may be NULL */, int32_t* face /* may be NULL */, int32_t* feature /* may be NULL */,
                       void* stream);

/* ---- ray casting against a triangle mesh: the first face along a ray, in the same hierarchy (csrc/mesh_raycast.hip)
 * vertices, faces, order, boxes, n_faces, leaf_size: the tree ngp_mesh_bvh_build made, read only.  rays_o, rays_d f32 [n,3]; directions
 * need not be normalised.  One launch, one lane per ray.  Per ray the face that minimises t in [t_min, t_max] by the watertight test of
 * Woop, Benthin & Wald 2013 in f32 (the formula in csrc/mesh_raycast.hip): no ray slips between two faces that share an edge or a vertex.
 * t [n]    : the ray parameter in units of |d| (the hit point is o + t d); +inf on a miss
 * face [n] : a row of `faces` (the caller's numbering); -1 on a miss
 * bary [n,2] : (v, w), the hit point is a + v (b - a) + w (c - a), the convention of sdf_query's closest point; 0 on a miss
 * side [n] : +1 the front of the face was hit (d . cross(b - a, c - a) < 0, by the sign of the determinant), -1 the back, 0 a miss
 * face, bary, side may be NULL; t has the same bits with or without them.  flags: NGP_RAYCAST_ANY_HIT stops at the first accepted face (the
 * occlusion query: t and face are then those of AN accepted face), NGP_RAYCAST_CULL_BACK / NGP_RAYCAST_CULL_FRONT skip back- / front-
 * facing faces.  A face without area is never hit.  A ray with a zero or non-finite direction, a NaN anywhere, or t_min <= t_max false
 * is a miss; the walk ends after a bounded number of steps for any bit pattern.  A result depends on its ray and the mesh alone.
 * Returns -1 without a launch for a null required pointer, a size bvh_bytes refuses, n < 0 or unknown flag bits; 0 without a launch for
 * n = 0 (rays_o, rays_d and t may then be null). */
#define NGP_RAYCAST_ANY_HIT 1
#define NGP_RAYCAST_CULL_BACK 2
#define NGP_RAYCAST_CULL_FRONT 4
int ngp_mesh_raycast(const float* rays_o, const float* rays_d, int n,
                     const float* vertices, const int32_t* faces, const int32_t* order, const float* boxes,
                     int n_faces, int leaf_size, float t_min, float t_max, int flags,
                     float* t /*[n]*/, int32_t* face /*[n], may be NULL*/, float* bary /*[n,2], may be NULL*/,
                     int32_t* side /*[n], may be NULL*/, void* stream);

/* ---- winding number of a triangle mesh: inside / outside for open, overlapping and unwelded meshes (csrc/mesh_winding.hip; DESIGN.md
 * section 3).  vertices, faces, order, boxes, n_faces, leaf_size: the tree ngp_mesh_bvh_build made, read only.
 * w(q) = (1 / 4 pi) sum_f Omega_f(q), Omega_f = 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) with a, b, c the corners
 * minus q, in f32 (the formula in csrc/mesh_winding.hip), and 0 where a . (b x c) == 0.  With cross(b - a, c - a) pointing outward a
 * closed mesh gives +1 inside and 0 outside; a point on a vertex and a face without area add 0.
 * moments: f32 [2 P - 1, 20], 16-byte aligned, one row per node of the tree:
 *     0..2 p (the area-weighted centroid of the faces below; the box centre where their area sums to 0)
 *     3 r (the distance from p to the farthest corner of the node's box, rounded upwards; -1: an empty node)
 *     4..6 N = sum 0.5 cross(b - a, c - a)    7 A = sum of the areas    8..16 T = sum (centroid_f - p) (x) (area vector)_f, row major
 *     17 1 for a node with faces, 0 for an empty one    18, 19 0
 * winding_bytes : the size of `moments`; -1 wherever ngp_mesh_bvh_bytes refuses
 * winding_build : fills moments from the tree, one launch per level, no atomics: the same mesh and order give the same bytes
 * winding_query : one launch, one lane per point, a preorder walk.  A node with d = p - q is accepted iff d.d > (beta r)^2 and then adds
 *                 N.d / |d|^3 (order_terms >= 1) + trace(T) / |d|^3 - 3 d.T d / |d|^5 (order_terms 2) in place of its faces; a leaf that
 *                 is not accepted adds Omega of each of its faces.  beta = +inf accepts nothing: the exact sum.  The sum is f32 in walk
 *                 order: winding [n] depends on its point and the tree alone.  A point with a coordinate that is not finite gets NaN.
 * All return -1 without a launch for a null required pointer, a size bvh_bytes refuses or n < 0; winding_query also for a beta below 1
 * or NaN and an order_terms other than 1 or 2, and it returns 0 without a launch for n = 0 (points and winding may then be null). */
long long ngp_mesh_winding_bytes(long long n_faces, int leaf_size);
int ngp_mesh_winding_build(const float* vertices, const int32_t* faces, const int32_t* order, const float* boxes, int n_faces,
                           int leaf_size, float* moments, void* stream);
int ngp_mesh_winding_query(const float* points, int n, const float* vertices, const int32_t* faces, const int32_t* order,
                           const float* moments, int n_faces, int leaf_size, float beta, int order_terms /* 1 or 2 */,
                           float* winding /*[n]*/, void* stream);

/* ---- connected components of a triangle mesh: labels, a per-component table, sub-mesh selection (csrc/mesh_components.hip; DESIGN.md
 * section 3).  faces int32 [T,3], n_vertices V, 1 <= T, V <= 2^31 - 1 (the package answers T = 0 and V = 0 without a call).  Two
 * vertices are connected when some face names both.  A face with an index outside [0, V) is bad: it joins nothing and gets face
 * component -1; a face that repeats an index still joins its vertices.  A vertex named by no good face is unused: component -1.
 * Components are numbered 0 .. C - 1 by increasing smallest vertex index.
 * components_bytes : the size of `workspace` for label and select_count (about max(T, V) + 4 V bytes)
 * components_rounds: n_rounds rounds of the min-index union-find on parent int32 [V] (parent[x] <= x; the caller starts it at
 *                    parent[x] = x): a hook pass over the faces, then a compress pass over the vertices.  changed int32 [n_rounds],
 *                    zeroed by the caller: changed[r] = 1 iff hook pass r moved something; passes behind the first that did not
 *                    return at once.  The labelling is complete after a pass with changed[r] = 0; at most V passes are needed.
 * components_label : after such a pass: vertex_component int32 [V], face_component int32 [T], counts int32 [3] = {C, bad faces,
 *                    unused vertices}, on the device
 * components_edge_keys : keys int64 [3 T]: min V + max per edge of every good face with three distinct indices, INT64_MAX otherwise
 * components_table : sorted_keys = those keys in ascending order.  table int32 [C,6] = vertices, faces, edges (distinct keys),
 *                    boundary edges (keys used once), non-manifold edges (keys used three or more times), euler = vertices - edges
 *                    + faces.  An edge belongs to the component of its ends.  Integer atomics only.
 * components_measure : order int64 [T] = the faces sorted by (face component, index), bad faces first; face_start int32 [C + 1]: where
 *                    component c starts in `order`; block_start int32 [C + 1]: the exclusive prefix sums of ceil(faces_c / 64);
 *                    partials: partial_bytes(T, C) bytes of scratch, 8-byte aligned.  area f64 [C] = sum of 0.5 |(b - a) x (c - a)|,
 *                    volume f64 [C] = sum of a . (b x c) / 6, terms in f64 from the f32 coordinates, summed in an order the input
 *                    fixes (no float atomics: the same input gives the same bytes); lo, hi f32 [C,3] the exact box (-0 below +0).
 * select_count     : keep uint8 [C].  vertex_map int32 [V], face_map int32 [T]: the index a kept vertex / face gets, -1 for the
 *                    others (bad faces and unused vertices included); counts int32 [2] = {vertices kept, faces kept}, on the device
 * select_emit      : after select_count, with n_out_vertices, n_out_faces its counts (both >= 1): the kept vertices (and normals, unless
 *                    NULL) and the kept faces, re-indexed, in their original relative order
 * All return -1 without a launch for a null required pointer or a size below 1. */
long long ngp_mesh_components_bytes(int n_faces, int n_vertices);
int ngp_mesh_components_rounds(const int32_t* faces, int n_faces, int n_vertices, int32_t* parent, int32_t* changed, int n_rounds,
                               void* stream);
int ngp_mesh_components_label(const int32_t* faces, int n_faces, int n_vertices, const int32_t* parent, void* workspace,
                              int32_t* vertex_component, int32_t* face_component, int32_t* counts /*[3]*/, void* stream);
int ngp_mesh_components_edge_keys(const int32_t* faces, int n_faces, int n_vertices, int64_t* keys /*[3 T]*/, void* stream);
int ngp_mesh_components_table(int n_faces, int n_vertices, const int32_t* vertex_component, const int32_t* face_component,
                              const int64_t* sorted_keys, int n_components, int32_t* table /*[C,6]*/, void* stream);
long long ngp_mesh_components_partial_bytes(int n_faces, int n_components);
int ngp_mesh_components_measure(const float* vertices, const int32_t* faces, const int64_t* order, int n_faces, int n_vertices,
                                const int32_t* face_start, const int32_t* block_start, int n_components, void* partials, double* area,
                                double* volume, float* lo, float* hi, void* stream);
int ngp_mesh_select_count(int n_faces, int n_vertices, const int32_t* vertex_component, const int32_t* face_component,
                          const uint8_t* keep, int n_components, void* workspace, int32_t* vertex_map, int32_t* face_map,
                          int32_t* counts /*[2]*/, void* stream);
int ngp_mesh_select_emit(const float* vertices, const float* normals /* may be NULL */, const int32_t* faces, int n_faces, int n_vertices,
                         const int32_t* vertex_map, const int32_t* face_map, int n_out_vertices, int n_out_faces, float* out_vertices,
                         float* out_normals /* NULL iff normals is */, int32_t* out_faces, void* stream);

/* ---- mesh simplification: vertex clustering on a grid with a quadric-optimal representative per cluster (csrc/mesh_simplify.hip;
 * DESIGN.md section 3).  vertices f32 [V,3], faces int32 [T,3], 1 <= V, 0 <= T (the package answers V = 0 without a call).
 * CELLS.  lo[3], inv_h[3], h[3] (f32) and n[3] are HOST arrays the caller chooses: every value finite, inv_h and h positive,
 * 1 <= n_k <= 2^21 and n_x n_y n_z < 2^63 (every key is then below INT64_MAX).  q_k = floorf((x_k - lo_k) * inv_h_k) in f32 (one subtraction, one multiplication), clamped to [0, n_k - 1] in
 * float, then key = q_x + n_x (q_y + n_y q_z) as int64.  A vertex with a coordinate that is not finite is BAD: key INT64_MAX, no
 * cluster, counted.  A face is BAD when an index is outside [0, V) or names a bad vertex: it contributes nothing, face_map -1, counted.
 * CLUSTERS.  One per distinct key, numbered 0 .. C - 1 by increasing key (a stable sort of the keys, the first slot of every run, a scan).
 * SURVIVING FACES.  A good face survives when its corners lie in three distinct clusters; survivors keep their input order and corner
 * order.  Output vertices are the clusters some surviving face names, numbered by increasing key.  Duplicate output faces stay.
 * QUADRICS, in f64 from the f32 coordinates, relative to the cell centre c = lo + (q + 1/2) h: every good face with nn = (b - a) x
 * (c' - a) != 0 adds, ONCE to each distinct cluster among its corners, with w = |nn| / 2, n = nn / |nn|, d = -n . (a - c):
 * A += w n n^T, b += w d n, area vector += nn / 2.  Per cluster also the sum of (v - c) over its vertices and their count.
 * REPRESENTATIVE.  mean = sum (v - c) / count, mu = regularization tr(A), y = (A + mu I)^-1 (-b + mu mean); y = mean when tr(A) = 0 or
 * regularization = +inf.  y is clamped to [-h / 2, h / 2] per axis and x = (float)(c + y).  The normal is the normalised area vector, 0
 * where that is 0.
 * simplify_bytes : the size of `workspace` for simplify_count (about V + T bytes)
 * simplify_keys  : keys int64 [V]; zeroes counts int32 [5] = {C, V', T', bad vertices, bad faces} and counts the bad vertices
 * simplify_count : sorted_keys, order int64 [V] = the keys in ascending order and the stable permutation that sorts them.  Writes
 *                  vertex_cluster int32 [V] (-1: bad), cluster_out int32 [V] (its first C slots: the output vertex of a cluster or -1),
 *                  vertex_map int32 [V], face_map int32 [T] (the output vertex / face, -1 for none) and the rest of counts, on the device.
 *                  T = 0 is allowed (faces and face_map may then be null).  This is all a face count needs: no quadric is formed.
 * simplify_incidence_keys : keys int64 [3 T]: key 3 f + k is the cluster of corner k of face f, INT64_MAX when the face is bad or has
 *                  nn = 0, or the cluster repeats that of an earlier corner of the face
 * simplify_runs_bytes : the size of `runs` (4-byte aligned scratch) for simplify_emit; -1 unless 1 <= V' <= C
 * simplify_emit  : incidence_keys, incidence_order int64 [3 T] = those keys sorted, stably, and the permutation; 3 T <= 2^31 - 1 (a run's
 *                  ends are int32).  n_clusters,
 *                  n_out_vertices, n_out_faces: the host's copies of counts (all >= 1).  Writes out_vertices f32 [V',3], out_normals f32
 *                  [V',3] (unless NULL) and out_faces int32 [T',3].  A cluster's sums run over its slice of the sorted lists in a fixed
 *                  order (lane l of a wave takes l, l + 64, ..., then an xor tree): no float atomics, the same input gives the same bytes.
 * All return -1 without a launch for a null required pointer, a size or grid outside the above, or a regularization that is not > 0. */
long long ngp_mesh_simplify_bytes(int n_faces, int n_vertices);
int ngp_mesh_simplify_keys(const float* vertices, int n_vertices, const float* lo /* host [3] */, const float* inv_h /* host [3] */,
                           const float* h /* host [3] */, const int32_t* n /* host [3] */, int64_t* keys /*[V]*/, int32_t* counts /*[5]*/,
                           void* stream);
int ngp_mesh_simplify_count(const int32_t* faces, int n_faces, int n_vertices, const int64_t* sorted_keys, const int64_t* order,
                            void* workspace, int32_t* vertex_cluster, int32_t* cluster_out, int32_t* vertex_map, int32_t* face_map,
                            int32_t* counts /*[5]*/, void* stream);
int ngp_mesh_simplify_incidence_keys(const float* vertices, const int32_t* faces, int n_faces, int n_vertices,
                                     const int32_t* vertex_cluster, int64_t* keys /*[3 T]*/, void* stream);
long long ngp_mesh_simplify_runs_bytes(int n_clusters, int n_out_vertices);
int ngp_mesh_simplify_emit(const float* vertices, const int32_t* faces, int n_faces, int n_vertices, const float* lo /* host [3] */,
                           const float* inv_h /* host [3] */, const float* h /* host [3] */, const int32_t* n /* host [3] */,
                           const int64_t* vertex_keys, const int64_t* vertex_order, const int64_t* incidence_keys,
                           const int64_t* incidence_order, const int32_t* vertex_cluster, const int32_t* cluster_out,
                           const int32_t* vertex_map, const int32_t* face_map, int n_clusters, int n_out_vertices, int n_out_faces,
                           double regularization, void* runs, float* out_vertices, float* out_normals /* may be NULL */,
                           int32_t* out_faces, void* stream);

/* ---- mesh smoothing: a vertex adjacency built on the device, Taubin's lambda | mu passes over it with a bounded displacement, and
 * area-weighted vertex normals (csrc/mesh_smooth.hip; DESIGN.md section 3, "Smoothing").  vertices f32 [V,3], faces int32 [T,3],
 * 1 <= V, 1 <= T, 6 T <= 2^31 - 1 (the package answers V = 0 and T = 0 without a call).
 * BAD FACES.  A face with an index outside [0, V), or with a repeated index, is BAD: it contributes nothing and is counted.
 * BAD VERTICES.  A vertex with a coordinate that is not finite is BAD: it never moves and keeps its bits, its neighbours leave it out of
 * their sums (their degree drops), it is counted.  A face that names a bad vertex is still a good face: the adjacency is integer
 * arithmetic only and depends on the set of faces alone, not on their order, their corner rotation or the schedule.
 * ADJACENCY (CSR).  Every good face emits six directed keys u V + w (int64), both directions of its three edges; a bad face emits six
 * times INT64_MAX.  sorted_keys = those keys in ascending order.  One run of equal keys is one directed edge: E2 runs in all.
 * row_start int32 [V + 1], neighbours int32 [6 T] (its first E2 slots are written), multiplicity uint8 [6 T] (likewise): the neighbours
 * of vertex v are neighbours[row_start[v] .. row_start[v + 1]), distinct and ascending; multiplicity is the run's length, the number of
 * good faces that use the undirected edge in either orientation, saturated at 255.  vertex_flags uint8 [V]: bit 0 BOUNDARY (some
 * incident edge has multiplicity 1), bit 1 NON-MANIFOLD (some incident edge has multiplicity >= 3), bit 2 UNUSED (no good face names the
 * vertex), bit 3 BAD.  counts int32 [4] = {E2, bad faces, bad vertices, boundary vertices}, on the device.
 * adjacency_bytes : the size of `workspace` for adjacency_build (about 30 T bytes); -1 for a T outside the limits
 * adjacency_keys  : keys int64 [6 T]; zeroes counts and counts the bad faces
 * adjacency_build : writes row_start, neighbours, multiplicity, vertex_flags and the rest of counts.  Nothing is read back: neighbours
 *                   and multiplicity are allocated at their bound 6 T, and a smoothing pass needs no more than row_start.
 * ONE SMOOTHING PASS (a lane per vertex) reads x_in and writes x_out, which must not be the same array.  N(i) = the row of i without
 * its bad neighbours; with boundary_mode CURVE a boundary vertex keeps only the neighbours across edges of multiplicity 1, so a boundary
 * smooths along itself.  x_out_i = x_in_i, bit for bit, when i is bad or unused, when fixed[i] != 0 (fixed uint8 [V], may be NULL), when
 * N(i) is empty, or when boundary_mode is FIXED and i is a boundary vertex; FREE treats every vertex alike.  Otherwise, per coordinate
 * and in f64 from the f32 values, every operation rounded once (no contraction):
 *     s = sum over j in N(i) of x_j, serially in ascending j;  m = s / |N(i)|;  y = x_i + factor (m - x_i);  x' = (float)y;
 *     then in f32: lo = x0_i - max_move, hi = x0_i + max_move;  x' < lo ? lo : x';  x' > hi ? hi : x'.
 * max_move: a HOST array of three f32, each >= 0, +inf = no bound on that axis (all three +inf: x0 is not read and may be NULL).  The
 * clamp makes |x' - x0| <= max_move hold up to the one rounding of x0 -+ max_move, after any number of passes.
 * mesh_smooth     : n_iterations Taubin iterations: a pass with factor lambda, then one with factor mu; mu == 0 is the plain Laplacian,
 *                   lambda passes only.  The positions start in x_a; pass p reads x_a and writes x_b for even p, the reverse for odd p,
 *                   so the result is in x_a after an even number of passes (n_iterations (mu == 0 ? 1 : 2)) and in x_b after an odd one.
 *                   x0 f32 [V,3]: the original positions, neither x_a nor x_b.  n_slots: the allocated length of neighbours and
 *                   multiplicity (rows are cut there); no index read from the CSR is followed outside [0, V).
 * vertex_normals_keys : keys int64 [3 T]: key 3 f + k is corner k of face f, INT64_MAX for a bad face
 * vertex_normals  : sorted_keys, order int64 [3 T] = those keys sorted, stably, and the permutation.  normals f32 [V,3]: the f64 sum of
 *                   the area vectors (b - a) x (c - a) / 2 of the vertex's faces in ascending slot order, divided by its length and
 *                   rounded to f32; 0 where the sum is 0 or not finite.  No float atomics: the same input gives the same bytes.
 * All return -1 without a launch for a null required pointer, a size outside the limits, a lambda or mu that is not finite, a max_move
 * that is negative or NaN, an unknown boundary_mode, or x_a == x_b. */
#define NGP_MESH_SMOOTH_FIXED 0
#define NGP_MESH_SMOOTH_CURVE 1
#define NGP_MESH_SMOOTH_FREE 2
long long ngp_mesh_adjacency_bytes(int n_faces);
int ngp_mesh_adjacency_keys(const int32_t* faces, int n_faces, int n_vertices, int64_t* keys /*[6 T]*/, int32_t* counts /*[4]*/,
                            void* stream);
int ngp_mesh_adjacency_build(const float* vertices, int n_faces, int n_vertices, const int64_t* sorted_keys, void* workspace,
                             int32_t* row_start /*[V + 1]*/, int32_t* neighbours /*[6 T]*/, uint8_t* multiplicity /*[6 T]*/,
                             uint8_t* vertex_flags /*[V]*/, int32_t* counts /*[4]*/, void* stream);
int ngp_mesh_smooth(float* x_a, float* x_b, const float* x0 /* may be NULL without a bound */, const int32_t* row_start,
                    const int32_t* neighbours, const uint8_t* multiplicity, const uint8_t* vertex_flags,
                    const uint8_t* fixed /* may be NULL */, int n_vertices, long long n_slots, int n_iterations, double lambda, double mu,
                    int boundary_mode, const float* max_move /* host [3] */, void* stream);
int ngp_mesh_vertex_normals_keys(const int32_t* faces, int n_faces, int n_vertices, int64_t* keys /*[3 T]*/, void* stream);
int ngp_mesh_vertex_normals(const float* vertices, const int32_t* faces, int n_faces, int n_vertices, const int64_t* sorted_keys,
                            const int64_t* order, float* normals /*[V,3]*/, void* stream);

/* ---- vertex colours from posed images (csrc/mesh_color.hip; DESIGN.md section 3, "Vertex colours").  vertices f32 [V,3], normals f32
 * [V,3] (unit), K f32 [3,3] (k_per_camera = 0) or [N,3,3] (1), c2w f32 [N,3,4] = (right, down, front | position) as ngp_get_rays reads it,
 * images f32 [N,H,W,C], C >= 3 (the first three channels are used), 1 <= V, 1 <= N, V N <= 2^31 - 1.  N is the number of cameras of ONE
 * CHUNK: the caller cuts the cameras into chunks, in ascending order, and passes each chunk's slices; accum, views and best_cos carry
 * across the chunks, and because every vertex meets its cameras in ascending index the result has the same bits for every chunk size.
 * PAIR j V + v is camera j of the chunk and vertex v.  In f32, every operation rounded once, dots as (x + y) + z:
 *     d = c - v;  nd = n . d;  two_sided and nd < 0: n = -n, nd = -nd;  cos = nd / sqrt(d . d)
 *     q = v - c;  p = (right . q, down . q, front . q)
 *     u = fx p.x / p.z + cx;  w = fy p.y / p.z + cy;  a = u - 0.5;  b = w - 0.5       the centre of pixel (i, j) is (i + 0.5, j + 0.5)
 *     ACCEPTED iff cos > cos_min and p.z > near and 0 <= a <= W - 1 and 0 <= b <= H - 1 and v and n are finite (a NaN fails)
 *     accepted: rays_o = v + eps n, rays_d = c - rays_o, sample = (a, b), cosv = cos, weight = cos cos
 *     rejected: rays_o = rays_d = 0 (ngp_mesh_raycast writes a miss for a zero direction without a walk), sample = cosv = weight = 0
 * eps: ONE f32 IN DEVICE MEMORY (no host read behind a default that depends on the mesh).  cos_min >= 0 and near >= 0.
 * OCCLUSION is ngp_mesh_raycast on rays_o, rays_d of the chunk with NGP_RAYCAST_ANY_HIT and t in [0, 1], called by the caller: t [V N].
 * ACCUMULATE (a lane per vertex, cameras j = 0 .. N - 1 in that order).  A pair COUNTS iff weight > 0 and t = +inf.  For one that counts:
 *     x0 = floor(a), y0 = floor(b), x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1), fx = a - x0, fy = b - y0 (f32, exact), then in f64
 *     rgb_k = (1 - fy) ((1 - fx) I[y0,x0,k] + fx I[y0,x1,k]) + fy ((1 - fx) I[y1,x0,k] + fx I[y1,x1,k])
 *     NGP_MESH_COLOR_BLEND: accum[v] += (w rgb_0, w rgb_1, w rgb_2, w), views[v] += 1
 *     NGP_MESH_COLOR_BEST : only if cos > best_cos[v], strictly (of equal cos the lowest camera stays): accum[v] = (w rgb, w),
 *                           views[v] = 1, best_cos[v] = cos
 *   accum f64 [V,4], views int32 [V] and best_cos f32 [V] (BEST only, else it may be NULL) start as zeroes.
 * FINISH: views > 0: colors = (float)(accum_k / accum_3), weight = (float)accum_3, filled = 0; else colors = weight = 0, filled = 255.
 * FILL, one Jacobi round over the CSR of ngp_mesh_adjacency_build: a vertex with filled_in = 255 and at least one neighbour with
 * filled_in != 255 takes the f64 mean of those neighbours' colours, summed in ascending neighbour order and rounded once, and
 * filled_out = round (1 .. 254); every other vertex copies filled_in.  colors is updated in place: a round writes only vertices that were
 * 255 in filled_in and reads only vertices that were not.  filled_in and filled_out must be two arrays.
 * No atomics: the same input gives the same bytes.  All return -1 without a launch for a null required pointer, a size outside the
 * limits, an unknown mode, a cos_min or near that is negative or NaN, or a round outside 1 .. 254. */
#define NGP_MESH_COLOR_BLEND 0
#define NGP_MESH_COLOR_BEST 1
int ngp_mesh_color_project(const float* vertices, const float* normals, int n_vertices, const float* K, int k_per_camera,
                           const float* c2w, int n_cameras, int width, int height, const float* eps /* device [1] */, float cos_min,
                           float near, int two_sided, float* rays_o /*[V N,3]*/, float* rays_d /*[V N,3]*/, float* sample /*[V N,2]*/,
                           float* weight /*[V N]*/, float* cosv /*[V N]*/, void* stream);
int ngp_mesh_color_accumulate(const float* images, int n_cameras, int height, int width, int channels, int n_vertices,
                              const float* sample, const float* weight, const float* cosv, const float* t, int mode,
                              double* accum /*[V,4]*/, int32_t* views /*[V]*/, float* best_cos /*[V], may be NULL for BLEND*/,
                              void* stream);
int ngp_mesh_color_finish(const double* accum, const int32_t* views, int n_vertices, float* colors /*[V,3]*/, float* weight /*[V]*/,
                          uint8_t* filled /*[V]*/, void* stream);
int ngp_mesh_color_fill(float* colors, const uint8_t* filled_in, uint8_t* filled_out, const int32_t* row_start,
                        const int32_t* neighbours, int n_vertices, long long n_slots, int round, void* stream);

/* ---- surface rendering: the compositor of a-7 driven by a signed distance (NeuS opacity) (csrc/surface.hip) ---------------------------
 * Per sample j of a ray: f_j = sdf, c_j = cosv = dir . grad f (formed by the caller), delta_j, t_j, rgb_j [3] and, unless aux is NULL,
 * aux_j [3] (e.g. the unit normal).  Per launch: s = inv_s[0] (DEVICE memory, one float: no host read), r = cos_anneal in [0, 1],
 * thr = T_threshold, bg.
 *     ic = -( relu(-c/2 + 1/2) (1 - r) + relu(-c) r )
 *     h  = ic delta / 2
 *     p  = sigmoid((f - h) s),  n = sigmoid((f + h) s),  sigmoid(x) = 1 / (1 + exp(-x))       (exp = inf gives 0, not NaN)
 *     a  = clip( (p - n + 1e-5) / (p + 1e-5), 0, 1 )
 *     T = 1;  stop at the first !(T > thr);  w = a T;  R += w rgb;  A += w aux;  D += w t;  O += w;  T <- T (1 - a);  M += 1
 *     rgb_out = R + bg (1 - O)
 * fwd writes total_samples[n] (= M), opacity[n], depth[n], rgb[n,3], rgb_out[n,3] (nullable), aux_out[n,3] (nullable; needs aux), all
 * indexed by the ray index rays_a[.,0], and ws[S], alphas[S]: w_j and a_j of the live samples, exact +0 behind the live count.
 * bwd takes the cotangents of opacity, depth, rgb (of rgb_out when bg != 0: the blend's share -bg sum_c dL_drgb is added to d opacity),
 * aux_out and ws -- all but dL_drgb nullable --, the forward's inputs and its total_samples and alphas, and writes d_sdf[S], d_cos[S],
 * d_rgbs[S,3], d_aux[S,3] (nullable) and d_inv_s[1].  With p' = p (1 - p), n' = n (1 - n), den = p + 1e-5, zero where the clip is active:
 *     da/df = s [ p'(1-a) - n' ] / den                     da/dh = -s [ p'(1-a) + n' ] / den
 *     da/dc = da/dh  delta/2  ( (1-r)/2 [-c/2+1/2 > 0] + r [-c > 0] )
 *     da/ds = [ (f-h) p'(1-a) - (f+h) n' ] / den
 * dL/da_j is the adjoint of the loop (a reverse sweep: finite when 1 - a_j is exactly 0) under the per-sample cotangent
 * G_j = g_rgb . rgb_j + g_aux . aux_j + g_depth t_j + g_opacity' + g_ws[j].  delta and t get no gradient.  Samples behind the live
 * count get exact +0 everywhere.  d_inv_s sums every live sample of the launch without atomics (per-ray rows in `workspace`, n_rays
 * floats, then one block in a fixed order): the same inputs give the same bits.
 * n_rays <= 0: returns 0 without a launch.  A ray with N == 0 writes zeros (rgb_out = bg).  A NaN sdf / cosv poisons its own ray only
 * (and d_inv_s).  -1 for a null required pointer. */
int ngp_surface_composite_fwd(const float* sdf, const float* cosv, const float* rgbs, const float* aux /* may be NULL */,
                              const float* deltas, const float* ts, const int32_t* rays_a, const float* inv_s /* device, [1] */,
                              float cos_anneal, float T_threshold, int n_rays, float bg, int32_t* total_samples, float* opacity,
                              float* depth, float* rgb, float* rgb_out /* may be NULL */, float* aux_out /* may be NULL */, float* ws,
                              float* alphas, void* stream);
int ngp_surface_composite_bwd(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb, const float* dL_daux,
                              const float* dL_dws, const float* sdf, const float* cosv, const float* rgbs, const float* aux,
                              const float* deltas, const float* ts, const int32_t* rays_a, const float* inv_s, float cos_anneal, int n_rays,
                              float bg, const int32_t* total_samples, const float* alphas, float* d_sdf, float* d_cos, float* d_rgbs,
                              float* d_aux /* may be NULL */, float* d_inv_s /* [1] */, float* workspace /* [n_rays] */, void* stream);

/* ---- importance resampling along rays: inverse-CDF refinement of marched sections (csrc/resample.hip) ---------------------------------
 * Sample j of a ray is the midpoint t_j of the SECTION [lo_j, hi_j] = [t_j - 0.5f delta_j, t_j + 0.5f delta_j]; gaps between sections
 * are skipped empty space.  Refinement only cuts sections: the union of a ray's sections stays what it was.  Row i of rays_a is
 * (ray index, start, N); rays_o, rays_d [n_orig, 3] and noise [n_orig] (in [0, 1)) are indexed by the RAY INDEX, ws, deltas, ts
 * [n_samples] by start + j.  K >= 1 draws per ray, floor_w >= 0 is added to every weight.  All arithmetic is f32, one rounding per
 * operation as written (no contraction), per ray in rays_a row order:
 *     w_j    = (ws_j < 0 ? 0 : ws_j) + floor_w
 *     c_j    = sum_{i <= j} w_i, summed 64 sections at a time: c_j = carry + (inclusive Kogge-Stone scan of the group, lane j mod 64:
 *              for d = 1, 2, .., 32: v_l += v_{l-d} for l >= d), carry = the c of the group's last lane, 0 for the first group
 *     the ray is COPIED THROUGH (every section kept as it is, t and delta bit for bit) if N = 0, if any ws_j is not finite, or if
 *     c_last = c_{N-1} is not > 0 or not finite
 *     draw k = 0 .. K-1:  u = (float(k) + noise) / float(K);  target = u c_last
 *         j      = the first section with c_j > target, by bisection (lo = 0, hi = N; mid = (lo + hi) / 2; c_mid > target ? hi = mid :
 *                  lo = mid + 1); no such section: the draw is dropped
 *         t*     = lo_j + (target - c_{j-1}) / w_j * delta_j           (c_{-1} = 0; left to right)
 *         kept   iff lo_j < t* < hi_j and (k = 0 or t* != the t* of draw k - 1)     (a zero-weight section gives inf / NaN: not kept)
 *     a section with m >= 1 kept cuts becomes m + 1 children with the edges lo_j, cuts.., hi_j; a child with the edges (a, b) has
 *     t = 0.5f (a + b), delta = b - a.  A section no cut fell into is its own only child, t_j and delta_j copied bit for bit.  Every
 *     child has xyz = o + t d per component, dir = d and parent = start + j, the index of its section in the INPUT buffers.
 *     Children are stored in ascending t: the first child of section j at j + (kept cuts in sections < j), the child that starts at the
 *     ray's kept cut number r (0-based, in draw order) in section j at j + r + 1.
 * count : fills the staged cuts stage_t / stage_j [n_rays K] (row i: its kept cuts, compacted, in draw order) and counts[i] = N_i +
 *         kept_i.  cdf [n_samples] is a workspace: a ray of more than 1024 sections keeps its CDF there, at start + j (shorter rays keep
 *         it in LDS and leave the workspace untouched).  A row of rays_a that points outside the buffers (ray index outside [0, n_orig), start or N < 0,
 *         start + N > n_samples) is given the count 0 and sets total[1] = 1; the caller zeroes total[2] beforehand.
 * scan  : rays_a_out[i] = (ray index of row i, exclusive prefix sum of counts, counts[i]), total[0] = the sum.  One block, no atomics.
 * write : after count and scan, with the same inputs: xyzs, dirs [total, 3], deltas_out, ts_out, parent [total].
 * No atomics anywhere: the same inputs give the same bytes.  n_rays <= 0 returns 0 without a launch; -1 for a null required pointer,
 * K < 1, n_orig < 1, n_samples < 0 or a floor_w that is not >= 0.  The caller keeps n_samples + n_rays K below 2^31. */
int ngp_resample_count(const float* ws, const float* deltas, const float* ts, const int32_t* rays_a, const float* noise, int n_rays,
                       int n_orig, long long n_samples, int K, float floor_w, float* cdf, float* stage_t, int32_t* stage_j,
                       int32_t* counts, int32_t* total /* [2], zeroed */, void* stream);
int ngp_resample_scan(const int32_t* counts, const int32_t* rays_a, int n_rays, int32_t* rays_a_out, int32_t* total, void* stream);
int ngp_resample_write(const float* rays_o, const float* rays_d, const float* deltas, const float* ts, const int32_t* rays_a,
                       const int32_t* rays_a_out, const float* stage_t, const int32_t* stage_j, int n_rays, int n_orig,
                       long long n_samples, int K, float* xyzs, float* dirs, float* deltas_out, float* ts_out, int32_t* parent,
                       void* stream);

/* ---- sphere tracing: the geometry value of an SDF field and a ray tracer over it (csrc/sdf_trace.hip) ---------------------------------
 * THE FIELD.  f(x) for a world position x in the box [-scale, scale]^3, all arithmetic f32:
 *     x01 = (x - lo) / (hi - lo), lo = -scale, hi = scale (two operations per component);
 *     enc = the F = 2 hash-grid embedding of x01 over the level table (1..16 levels, dense and hashed), bit for bit what ngp_hash_fwd_f32
 *           gives on x01 -- on faces and outside the box too; every index stays inside its level;
 *     h = [x (3) | enc (2 L)];  `depth` times  h <- softplus(W h + b)  with `width` outputs;  f = w_out . h + b_out.
 *     Every sum starts at its bias and adds its terms in input-index order, one fmaf each.  softplus is torch's Softplus(beta = 100):
 *     z = 100 h; z > 20 ? h : log1pf(expf(z)) / 100.
 * wpack, fp32: W0[width][3 + 2 L] | b0[width] | (Wi[width][width] | bi[width]) x (depth - 1) | w_out[width] | b_out.  Supported: width 16,
 * 32 or 64, depth 1 or 2 (the default field: L = 16, width 64, depth 2).
 * THE TRACE, per ray, directions unit vectors, dt_min = sqrt(3) / 1024, one rounding per operation as written:
 *     (t1, t2) = the slab test of the box (near plane 0.01).  A miss on the slab, or a t2 that is not finite: MISS with t = -1.
 *     t = t1, have_prev = false, n_eval = 0, f_last = 0.  Repeat:
 *       1. !(t < t2): MISS with t = t2.
 *       2. the occupancy cell of o + t d (the march's cell rule at step dt_min; cascades == 1: cascade 0 for every point).
 *       3. cell empty: t' = (the march's skip target from t) + dt_min, have_prev = false; !(t' > t): ABANDONED at t; t = t'.  The
 *          + dt_min puts the next probe INSIDE the next cell, never on its face.  No evaluation.
 *       4. cell occupied: n_eval == max_evals: ABANDONED at t.  f = f(o + t d), n_eval += 1, f_last = f; f not finite: ABANDONED at t.
 *       5. f > eps: prev = (t, f), have_prev = true, t = t + fmaxf(f * step_scale, min_step); repeat.
 *       6. f >= 0: HIT at t.
 *       7. !have_prev: INSIDE at t (the surface is in front of the first evaluated point of this occupied stretch).
 *       8. a = prev, b = (t, f): exactly n_refine bisections, each one evaluation that counts in n_eval and ignores max_evals:
 *          tm = 0.5f (ta + tb); fm not finite: ABANDONED at tm; fm >= 0 replaces a, otherwise b.
 *          Then t = ta + ((tb - ta) * fa) / (fa - fb): HIT at t, or ABANDONED at tb if that t is not finite.
 *     Outputs per ray: status (0 MISS, 1 HIT, 2 INSIDE, 3 ABANDONED), t, xyz = o + t d per component, n_eval, f_last (the last
 *     evaluated value).  An output depends on its ray alone: no atomics on results, the same bytes whatever the batch order.  Rows
 *     beyond n_rays are not touched.  stats (may be NULL; two counters the caller zeroes): += the lane slots of the evaluation rounds,
 *     += the slots that held an evaluation -- a measurement, the only atomics of the launch.
 * density_bitfield: cascades * grid_size^3 bits in the march's layout; coarse (may be NULL): ngp_bitfield_coarsen of it.
 * Both return 0 without a launch for n = 0, and -1 -- nothing launched, nothing written -- for n < 0, a null required pointer, a
 * level table with n_features != 2, no level or more than 16, or a level outside the table, an unsupported width / depth, a table
 * (or enc_out) that is not 8-byte aligned, scale not > 0, cascades outside 1..8, a grid_size that is not a power of two >= 8 or
 * whose cascades * grid_size^3 / 512 coarse bits exceed 32 768, eps < 0, step_scale <= 0, min_step < 0, n_refine outside 0..64 or
 * max_evals outside 0..2^20. */
int ngp_sdf_eval(const float* xyzs, const float* table, const ngp_hash_levels* lv, const float* wpack, int width, int depth, float scale,
                 int n, float* f, float* enc_out /* [n, 2 L], may be NULL */, void* stream);
int ngp_sdf_trace(const float* rays_o, const float* rays_d, const uint8_t* density_bitfield, const uint32_t* coarse /* may be NULL */,
                  const float* table, const ngp_hash_levels* lv, const float* wpack, int width, int depth, int cascades, float scale,
                  int grid_size, int n_rays, float eps, float step_scale, float min_step, int n_refine, int max_evals, int32_t* status,
                  float* t, float* xyz, int32_t* n_eval, float* f_last, unsigned long long* stats /* [2], may be NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGP_HIP_H */
