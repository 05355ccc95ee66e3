// optim.hip -- device-resident training-step epilogue for gfx950: MSE loss + its gradient, GradScaler logic,
// cosine learning-rate schedule and a dense Adam pass that also unscales and zeroes the gradients.
//
// Replaces, for the fused trainer (ngp_hip/trainer.py), the host-driven sequence of reference train.py:193-201:
//   F.mse_loss -> grad_scaler.scale(loss).backward() -> grad_scaler.step(optimizer) [unscale pass + inf check (host
//   sync in stock torch) + Adam] -> grad_scaler.update() -> scheduler.step()  and optimizer.zero_grad().
// Everything the host used to decide (skip the step on inf/nan, grow/back off the loss scale, the step's learning
// rate and bias corrections) is decided by a one-thread prologue kernel from device-resident state, so the whole
// optimisation step is a fixed sequence of launches with no read-back (hipGraph-capturable).
// Dense Adam matches torch.optim.Adam(eps=1e-15) arithmetic (train.py:151-156): every one of the 11.4 M table entries
// is visited each step, exactly like the reference; traffic = read g,p,m,v + write p,m,v,g = 8 x 4 B per parameter
// (3 x 4 B for entries that have never received a gradient: they are exact fixed points and are left alone).
#include "ngp_device.h"

namespace ngp {


// (train_prologue_thread, the one-thread GradScaler / schedule decision, lives in ngp_device.h: round 5's scatter-add runs it too)
__global__ void train_prologue_kernel(float* __restrict__ sf, int32_t* __restrict__ si, float lr0, float eta_min, int t_max,
                                      float beta1, float beta2, float growth, float backoff, int growth_interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    train_prologue_thread(sf, si, lr0, eta_min, t_max, beta1, beta2, growth, backoff, growth_interval);
}

// Prologue of an optimizer step driven by torch.cuda.amp.GradScaler (compat/apex FusedAdam under the reference's unchanged
// train.py:143-149,198-201): the scale and the inf flag are the scaler's own device tensors, the learning rate comes from
// torch's scheduler on the host; the step counter of the bias corrections advances only when the step is not skipped.
__device__ __forceinline__ void adam_amp_prologue_thread(float* __restrict__ sf, int32_t* __restrict__ si, const float* __restrict__ grad_scale,
                                                         const bool skip, float lr, float beta1, float beta2) {
    sf[SF_INV_SCALE] = grad_scale ? 1.0f / *grad_scale : 1.0f;
    sf[SF_LR] = lr;
    si[SI_SKIP] = skip ? 1 : 0;
    if (!skip) {
        const int step = si[SI_OPT_STEP] + 1;
        si[SI_OPT_STEP] = step;
        sf[SF_BC1] = 1.0f - powf(beta1, (float)step);
        sf[SF_BC2_SQRT] = sqrtf(1.0f - powf(beta2, (float)step));
    } else {
        si[SI_SKIPPED_TOTAL] += 1;
    }
}
__global__ void adam_amp_prologue_kernel(float* __restrict__ sf, int32_t* __restrict__ si, const float* __restrict__ grad_scale,
                                         const float* __restrict__ found_inf, float lr, float beta1, float beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    adam_amp_prologue_thread(sf, si, grad_scale, found_inf && *found_inf != 0.0f, lr, beta1, beta2);
}

// The same launch also finishes the MLP backward: blocks 0..146 add up the per-block weight-gradient slabs (ngp_device.h); the
// scalar bookkeeping rides in one extra block.  The launch exists anyway and is latency-, not work-bound (5 us for one thread).
__global__ void __launch_bounds__(NGP_MLP_REDUCE_THREADS) train_prologue_reduce_kernel(float* __restrict__ sf, int32_t* __restrict__ si, float lr0,
                                                                    float eta_min, int t_max, float beta1, float beta2, float growth,
                                                                    float backoff, int growth_interval,
                                                                    const float* __restrict__ parts, int n_parts,
                                                                    float* __restrict__ dW) {
    if (blockIdx.x == NGP_MLP_REDUCE_BLOCKS) {
        if (threadIdx.x == 0) train_prologue_thread(sf, si, lr0, eta_min, t_max, beta1, beta2, growth, backoff, growth_interval);
        return;
    }
    mlp_dw_reduce_block(parts, n_parts, dW, blockIdx.x);
}

// the dense Adam pass itself (adam_table_pass) lives in ngp_device.h: the fused "table + MLP + repack" kernel of mlp.hip runs the
// same code.  SHADOW: also refresh a bf16 copy of the parameters (the table the bf16 hash forward gathers from).
template <int SHADOW>
__global__ void __launch_bounds__(256) adam_kernel(float4* __restrict__ p, float4* __restrict__ g, float4* __restrict__ m,
                                                   float4* __restrict__ v, long n4, const float* __restrict__ sf,
                                                   const int32_t* __restrict__ si, float beta1, float beta2, float eps,
                                                   uint2* __restrict__ shadow) {
    adam_table_pass<SHADOW>(p, g, m, v, n4, sf, si, beta1, beta2, eps, shadow, (long)blockIdx.x, (long)gridDim.x);
}

// Multi-tensor form (compat/apex FusedAdam: the reference's train.py:143-149 hands it model.parameters() = the table + five weight
// matrices): ONE launch sweeps all of a parameter group's tensors instead of one launch per tensor.  Every block walks the tensor
// list and takes its grid-stride share of each (the table dominates; the small matrices cost a few trips).
struct AdamMulti {
    float4* p[NGP_ADAM_MULTI_MAX];
    float4* g[NGP_ADAM_MULTI_MAX];
    float4* m[NGP_ADAM_MULTI_MAX];
    float4* v[NGP_ADAM_MULTI_MAX];
    long n4[NGP_ADAM_MULTI_MAX];
    int count;
};
__global__ void __launch_bounds__(256) adam_multi_kernel(AdamMulti T, const float* __restrict__ sf, const int32_t* __restrict__ si,
                                                         float beta1, float beta2, float eps) {
    for (int t = 0; t < T.count; ++t)
        adam_table_pass<0>(T.p[t], T.g[t], T.m[t], T.v[t], T.n4[t], sf, si, beta1, beta2, eps, (uint2*)nullptr, (long)blockIdx.x,
                           (long)gridDim.x);
}

// GradScaler's inf / nan check over up to NGP_ADAM_MULTI_MAX gradient tensors in ONE read-only pass (torch's own check,
// _amp_foreach_non_finite_check_and_unscale_ with a unit scale, reads AND rewrites every gradient: twice the traffic, and tens of
// microseconds of Python in front of it).  found[0] = 1.0f when any value is not finite; the caller clears it beforehand.
struct FiniteMulti {
    const float4* g[NGP_ADAM_MULTI_MAX];
    long n4[NGP_ADAM_MULTI_MAX];
    int count;
};
__global__ void __launch_bounds__(256) check_finite_multi_kernel(FiniteMulti T, float* __restrict__ found) {
    bool bad = false;
    for (int t = 0; t < T.count; ++t)
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < T.n4[t]; i += (long)gridDim.x * blockDim.x) {
            const float4 a = T.g[t][i];
            // x - x is 0 for every finite x and NaN for inf / NaN: one test for the four lanes' sum of such differences
            bad |= !(((a.x - a.x) + (a.y - a.y)) + ((a.z - a.z) + (a.w - a.w)) == 0.0f);
        }
    if (__any(bad) && (threadIdx.x & 63) == 0) *found = 1.0f;
}

// Round 6: the check and the prologue in ONE launch (the reference-shaped loop's optimizer step was fill + check + prologue + Adam: three
// ~5-10 us launches in front of the sweep, profiles/r06_modules_path_timeline.txt).  Every block reports with ONE relaxed atomic that
// carries both its arrival (low 16 bits; the grid has <= 4096 blocks) and whether it saw a non-finite value (high bits), so the last block
// out knows the verdict from the value the atomic returns -- no fence anywhere: a first version with __threadfence() in front of the
// arrival count took 260 us, 4096 agent-scope releases each writing back and invalidating an L2 full of the gradients just produced.
// And not one counter: 4096 same-address atomics are ~10 ns each, 54 us (measured).  Two levels: block b reports to counter b % 16 (128
// bytes apart), the last arrival of each reports that counter's sum to the top one (done[0]; the sub-counters are done[32 (1 + k)]).
// The last block stores the flag (GradScaler.update() reads it after step()), runs the one-thread prologue and rearms the counter;
// block 0 clears `clear_next`, the flag the caller hands to the NEXT step (two flags used alternately: this step's cannot be cleared
// here, and a fill launch per step is what this removes).
__global__ void __launch_bounds__(256) check_finite_prologue_kernel(FiniteMulti T, float* __restrict__ found, float* __restrict__ clear_next,
                                                                    uint32_t* __restrict__ done, float* __restrict__ sf,
                                                                    int32_t* __restrict__ si, const float* __restrict__ grad_scale, float lr,
                                                                    float beta1, float beta2) {
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int t = 0; t < T.count; ++t)
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < T.n4[t]; i += (long)gridDim.x * blockDim.x) {
            const float4 a = T.g[t][i];
            bad |= !(((a.x - a.x) + (a.y - a.y)) + ((a.z - a.z) + (a.w - a.w)) == 0.0f);
        }
    if (__any(bad) && (threadIdx.x & 63) == 0) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0 && clear_next) *clear_next = 0.0f;
        const uint32_t k = blockIdx.x & 15u, members = (gridDim.x + 15u - k) >> 4;           // blocks b with b % 16 == k
        uint32_t* sub = done + 32u * (1u + k);
        const uint32_t mine = 1u + (s_bad ? 0x10000u : 0u);
        const uint32_t old = __hip_atomic_fetch_add(sub, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((old & 0xffffu) == members - 1u) {
            __hip_atomic_store(sub, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t groups = gridDim.x < 16u ? gridDim.x : 16u;
            const uint32_t up = 1u + (((old + mine) >> 16) ? 0x10000u : 0u);
            const uint32_t top = __hip_atomic_fetch_add(done, up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((top & 0xffffu) == groups - 1u) {
                const bool skip = ((top + up) >> 16) != 0u;
                __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (skip) *found = 1.0f;
                adam_amp_prologue_thread(sf, si, grad_scale, skip, lr, beta1, beta2);
            }
        }
    }
}

__global__ void __launch_bounds__(256) cast_bf16_kernel(const float4* __restrict__ src, uint2* __restrict__ dst, long n4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 a = src[i];
        dst[i] = make_uint2(f32_to_bf16_bits(a.x) | (f32_to_bf16_bits(a.y) << 16), f32_to_bf16_bits(a.z) | (f32_to_bf16_bits(a.w) << 16));
    }
}

// rgb_final = rgb + bg (1 - opacity) (rendering.py:219-226); loss = mean((rgb_final - target)^2) (train.py:193);
// writes the LOSS-SCALED gradients w.r.t. the compositor outputs.  One block.
__global__ void __launch_bounds__(1024) mse_loss_grad_kernel(const float* __restrict__ rgb, const float* __restrict__ opacity,
                                                             const float* __restrict__ target, float bg, int n_rays,
                                                             float* __restrict__ sf, float* __restrict__ g_rgb,
                                                             float* __restrict__ g_opacity) {
    __shared__ float part[16];
    const float scale = sf[SF_LOSS_SCALE];
    const float k = 2.0f / (3.0f * (float)n_rays) * scale;
    float acc = 0.0f;
    for (int r = threadIdx.x; r < n_rays; r += blockDim.x) {
        const float b = bg * (1.0f - opacity[r]);
        float go = -0.0f;                                   // -0: go is -bg * sum(gr) down to the sign of a zero (the backend turns 0 - x into -x)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float diff = (rgb[3 * r + c] + b) - target[3 * r + c];
            acc += diff * diff;
            const float gr = k * diff;
            g_rgb[3 * r + c] = gr;
            go -= bg * gr;
        }
        g_opacity[r] = go;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += part[w];
        sf[SF_LOSS] = s / (3.0f * (float)n_rays);
    }
}

}  // namespace ngp

using namespace ngp;

extern "C" {

// ---- stream plumbing: device-scope events ---------------------------------------------------------------------------------------
// The prefetched march lives on a side stream; the two streams meet through events.  An event created without
// hipEventDisableSystemFence makes the queue write back and invalidate its caches to SYSTEM scope when it is recorded -- the step
// paid 7 + 9 us for its two meeting points.  Both sides are kernels on this device: a device-scope event is all they need.
int ngp_event_create(void** event) {
    if (!event) return -1;
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) return -1;
    *event = (void*)e;
    return 0;
}
int ngp_event_record(void* event, void* stream) { return hipEventRecord((hipEvent_t)event, (hipStream_t)stream) == hipSuccess ? 0 : -1; }
int ngp_stream_wait_event(void* stream, void* event) {
    return hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0) == hipSuccess ? 0 : -1;
}
int ngp_event_destroy(void* event) { return hipEventDestroy((hipEvent_t)event) == hipSuccess ? 0 : -1; }
// the HOST waits until the work recorded in front of the event has completed (completion only: no host-visible data is implied)
int ngp_event_synchronize(void* event) { return hipEventSynchronize((hipEvent_t)event) == hipSuccess ? 0 : -1; }

// A non-blocking stream of the LOWEST priority the device offers, for work that should only take the CUs the step's own kernels
// leave free (FusedTrainer's prefetched march: launched at equal priority it is dispatched in front of the scatter-add's persistent
// workgroups and runs beside them for the whole launch).  *lo / *hi (nullable) return the priority range.
int ngp_stream_create_low_priority(void** stream, int* lo, int* hi) {
    if (!stream) return -1;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return -1;
    hipStream_t s;
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least) != hipSuccess) return -1;
    *stream = (void*)s;
    if (lo) *lo = least;
    if (hi) *hi = greatest;
    return 0;
}
int ngp_stream_destroy(void* stream) { return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? 0 : -1; }

// A host-visible word the device can report into without anybody waiting: pinned host memory owned by the caller through this
// pair, and an asynchronous device-to-host copy on a stream of the caller's choice (FusedTrainer's side stream reports each
// prefetched march's sample count this way; the host reads whatever has arrived).  Deliberately not torch's pinned tensors:
// its caching host allocator records events on the copy's stream and would touch that stream again after ngp_stream_destroy.
int ngp_host_alloc(void** host, long long bytes) {
    if (!host || bytes <= 0) return -1;
    return hipHostMalloc(host, (size_t)bytes, hipHostMallocDefault) == hipSuccess ? 0 : -1;
}
int ngp_host_free(void* host) { return hipHostFree(host) == hipSuccess ? 0 : -1; }
int ngp_copy_to_host_async(void* host, const void* dev, long long bytes, void* stream) {
    if (!host || !dev || bytes <= 0) return -1;
    return hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? 0 : -1;
}

int ngp_train_prologue(float* state_f, int32_t* state_i, float lr0, float eta_min, int t_max, float beta1, float beta2,
                       float growth, float backoff, int growth_interval, void* stream) {
    hipLaunchKernelGGL(train_prologue_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state_f, state_i, lr0, eta_min, t_max,
                       beta1, beta2, growth, backoff, growth_interval);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_adam_amp_prologue(float* state_f, int32_t* state_i, const float* grad_scale, const float* found_inf, float lr, float beta1,
                          float beta2, void* stream) {
    hipLaunchKernelGGL(adam_amp_prologue_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state_f, state_i, grad_scale, found_inf, lr,
                       beta1, beta2);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_train_prologue_reduce(float* state_f, int32_t* state_i, float lr0, float eta_min, int t_max, float beta1, float beta2,
                              float growth, float backoff, int growth_interval, const float* dW_parts, int n_parts, float* dW,
                              void* stream) {
    if (n_parts <= 0 || !dW_parts || !dW) return -1;
    hipLaunchKernelGGL(train_prologue_reduce_kernel, dim3(NGP_MLP_REDUCE_BLOCKS + 1), dim3(NGP_MLP_REDUCE_THREADS), 0, (hipStream_t)stream, state_f, state_i,
                       lr0, eta_min, t_max, beta1, beta2, growth, backoff, growth_interval, dW_parts, n_parts, dW);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_adam_step(float* p, float* g, float* m, float* v, long long n, const float* state_f, const int32_t* state_i, float beta1,
                  float beta2, float eps, void* stream) {
    if (n <= 0) return 0;
    if (n % 4 != 0) return -1;
    const long n4 = (long)(n / 4);
    long blocks = (n4 + 255) / 256;
    if (blocks > 256L * 16) blocks = 256L * 16;
    hipLaunchKernelGGL(adam_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float4*)p, (float4*)g, (float4*)m,
                       (float4*)v, n4, state_f, state_i, beta1, beta2, eps, (uint2*)nullptr);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_adam_multi(int n_tensors, float* const* p, float* const* g, float* const* m, float* const* v, const long long* n,
                   const float* state_f, const int32_t* state_i, float beta1, float beta2, float eps, void* stream) {
    if (n_tensors <= 0) return 0;
    if (n_tensors > NGP_ADAM_MULTI_MAX || !p || !g || !m || !v || !n) return -1;
    AdamMulti T;
    long most = 0;
    T.count = n_tensors;
    for (int t = 0; t < n_tensors; ++t) {
        if (n[t] <= 0 || n[t] % 4 != 0 || !p[t] || !g[t] || !m[t] || !v[t]) return -1;
        T.p[t] = (float4*)p[t]; T.g[t] = (float4*)g[t]; T.m[t] = (float4*)m[t]; T.v[t] = (float4*)v[t];
        T.n4[t] = (long)(n[t] / 4);
        if (T.n4[t] > most) most = T.n4[t];
    }
    long blocks = (most + 255) / 256;
    if (blocks > 256L * 16) blocks = 256L * 16;
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T, state_f, state_i, beta1, beta2, eps);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_check_finite_multi(int n_tensors, const float* const* g, const long long* n, float* found_inf, void* stream) {
    if (n_tensors <= 0) return 0;
    if (n_tensors > NGP_ADAM_MULTI_MAX || !g || !n || !found_inf) return -1;
    FiniteMulti T;
    long most = 0;
    T.count = n_tensors;
    for (int t = 0; t < n_tensors; ++t) {
        if (n[t] <= 0 || n[t] % 4 != 0 || !g[t]) return -1;
        T.g[t] = (const float4*)g[t];
        T.n4[t] = (long)(n[t] / 4);
        if (T.n4[t] > most) most = T.n4[t];
    }
    long blocks = (most + 255) / 256;
    if (blocks > 256L * 16) blocks = 256L * 16;
    hipLaunchKernelGGL(check_finite_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T, found_inf);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_adam_amp_check_prologue(int n_tensors, const float* const* g, const long long* n, float* found_inf, float* clear_next,
                                uint32_t* done, float* state_f, int32_t* state_i, const float* grad_scale, float lr, float beta1,
                                float beta2, void* stream) {
    if (n_tensors <= 0 || n_tensors > NGP_ADAM_MULTI_MAX || !g || !n || !found_inf || !done || !state_f || !state_i) return -1;
    FiniteMulti T;
    long most = 0;
    T.count = n_tensors;
    for (int t = 0; t < n_tensors; ++t) {
        if (n[t] <= 0 || n[t] % 4 != 0 || !g[t]) return -1;
        T.g[t] = (const float4*)g[t];
        T.n4[t] = (long)(n[t] / 4);
        if (T.n4[t] > most) most = T.n4[t];
    }
    long blocks = (most + 255) / 256;
    if (blocks > 256L * 16) blocks = 256L * 16;          // (< 2^16: the arrival count shares its word with the verdict)
    hipLaunchKernelGGL(check_finite_prologue_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T, found_inf, clear_next, done,
                       state_f, state_i, grad_scale, lr, beta1, beta2);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_adam_step_bf16(float* p, float* g, float* m, float* v, long long n, const float* state_f, const int32_t* state_i,
                       float beta1, float beta2, float eps, uint16_t* p_bf16, void* stream) {
    if (n <= 0) return 0;
    if (n % 4 != 0 || !p_bf16) return -1;
    const long n4 = (long)(n / 4);
    long blocks = (n4 + 255) / 256;
    if (blocks > 256L * 16) blocks = 256L * 16;
    hipLaunchKernelGGL(adam_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float4*)p, (float4*)g, (float4*)m,
                       (float4*)v, n4, state_f, state_i, beta1, beta2, eps, (uint2*)p_bf16);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_cast_f32_bf16(const float* src, uint16_t* dst, long long n, void* stream) {
    if (n <= 0) return 0;
    if (n % 4 != 0) return -1;
    const long n4 = (long)(n / 4);
    long blocks = (n4 + 255) / 256;
    if (blocks > 256L * 16) blocks = 256L * 16;
    hipLaunchKernelGGL(cast_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)src, (uint2*)dst, n4);
    NGP_LAUNCH_CHECK();
    return 0;
}

// The same gradients from as many blocks as the rays need, and the per-ray squared error instead of the reduced loss (the reader sums
// it when it logs -- like ngp_composite_train_fused's sq_err): the one-block form above walks 65 536 rays in 64 dependent trips (50 us).
__global__ void __launch_bounds__(256) mse_loss_grad_rays_kernel(const float* __restrict__ rgb, const float* __restrict__ opacity,
                                                                 const float* __restrict__ target, float bg, int n_rays,
                                                                 const float* __restrict__ sf, float* __restrict__ g_rgb,
                                                                 float* __restrict__ g_opacity, float* __restrict__ sq_err) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    const float k = 2.0f / (3.0f * (float)n_rays) * sf[SF_LOSS_SCALE];
    const float b = bg * (1.0f - opacity[r]);
    float go = -0.0f, se = 0.0f;                            // (-0: see mse_loss_grad_kernel)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float diff = (rgb[3 * r + c] + b) - target[3 * r + c];
        se += diff * diff;
        const float gr = k * diff;
        g_rgb[3 * r + c] = gr;
        go -= bg * gr;
    }
    g_opacity[r] = go;
    if (sq_err) sq_err[r] = se;
}

int ngp_mse_loss_grad_rays(const float* rgb, const float* opacity, const float* target, float bg, int n_rays, const float* state_f,
                           float* g_rgb, float* g_opacity, float* sq_err, void* stream) {
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(mse_loss_grad_rays_kernel, dim3((n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, rgb, opacity, target, bg,
                       n_rays, state_f, g_rgb, g_opacity, sq_err);
    NGP_LAUNCH_CHECK();
    return 0;
}

int ngp_mse_loss_grad(const float* rgb, const float* opacity, const float* target, float bg, int n_rays, float* state_f,
                      float* g_rgb, float* g_opacity, void* stream) {
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(mse_loss_grad_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rgb, opacity, target, bg, n_rays, state_f,
                       g_rgb, g_opacity);
    NGP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
