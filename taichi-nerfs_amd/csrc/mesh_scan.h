// mesh_scan.h -- the integer scan of a flag array that the mesh files number things with (components, selection, simplification):
// a wave per MESH_SCAN_CHUNK slots counts, one block scans the chunk totals, the wave walk again writes the indices.  Three launches,
// integer arithmetic only: the result depends on the flags alone.
#pragma once
#include "ngp_device.h"

namespace ngp {

constexpr int MESH_SCAN_CHUNK = 512;       // slots per wave of the scan: 8 rounds of 64 lanes

__host__ __device__ __forceinline__ long long mesh_scan_chunks(long long n) { return (n + MESH_SCAN_CHUNK - 1) / MESH_SCAN_CHUNK; }

static __global__ void __launch_bounds__(256) mesh_scan_count_kernel(const uint8_t* __restrict__ flags, int bit, long long n, int32_t* chunk) {
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long first = wave * MESH_SCAN_CHUNK;
    if (first >= n) return;
    const int lane = threadIdx.x & 63;
    int total = 0;
    for (int r = 0; r < MESH_SCAN_CHUNK / 64; ++r) {
        const long long i = first + 64 * r + lane;
        const bool on = i < n && (flags[i] & bit);
        total += __popcll(__ballot(on));
    }
    if (lane == 0) chunk[wave] = total;
}

// one block: exclusive scan of the chunk totals in place, their sum (<= n < 2^31) to *total
static __global__ void __launch_bounds__(256) mesh_scan_block_kernel(int32_t* __restrict__ chunk, long long chunks, int32_t* __restrict__ total) {
    __shared__ int part[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long long run = (chunks + 255) / 256;
    const long long lo = min(t * run, chunks), hi = min(lo + run, chunks);
    int s = 0;
    for (long long c = lo; c < hi; ++c) s += chunk[c];
    const int incl = wave_scan_add_i(s, lane);
    if (lane == 63) part[wv] = incl;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < wv) base += part[k];
        all += part[k];
    }
    if (t == 0) *total = all;
    int acc = base + incl - s;
    for (long long c = lo; c < hi; ++c) {
        const int x = chunk[c];
        chunk[c] = acc;
        acc += x;
    }
}

// RUNS = false: index[i] = the number of flagged slots before i where slot i is flagged, else -1.
// RUNS = true : index[i] = the number of flagged slots up to and including i, minus one: with the first slot of every run flagged, the
//               number of the run that slot i lies in (-1 in front of the first flag).
template <bool RUNS>
__global__ void __launch_bounds__(256) mesh_scan_index_kernel(const uint8_t* __restrict__ flags, int bit, long long n,
                                                              const int32_t* __restrict__ chunk, int32_t* __restrict__ index) {
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long first = wave * MESH_SCAN_CHUNK;
    if (first >= n) return;
    const int lane = threadIdx.x & 63;
    int run = chunk[wave];
    for (int r = 0; r < MESH_SCAN_CHUNK / 64; ++r) {
        const long long i = first + 64 * r + lane;
        const bool on = i < n && (flags[i] & bit);
        const unsigned long long m = __ballot(on);
        const int before = run + __popcll(m & ((1ull << lane) - 1ull));
        if (i < n) index[i] = RUNS ? before + (on ? 1 : 0) - 1 : (on ? before : -1);
        run += __popcll(m);
    }
}

// index[i] of the flagged slots of flags[0, n), their number to *total; chunk: int32 [mesh_scan_chunks(n)] of scratch
template <bool RUNS = false>
static inline void mesh_scan(const uint8_t* flags, int bit, long long n, int32_t* chunk, int32_t* index, int32_t* total, hipStream_t s) {
    const long long chunks = mesh_scan_chunks(n);
    const unsigned blocks = (unsigned)((chunks + 3) / 4);
    hipLaunchKernelGGL(mesh_scan_count_kernel, dim3(blocks), dim3(256), 0, s, flags, bit, n, chunk);
    hipLaunchKernelGGL(mesh_scan_block_kernel, dim3(1), dim3(256), 0, s, chunk, chunks, total);
    hipLaunchKernelGGL(mesh_scan_index_kernel<RUNS>, dim3(blocks), dim3(256), 0, s, flags, bit, n, chunk, index);
}

}  // namespace ngp
