// The exclusive int scan shared by marching cubes (mc_kernels.hip) and the triangle grid (mesh_distance_kernels.hip): three passes over
// kChunk-element blocks -- per-block sums, a one-workgroup scan of the sums, a local scan plus the block's offset.  Deterministic: no
// atomics.  Everything has internal linkage: each translation unit that includes this header gets its own kernels.
#pragma once

#include "sobfu_device.hpp"
#include "sobfu_scan_layout.hpp"  // kBlock, kItems, kChunk

namespace sobfu_hip {
namespace {

// block-wide exclusive prefix of one int per lane; returns the prefix, *total = block sum (valid in every lane)
SOBFU_DEV int block_exclusive(int v, int* total, int* s_wave /* kBlock / 64 + 1 */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int n = __shfl_up(incl, o, 64);
        if (lane >= o) incl += n;
    }
    __syncthreads();  // s_wave may still be read from the previous call
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        int t = s_wave[w];
        if (w < wave) base += t;
        sum += t;
    }
    *total = sum;
    return base + incl - v;
}

// pass 2: exclusive scan of n ints by ONE workgroup (n = number of workgroups of pass 1 / pass 3: a few thousand)
SOBFU_DEV void scan_blocks(int* __restrict__ v, int n, int* __restrict__ total_out) {
    __shared__ int s_wave[17];
    __shared__ int s_carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int b = 0; b < n; b += 1024) {
        const int i = b + threadIdx.x, x = i < n ? v[i] : 0;
        int incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int base = s_carry;
        for (int w = 0; w < wave; ++w) base += s_wave[w];
        if (i < n) v[i] = base + incl - x;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = base + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = s_carry;
}
__global__ void __launch_bounds__(1024) scan_blocks_kernel(int* __restrict__ v, int n, int* __restrict__ total_out) { scan_blocks(v, n, total_out); }

// generic int exclusive scan, same three passes: sums of kChunk-element blocks, scan of the sums, local scan + offset
__global__ void __launch_bounds__(kBlock) chunk_sum_kernel(const int* __restrict__ in, int n, int* __restrict__ block_sum) {
    __shared__ int s_wave[kBlock / 64 + 1];
    int s = 0;
    for (int it = 0; it < kItems; ++it) {
        const size_t i = (size_t) blockIdx.x * kChunk + (size_t) it * kBlock + threadIdx.x;
        s += i < (size_t) n ? in[i] : 0;
    }
    int total;
    block_exclusive(s, &total, s_wave);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}
__global__ void __launch_bounds__(kBlock) chunk_scan_kernel(const int* __restrict__ in, int n, const int* __restrict__ block_off,
                                                            int* __restrict__ out) {
    __shared__ int s_wave[kBlock / 64 + 1];
    int run = block_off[blockIdx.x];
#pragma unroll 1
    for (int it = 0; it < kItems; ++it) {
        const size_t i = (size_t) blockIdx.x * kChunk + (size_t) it * kBlock + threadIdx.x;
        const int x = i < (size_t) n ? in[i] : 0;
        int total;
        const int pos = run + block_exclusive(x, &total, s_wave);
        if (i < (size_t) n) out[i] = pos;
        run += total;
    }
}

int scan_in_place_sums(int* d_sums, int nb, int* d_total, hipStream_t st) {
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1024), 0, st, d_sums, nb, d_total);
    return (int) hipGetLastError();
}

// exclusive scan of n ints, in -> out (two arrays), d_blk: (n + kChunk - 1) / kChunk + 1 ints of scratch whose last element
// receives the total
inline int scan_exclusive(const int* d_in, int n, int* d_out, int* d_blk, hipStream_t st) {
    const int nb = (n + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(chunk_sum_kernel, dim3(nb), dim3(kBlock), 0, st, d_in, n, d_blk);
    int rc = (int) hipGetLastError();
    if (rc == 0) rc = scan_in_place_sums(d_blk, nb, d_blk + nb, st);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(chunk_scan_kernel, dim3(nb), dim3(kBlock), 0, st, d_in, n, (const int*) d_blk, d_out);
    return (int) hipGetLastError();
}

}  // namespace
}  // namespace sobfu_hip
