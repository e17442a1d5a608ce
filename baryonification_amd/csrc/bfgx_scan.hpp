// bfgx_scan.hpp -- exclusive scan of int32 counts for gfx950 and its one host launcher: the "count -> scan -> fill" of the grid plan's
// per-block halo lists, of the snapshot plan's per-cell halo lists and of the two levels of the particle deposit's counting sort.
#pragma once
#include "bfgx_tables.hpp"

namespace bfgx {

// ---- exclusive scan of int32 counts (n up to 2^31): 4096 elements per block, block sums scanned by one block
constexpr int kScanPerBlock = 4 * kTabThreads;

__global__ void __launch_bounds__(kTabThreads)
scan_blocks_kernel(int64_t n, const int32_t *__restrict__ in, int32_t *__restrict__ out, int32_t *__restrict__ block_sums, int in_stride)
{
    // in_stride: words between two counts (counters that many workgroups add to sit a cache line apart)
    __shared__ int sh[kTabThreads];
    const int64_t base = (int64_t)blockIdx.x * kScanPerBlock + 4 * (int64_t)threadIdx.x;
    int v[4], s = 0;
    for (int q = 0; q < 4; ++q) { v[q] = (base + q < n) ? in[(base + q) * in_stride] : 0; s += v[q]; }
    int tot;
    int pre = block_excl_scan_int(s, sh, tot);
    for (int q = 0; q < 4; ++q) { if (base + q < n) out[base + q] = pre; pre += v[q]; }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

// one block: exclusive scan of up to kScanPerBlock block sums, in place; total -> *total_out
__global__ void __launch_bounds__(kTabThreads)
scan_sums_kernel(int nb, int32_t *__restrict__ block_sums, int64_t *__restrict__ total_out)
{
    __shared__ int sh[kTabThreads];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < nb; c0 += kScanPerBlock) {
        const int base = c0 + 4 * threadIdx.x;
        int v[4], s = 0;
        for (int q = 0; q < 4; ++q) { v[q] = (base + q < nb) ? block_sums[base + q] : 0; s += v[q]; }
        int tot;
        int pre = block_excl_scan_int(s, sh, tot) + (int)carry;
        for (int q = 0; q < 4; ++q) { if (base + q < nb) block_sums[base + q] = pre; pre += v[q]; }
        __syncthreads();
        if (threadIdx.x == 0) carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(256)
scan_add_kernel(int64_t n, int32_t *__restrict__ out, const int32_t *__restrict__ block_sums)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] += block_sums[i / kScanPerBlock];
}

// blocks of scan_blocks_kernel for n counts = the words of block_sums a scan of n needs
inline int scan_block_count(int64_t n) { return (int)((n + kScanPerBlock - 1) / kScanPerBlock); }

// out[i] = in[0] + .. + in[i - 1] for i < n, *total = the sum of all n; block_sums [scan_block_count(n)] is scratch.  out may be in itself
// (the deposit scans its level-1 histograms in place): a block has read its 4096 counts before it writes any.  The caller checks hipGetLastError.
static inline void exclusive_scan(hipStream_t stream, int64_t n, const int32_t *in, int32_t *out, int32_t *block_sums, int64_t *total)
{
    const int nb = scan_block_count(n);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(nb), dim3(kTabThreads), 0, stream, n, in, out, block_sums, 1);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kTabThreads), 0, stream, nb, block_sums, total);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, out, (const int32_t *)block_sums);
}

}  // namespace bfgx
