// Inclusive scan of columns of Goldilocks words, in place, three launches: the running products of the Z columns (stark.hip:
// gl_mul, prefix) and the suffix sums of the opening's division by X - z (fri.hip: gl_add, suffix).  One column per blockIdx.y:
// data at d + y * n, block totals at tot + y * scan_tot_stride(n).
//
// A tile is kScanTile = 2048 positions, 8 per thread of a 256-thread block; the thread totals go through a Hillis-Steele pass over
// 256 LDS words (8 steps, two barriers each: a faster scan is a different piece of work).  The direction is a mirrored index:
// position j of a suffix scan is word n - 1 - j, and everything else is the prefix scan over positions, so the totals kernel does
// not know the direction.  Field addition and multiplication are exact: the order of association does not show in the words.
#pragma once
#include <hip/hip_runtime.h>

#include "gl.cuh"

namespace ola {

constexpr size_t kScanTile = 2048;

struct ScanSum { static constexpr u64 identity = 0; static __device__ __forceinline__ u64 op(u64 a, u64 b) { return gl_add(a, b); } };
struct ScanProduct { static constexpr u64 identity = 1; static __device__ __forceinline__ u64 op(u64 a, u64 b) { return gl_mul(a, b); } };

template <bool Suffix>
__device__ __forceinline__ size_t scan_word(size_t j, size_t n) { return Suffix ? n - 1 - j : j; }

// Hillis-Steele over the 256 thread totals: returns thread t's inclusive total, leaves them all in sh
template <typename Op>
__device__ __forceinline__ u64 scan_block_totals(u64* sh, int t, u64 run) {
    sh[t] = run;
    __syncthreads();
    u64 incl = run;
    for (int s = 1; s < 256; s <<= 1) {
        const u64 other = (t >= s) ? sh[t - s] : Op::identity;
        __syncthreads();
        incl = Op::op(incl, other);
        sh[t] = incl;
        __syncthreads();
    }
    return incl;
}

template <typename Op, bool Suffix>
__global__ __launch_bounds__(256) void field_scan_tile_kernel(u64* __restrict__ d_all, size_t n, u64* __restrict__ tot_all, size_t tot_stride) {
    __shared__ u64 sh[256];
    u64* __restrict__ d = d_all + (size_t)blockIdx.y * n;
    u64* __restrict__ block_tot = tot_all + (size_t)blockIdx.y * tot_stride;
    const size_t j0 = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * 8;      // thread t owns positions [j0, j0 + 8)
    const int t = threadIdx.x;
    u64 v[8];
    u64 run = Op::identity;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        run = Op::op(run, j0 + i < n ? d[scan_word<Suffix>(j0 + i, n)] : Op::identity);
        v[i] = run;
    }
    const u64 incl = scan_block_totals<Op>(sh, t, run);
    const u64 excl = (t > 0) ? sh[t - 1] : Op::identity;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (j0 + i < n) d[scan_word<Suffix>(j0 + i, n)] = Op::op(v[i], excl);
    if (t == 255) block_tot[blockIdx.x] = incl;
}
// exclusive scan of a column's block totals in place, one workgroup: each thread owns a contiguous chunk, the chunk totals are
// combined as the thread totals of a tile are
template <typename Op>
__global__ __launch_bounds__(256) void field_scan_totals_kernel(u64* __restrict__ tot_all, size_t nblocks, size_t tot_stride) {
    __shared__ u64 sh[256];
    u64* __restrict__ tot = tot_all + (size_t)blockIdx.y * tot_stride;
    const int t = threadIdx.x;
    const size_t per = (nblocks + 255) / 256;
    const size_t lo = (size_t)t * per, hi = lo + per < nblocks ? lo + per : nblocks;
    u64 run = Op::identity;
    for (size_t i = lo; i < hi; i++) run = Op::op(run, tot[i]);
    scan_block_totals<Op>(sh, t, run);
    u64 acc = (t > 0) ? sh[t - 1] : Op::identity;
    for (size_t i = lo; i < hi; i++) {
        const u64 v = tot[i];
        tot[i] = acc;
        acc = Op::op(acc, v);
    }
}
template <typename Op, bool Suffix>
__global__ __launch_bounds__(256) void field_scan_apply_kernel(u64* __restrict__ d_all, size_t n, const u64* __restrict__ tot_all, size_t tot_stride) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    u64* __restrict__ d = d_all + (size_t)blockIdx.y * n;
    const u64* __restrict__ tot = tot_all + (size_t)blockIdx.y * tot_stride;
    d[k] = Op::op(d[k], tot[scan_word<Suffix>(k, n) / kScanTile]);
}

// words of block totals per column
static size_t scan_tot_stride(size_t n) { return (n + kScanTile - 1) / kScanTile + 1; }
// `ncols` adjacent columns of n words each, in place; tot: work space of ncols * scan_tot_stride(n) words
template <typename Op, bool Suffix>
void scan_inclusive(hipStream_t stream, u64* cols, size_t n, size_t ncols, u64* tot) {
    if (ncols == 0) return;
    const size_t nblocks = (n + kScanTile - 1) / kScanTile, ts = scan_tot_stride(n);
    hipLaunchKernelGGL((field_scan_tile_kernel<Op, Suffix>), dim3((unsigned)nblocks, (unsigned)ncols), dim3(256), 0, stream, cols, n, tot, ts);
    if (nblocks > 1) {
        hipLaunchKernelGGL((field_scan_totals_kernel<Op>), dim3(1, (unsigned)ncols), dim3(256), 0, stream, tot, nblocks, ts);
        hipLaunchKernelGGL((field_scan_apply_kernel<Op, Suffix>), dim3((unsigned)((n + 255) / 256), (unsigned)ncols), dim3(256), 0, stream, cols, n, tot, ts);
    }
}

}  // namespace ola
