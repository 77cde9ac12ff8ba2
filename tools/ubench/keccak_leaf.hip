// The column-major Keccak-256 leaf kernel of merkle.hip on its own, for tools/isa_count.py: the same body (keccak.cuh's sponge over a
// word callback, one thread per leaf, consecutive lanes on consecutive addresses) without the rest of the library, so that the
// static count is of this kernel alone.
//
//   python tools/isa_count.py tools/ubench/keccak_leaf.hip --filter keccak_leaf_colmajor_kernel --trips 24,5,24
//
// The loops are, in the order of their back edges: the 24 rounds of a full block's permutation, the full blocks of 17 words (5 for a
// 94-column leaf), the 24 rounds of the last (padded) block's permutation.  docs/EXPERIMENTS.md ("Keccak-256 leaves") records what the tool printed.
#include <hip/hip_runtime.h>

#include "keccak.cuh"

using namespace ola;

extern "C" __global__ __launch_bounds__(256) void keccak_leaf_colmajor_kernel(const u64* __restrict__ base, size_t col_stride, int ncols, size_t num_leaves,
                                                                              u64* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= num_leaves) return;
    u64 d[4];
    keccak_hash_words([&](u32 i) { return gl_canon(base[(size_t)i * col_stride + j]); }, (u32)ncols, d);
    ulonglong2* o = reinterpret_cast<ulonglong2*>(out + j * 4);
    o[0] = make_ulonglong2(d[0], d[1]);
    o[1] = make_ulonglong2(d[2], d[3]);
}
