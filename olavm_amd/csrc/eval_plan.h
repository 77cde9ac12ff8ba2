// The launch plan of eval_points_wide_kernel (fri.hip): how many steps of the hi power table a workgroup walks and how many chunk
// partials that leaves per column and point.  Host code only, no HIP: tests/host_eval_plan_check.cpp compiles it with a plain host
// compiler and checks it for every size and column count.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace ola {

constexpr int kEvalWideCols = 4;            // columns per workgroup (EVALW_C)
constexpr unsigned kEvalWideMaxKh = 512;    // 2 products per step and sum: 1024 x 2^54 <= 2^64 (EVALW_MAX_KH)
constexpr int kEvalWideMinLogN = 15;

struct EvalWidePlan { unsigned kh_per_block, nchunks; };

// OLA_EVAL_WIDE_KH=N: a power of two in 2..512, anything else is 0 (= not forced)
inline unsigned eval_wide_forced_kh(const char* s) {
    if (!s || !*s) return 0;
    char* end = nullptr;
    const unsigned long v = strtoul(s, &end, 10);
    if (*end || s[0] < '0' || s[0] > '9' || v < 2 || v > kEvalWideMaxKh || (v & (v - 1))) return 0;
    return (unsigned)v;
}

// z^k = lo[k mod 2^h] hi[k >> h], h = (log_n + 1) / 2: nlo_blocks = 2^h / 256 workgroups side by side cover the lo table, and the
// nhi = 2^(log_n - h) steps of the hi table are cut into nhi / kh_per_block splits; chunk = split * nlo_blocks + lo block.
// forced = 0: enough workgroups to fill the chip several times over, as many steps per workgroup as that leaves (the fold, the
// multiplication by lo[kl] and the sum over the workgroup cost about twenty steps); forced = N: min(N, nhi) steps.
inline EvalWidePlan eval_wide_plan(int log_n, uint32_t ncols, unsigned forced) {
    const int h = (log_n + 1) / 2;
    const size_t nlo_blocks = ((size_t)1 << h) / 256, nhi = (size_t)1 << (log_n - h), groups = (ncols + kEvalWideCols - 1) / kEvalWideCols;
    size_t per = kEvalWideMaxKh;
    if (forced) per = forced;
    else while (per > 32 && nlo_blocks * groups * (nhi / per) < 2048) per >>= 1;
    if (per > nhi) per = nhi;
    return EvalWidePlan{(unsigned)per, (unsigned)(nlo_blocks * (nhi / per))};
}

}  // namespace ola
