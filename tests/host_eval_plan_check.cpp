// olavm_amd/csrc/eval_plan.h on the host alone: the launch plan of eval_points_wide_kernel for every size and column count, with
// and without OLA_EVAL_WIDE_KH, and the values it takes at the shapes the suite proves.  Run by tests/test_host_api.py.
#include <cstdio>
#include <cstring>

#include "eval_plan.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_plan(int log_n, uint32_t ncols, unsigned forced) {
    const ola::EvalWidePlan p = ola::eval_wide_plan(log_n, ncols, forced);
    const int h = (log_n + 1) / 2;
    const size_t nlo_blocks = ((size_t)1 << h) / 256, nhi = (size_t)1 << (log_n - h);
    const unsigned per = p.kh_per_block;
    CHECK(per >= 2 && per % 2 == 0, "log_n %d cols %u forced %u: per %u (the kernel takes two steps per turn)", log_n, ncols, forced, per);
    CHECK(nhi % per == 0, "log_n %d cols %u forced %u: per %u does not divide nhi %zu", log_n, ncols, forced, per, nhi);
    CHECK(per <= ola::kEvalWideMaxKh, "log_n %d cols %u forced %u: per %u (1024 products of 2^54 is the bound of the 64-bit sums)", log_n, ncols, forced, per);
    CHECK((size_t)p.nchunks == nlo_blocks * nhi / per, "log_n %d cols %u forced %u: %u chunks", log_n, ncols, forced, p.nchunks);
    CHECK(nlo_blocks * 256 == ((size_t)1 << h), "log_n %d: the lo table is not a whole number of workgroups", log_n);
    if (forced) CHECK(per == (forced < nhi ? forced : nhi), "log_n %d cols %u: forced %u gives %u", log_n, ncols, forced, per);
    else CHECK(per >= 32 || per == nhi, "log_n %d cols %u: per %u", log_n, ncols, per);
}

int main() {
    for (int log_n = ola::kEvalWideMinLogN; log_n <= 30; log_n++)
        for (uint32_t ncols = 1; ncols <= 200; ncols++) {
            check_plan(log_n, ncols, 0);
            for (unsigned forced = 2; forced <= 512; forced *= 2) check_plan(log_n, ncols, forced);
        }
    // the shapes whose proof bytes the suite compares: 32 steps per workgroup, whatever the column count
    for (int log_n = 15; log_n <= 18; log_n++)
        for (uint32_t ncols = 1; ncols <= 200; ncols++)
            CHECK(ola::eval_wide_plan(log_n, ncols, 0).kh_per_block == 32, "log_n %d cols %u: %u", log_n, ncols, ola::eval_wide_plan(log_n, ncols, 0).kh_per_block);
    CHECK(ola::eval_wide_plan(20, 94, 0).kh_per_block == 32, "2^20 x 94: %u", ola::eval_wide_plan(20, 94, 0).kh_per_block);
    // the longer loops: full-size proofs only
    CHECK(ola::eval_wide_plan(22, 94, 0).kh_per_block == 128, "2^22 x 94: %u", ola::eval_wide_plan(22, 94, 0).kh_per_block);
    CHECK(ola::eval_wide_plan(23, 94, 0).kh_per_block == 256, "2^23 x 94: %u", ola::eval_wide_plan(23, 94, 0).kh_per_block);
    CHECK(ola::eval_wide_plan(24, 94, 0).kh_per_block == 512, "2^24 x 94: %u", ola::eval_wide_plan(24, 94, 0).kh_per_block);
    // what tests/test_gpu_fallback_paths.py forces
    CHECK(ola::eval_wide_plan(15, 9, 2).kh_per_block == 2 && ola::eval_wide_plan(15, 9, 2).nchunks == 64, "2 at 2^15");
    CHECK(ola::eval_wide_plan(15, 9, 512).kh_per_block == 128 && ola::eval_wide_plan(15, 9, 512).nchunks == 1, "512 at 2^15 clamps to nhi");
    CHECK(ola::eval_wide_plan(18, 9, 64).kh_per_block == 64 && ola::eval_wide_plan(18, 9, 64).nchunks == 16, "64 at 2^18");
    CHECK(ola::eval_wide_plan(18, 9, 512).kh_per_block == 512 && ola::eval_wide_plan(18, 9, 512).nchunks == 2, "512 at 2^18");
    // the switch's values
    const struct { const char* s; unsigned want; } env[] = {{nullptr, 0}, {"", 0}, {"0", 0}, {"1", 0}, {"2", 2}, {"3", 0}, {"64", 64}, {"512", 512},
        {"1024", 0}, {"-2", 0}, {"+2", 0}, {" 2", 0}, {"2 ", 0}, {"2x", 0}, {"0x10", 0}, {"96", 0}, {"99999999999999999999999", 0}};
    for (const auto& e : env)
        CHECK(ola::eval_wide_forced_kh(e.s) == e.want, "OLA_EVAL_WIDE_KH=%s gives %u", e.s ? e.s : "(unset)", ola::eval_wide_forced_kh(e.s));
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("eval plan ok\n");
    return 0;
}
