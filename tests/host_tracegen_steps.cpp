// Stand-alone check of OLA_TRACEGEN_STEPS_ONLY (include/ola_tracegen.h), compiled together with olavm_amd/csrc/host/tracegen.cpp under
// -fsanitize=address,undefined by tests/test_cpu_tablegen_abi.py: one program with tape, storage and memory instructions is run with and
// without the flag; the records must be the ordinary CPU table's columns, the listing the ordinary program table's, the other tables equal.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/ola_tracegen.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, ola_tracegen_last_error()); return 1; } } while (0)

int main() {
    // r9 = fp; r1 = 100 (base), store 1..4 at [100..103] and key words at [104..107], sstore, sload, tstore 4 words, tload them back, end
    const uint32_t ADD = 31, MOV = 27, MSTORE = 21, END = 20, SLOAD = 11, SSTORE = 10, TLOAD = 9, TSTORE = 8;
    std::vector<OlaInstr> p;
    p.push_back({MOV, 1, -1, -1, 1, 100});
    for (uint64_t i = 0; i < 8; i++) {
        p.push_back({MOV, 2, -1, -1, 1, 7 + i});
        p.push_back({MSTORE, 2, 1, -1, 1, i});
    }
    p.push_back({ADD, 3, 1, -1, 1, 4});              // r3 = 104: the slot key; r1 = 100: the value
    p.push_back({SSTORE, -1, 3, 1, 0, 0});
    p.push_back({MOV, 4, -1, -1, 1, 200});
    p.push_back({SLOAD, -1, 3, 4, 0, 0});
    p.push_back({TSTORE, -1, 1, -1, 1, 4});
    p.push_back({MOV, 5, -1, -1, 1, 300});
    p.push_back({MOV, 6, -1, -1, 1, 1});
    p.push_back({TLOAD, 5, 6, -1, 1, 4});
    p.push_back({END, -1, -1, -1, 0, 0});
    const uint64_t code[4] = {1, 2, 3, 4}, stor[4] = {5, 6, 7, 8};
    OlaTraceSet *full = nullptr, *lean = nullptr;
    CHECK(ola_tracegen_run(p.data(), p.size(), code, stor, 4, 2, 0, 0, 1 << 12, 0, &full) == 0);
    CHECK(ola_tracegen_run(p.data(), p.size(), code, stor, 4, 2, 0, 0, 1 << 12, OLA_TRACEGEN_STEPS_ONLY, &lean) == 0);
    uint64_t n_steps = 0;
    uint32_t log_n = 0;
    const uint64_t *steps = nullptr, *listing = nullptr, *data = nullptr;
    CHECK(ola_tracegen_cpu_steps(full, &n_steps, &steps) == -1 && ola_tracegen_prog_listing(full, &log_n, &listing) == -1);
    CHECK(ola_tracegen_cpu_steps(lean, &n_steps, &steps) == 0 && ola_tracegen_prog_listing(lean, &log_n, &listing) == 0);
    CHECK(n_steps == ola_tracegen_cpu_rows(full) && n_steps == ola_tracegen_cpu_rows(lean) && n_steps > 20);
    for (uint32_t t = 0; t < 12; t++) {
        uint32_t c0, l0, c1, l1;
        const uint64_t *d0, *d1;
        CHECK(ola_tracegen_table(full, t, &c0, &l0, &d0) == 0 && ola_tracegen_table(lean, t, &c1, &l1, &d1) == 0);
        CHECK(c0 == c1 && l0 == l1 && d0);
        const size_t n = (size_t)1 << l0;
        if (t == 0) {
            CHECK(!d1 && c0 == 94);
            for (size_t w = 0; w < 65; w++) CHECK(std::memcmp(steps + w * n_steps, d0 + (w + 1) * n, n_steps * 8) == 0);
            CHECK(std::memcmp(steps + 65 * n_steps, d0 + 88 * n, n_steps * 8) == 0);
        } else if (t == 10) {
            CHECK(!d1 && c0 == 18 && l0 == log_n);
            const size_t cols[7] = {0, 1, 2, 3, 4, 5, 17};
            for (size_t k = 0; k < 7; k++) CHECK(std::memcmp(listing + k * n, d0 + cols[k] * n, n * 8) == 0);
        } else {
            CHECK(d1 && std::memcmp(d0, d1, (size_t)c0 * n * 8) == 0);
        }
    }
    uint64_t b0[2], b1[2];
    CHECK(ola_tracegen_betas(full, b0) == 0 && ola_tracegen_betas(lean, b1) == 0 && b0[0] == b1[0] && b0[1] == b1[1]);
    (void)data;
    ola_tracegen_free(full);
    ola_tracegen_free(lean);
    std::printf("ok: %llu steps\n", (unsigned long long)n_steps);
    return 0;
}
