// Stand-alone check of OLA_TRACEGEN_CELLS_ONLY (include/ola_tracegen.h), compiled together with olavm_amd/csrc/host/tracegen.cpp under
// -fsanitize=address,undefined by tests/test_mem_tablegen_abi.py: one program with stack and heap cells, comparisons and range checks is
// run with and without the flag; the cells, sorted, must be the live rows of the ordinary memory table, the operands the comparison table's,
// the CPU's values the head of the range-check table, the three tables' shapes the ordinary ones and the other tables equal.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/ola_tracegen.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, ola_tracegen_last_error()); return 1; } } while (0)

int main() {
    const uint32_t ADD = 31, MOV = 27, MLOAD = 22, MSTORE = 21, END = 20, RC = 19, GTE = 13;
    const uint64_t P = 0xFFFFFFFF00000001ULL, top = P - 0xFFFFFFFFULL;
    std::vector<OlaInstr> p;
    p.push_back({MOV, 1, -1, -1, 1, 100});                   // r1: stack base
    p.push_back({MOV, 3, -1, -1, 1, top - 9});               // r3: heap base
    for (uint64_t i = 0; i < 4; i++) {
        p.push_back({MOV, 2, -1, -1, 1, 7 + 3 * i});
        p.push_back({MSTORE, 2, 1, -1, 1, i});
        p.push_back({MSTORE, 2, 3, -1, 1, 2 * i});
    }
    for (uint64_t i = 0; i < 4; i++) {
        p.push_back({MLOAD, 4, 1, -1, 1, 3 - i});
        p.push_back({MLOAD, 5, 3, -1, 1, 2 * i});
        p.push_back({GTE, 6, 4, 5, 0, 0});
        p.push_back({GTE, 6, 5, 4, 0, 0});
        p.push_back({RC, -1, -1, 4, 0, 0});
    }
    p.push_back({ADD, 6, 4, 5, 0, 0});
    p.push_back({END, -1, -1, -1, 0, 0});
    const uint64_t code[4] = {1, 2, 3, 4}, stor[4] = {5, 6, 7, 8};
    OlaTraceSet *full = nullptr, *lean = nullptr;
    CHECK(ola_tracegen_run(p.data(), p.size(), code, stor, 4, 2, 0, 0, 1 << 12, 0, &full) == 0);
    CHECK(ola_tracegen_run(p.data(), p.size(), code, stor, 4, 2, 0, 0, 1 << 12, OLA_TRACEGEN_CELLS_ONLY, &lean) == 0);
    uint64_t n_cells = 0, n_ops = 0, n_rc = 0, n_steps = 0;
    const uint64_t *cells = nullptr, *ops = nullptr, *rc = nullptr, *steps = nullptr;
    CHECK(ola_tracegen_mem_cells(full, &n_cells, &cells) == -1 && ola_tracegen_cmp_ops(full, &n_ops, &ops) == -1 &&
          ola_tracegen_cpu_rc_values(full, &n_rc, &rc) == -1);
    CHECK(ola_tracegen_mem_cells(lean, &n_cells, &cells) == 0 && ola_tracegen_cmp_ops(lean, &n_ops, &ops) == 0 &&
          ola_tracegen_cpu_rc_values(lean, &n_rc, &rc) == 0);
    CHECK(ola_tracegen_cpu_steps(lean, &n_steps, &steps) == 0 && n_steps == ola_tracegen_cpu_rows(full));      // the flag implies STEPS_ONLY
    CHECK(n_cells == 16 && n_ops == 8 && n_rc == 4);
    for (uint32_t t = 0; t < 12; t++) {
        uint32_t c0, l0, c1, l1;
        const uint64_t *d0, *d1;
        CHECK(ola_tracegen_table(full, t, &c0, &l0, &d0) == 0 && ola_tracegen_table(lean, t, &c1, &l1, &d1) == 0);
        CHECK(c0 == c1 && l0 == l1 && d0);
        const size_t n = (size_t)1 << l0;
        if (t == 1) {                                        // memory: columns 3, 4, 5, 18, 17 of its live rows are the sorted cells
            CHECK(!d1 && c0 == 29);
            std::vector<std::array<uint64_t, 5>> sorted(n_cells);
            for (size_t i = 0; i < n_cells; i++) sorted[i] = {cells[i], cells[n_cells + i], cells[2 * n_cells + i], cells[3 * n_cells + i], cells[4 * n_cells + i]};
            std::sort(sorted.begin(), sorted.end());         // no two cells of this program share (address, clock)
            const size_t cols[5] = {3, 4, 5, 18, 17};
            for (size_t i = 0; i < n_cells; i++)
                for (size_t k = 0; k < 5; k++) CHECK(d0[cols[k] * n + i] == sorted[i][k]);
            CHECK(d0[2 * n + n_cells - 1] == 1 && d0[2 * n + n_cells] == 0);
        } else if (t == 3) {
            CHECK(!d1 && c0 == 6);
            for (size_t i = 0; i < n_ops; i++) CHECK(d0[i] == ops[i] && d0[n + i] == ops[n_ops + i] && d0[5 * n + i] == 1);
        } else if (t == 4) {
            CHECK(!d1 && c0 == 12);
            for (size_t i = 0; i < n_rc; i++) CHECK(d0[4 * n + i] == rc[i] && d0[i] == 1);       // RC_VAL, RC_CPU_FILTER
        } else if (t == 0 || t == 10) {
            CHECK(!d1);
        } else {
            CHECK(d1 && std::memcmp(d0, d1, (size_t)c0 * n * 8) == 0);
        }
    }
    ola_tracegen_free(full);
    ola_tracegen_free(lean);
    std::printf("ok: %llu cells\n", (unsigned long long)n_cells);
    return 0;
}
