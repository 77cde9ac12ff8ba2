// Stand-alone check of OLA_TRACEGEN_HASHES_ONLY (include/ola_tracegen.h), compiled together with olavm_amd/csrc/host/tracegen.cpp under
// -fsanitize=address,undefined by tests/test_storage_tablegen_abi.py: a program that stores a slot, loads it and overwrites it is run with
// and without the flag (program hash proven).  The lean run's access records must be what the ordinary storage table holds per 256-row
// block, its Poseidon inputs and filters the ordinary Poseidon table's with the accesses' 512 rows left zero, the two tables' shapes the
// ordinary ones, the other tables equal, and ola_tracegen_program_beta of the ordinary run's roots the ordinary run's challenge.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/ola_tracegen.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (%s)\n", __LINE__, #c, ola_tracegen_last_error()); return 1; } } while (0)

int main() {
    const uint32_t MOV = 27, MSTORE = 21, END = 20, SLOAD = 11, SSTORE = 10;
    std::vector<OlaInstr> p;
    p.push_back({MOV, 1, -1, -1, 1, 200});                   // r1: the slot key's address
    p.push_back({MOV, 3, -1, -1, 1, 300});                   // r3: the stored value's address
    p.push_back({MOV, 4, -1, -1, 1, 400});                   // r4: where SLOAD puts the value
    for (uint64_t i = 0; i < 4; i++) {
        p.push_back({MOV, 2, -1, -1, 1, 9 + i});
        p.push_back({MSTORE, 2, 1, -1, 1, i});
        p.push_back({MOV, 2, -1, -1, 1, 70 + 5 * i});
        p.push_back({MSTORE, 2, 3, -1, 1, i});
    }
    p.push_back({SSTORE, -1, 1, 3, 0, 0});
    p.push_back({SLOAD, -1, 1, 4, 0, 0});
    p.push_back({MOV, 2, -1, -1, 1, 123456789});
    p.push_back({MSTORE, 2, 3, -1, 1, 2});
    p.push_back({SSTORE, -1, 1, 3, 0, 0});
    p.push_back({END, -1, -1, -1, 0, 0});
    const uint64_t code[4] = {1, 2, 3, 4}, stor[4] = {5, 6, 7, 8};
    const uint32_t hash = OLA_TRACEGEN_PROVE_PROGRAM_HASH;
    OlaTraceSet *full = nullptr, *lean = nullptr, *cells = nullptr, *fixed = nullptr;
    CHECK(ola_tracegen_run(p.data(), p.size(), code, stor, 4, 2, 0, 0, 1 << 12, hash, &full) == 0);
    CHECK(ola_tracegen_run(p.data(), p.size(), code, stor, 4, 2, 0, 0, 1 << 12, hash | OLA_TRACEGEN_HASHES_ONLY, &lean) == 0);
    CHECK(ola_tracegen_run(p.data(), p.size(), code, stor, 4, 2, 0, 0, 1 << 12, hash | OLA_TRACEGEN_CELLS_ONLY, &cells) == 0);
    CHECK(ola_tracegen_run(p.data(), p.size(), code, stor, 4, 2, 77, 88, 1 << 12, hash | OLA_TRACEGEN_HASHES_ONLY | OLA_TRACEGEN_EXPLICIT_BETAS, &fixed) == 0);
    uint64_t n_access = 0, n = 0, betas[2], lean_betas[2];
    const uint64_t *acc = nullptr, *in = nullptr, *f = nullptr, *data = nullptr;
    uint32_t log_p = 0;
    CHECK(ola_tracegen_storage_accesses(full, &n_access, &acc) == -1 && ola_tracegen_poseidon_inputs(full, &log_p, &in, &f) == -1);
    CHECK(ola_tracegen_storage_accesses(cells, &n_access, &acc) == -1 && std::strstr(ola_tracegen_last_error(), "HASHES_ONLY"));
    CHECK(ola_tracegen_storage_accesses(lean, &n_access, &acc) == 0 && ola_tracegen_poseidon_inputs(lean, &log_p, &in, &f) == 0);
    uint64_t n_cells = 0;
    CHECK(ola_tracegen_mem_cells(cells, &n_cells, &data) == 0 && ola_tracegen_mem_cells(lean, &n, &data) == 0 && n == n_cells && n > 30);   // the flag implies CELLS_ONLY
    CHECK(n_access == 5);
    const uint64_t want_flags[5] = {1 | 4, 1, 0, 1, 2};      // the silent write of the program hash, SSTORE, SLOAD, SSTORE, the program-hash read
    for (size_t a = 0; a < 5; a++) CHECK(acc[12 * n_access + a] == want_flags[a]);
    CHECK(ola_tracegen_betas(full, betas) == 0 && ola_tracegen_betas(lean, lean_betas) == 0);
    CHECK(lean_betas[0] == betas[0] && lean_betas[1] == ~0ull);                                                    // not known before the tree is hashed
    CHECK(ola_tracegen_betas(fixed, lean_betas) == 0 && lean_betas[0] == 77 && lean_betas[1] == 88);
    uint32_t c5, l5, c7, l7, c, l;
    const uint64_t *psdn, *st, *none;
    CHECK(ola_tracegen_table(full, 5, &c5, &l5, &psdn) == 0 && ola_tracegen_table(full, 7, &c7, &l7, &st) == 0 && psdn && st && c5 == 134 && c7 == 48);
    CHECK(ola_tracegen_table(lean, 5, &c, &l, &none) == 0 && !none && c == c5 && l == l5 && l == log_p);
    CHECK(ola_tracegen_table(lean, 7, &c, &l, &none) == 0 && !none && c == c7 && l == l7);
    const size_t np = (size_t)1 << l5, ns = (size_t)1 << l7;
    CHECK(ns == 1024 && st[47 * ns + 1023] == 0);            // four accesses with rows: no padding
    std::vector<char> owned(np, 0);
    for (size_t a = 1, q = 0; a < 5; a++, q++) {
        const size_t leaf = 256 * q + 255;
        for (size_t w = 0; w < 4; w++) {
            CHECK(acc[w * n_access + a] == st[(13 + w) * ns + leaf]);                 // the tree key: COL_ST_ADDR_RANGE
            CHECK(acc[(4 + w) * n_access + a] == st[(21 + w) * ns + leaf]);           // the leaf after the access: COL_ST_PATH_RANGE at layer 256
        }
        CHECK((acc[12 * n_access + a] & 1) == st[9 * ns + leaf] && ((acc[12 * n_access + a] >> 1) & 1) == st[46 * ns + leaf]);
        CHECK(st[0 * ns + leaf] == q + 1);
        const size_t row = acc[13 * n_access + a];
        CHECK(row + 512 <= np);
        for (size_t k = 0; k < 512; k++) {
            CHECK(!owned[row + k] && psdn[2 * np + row + k] + psdn[3 * np + row + k] == 1);       // a storage leaf or branch hash of the ordinary table
            owned[row + k] = 1;
        }
        CHECK(psdn[2 * np + row + 510] == 1 && psdn[2 * np + row + 511] == 1 && psdn[3 * np + row] == 1);          // layer 256 last, layer 1 first
    }
    for (size_t w = 0; w < 4; w++) CHECK(acc[w * n_access] == code[w] && acc[w * n_access + 4] == code[w] && acc[(4 + w) * n_access] == acc[(4 + w) * n_access + 4]);
    for (size_t r = 0; r < np; r++) {
        for (size_t k = 0; k < 4; k++) CHECK(f[k * np + r] == (owned[r] ? 0 : psdn[k * np + r]));
        for (size_t k = 0; k < 12; k++) CHECK(in[k * np + r] == (owned[r] ? 0 : psdn[(4 + k) * np + r]));
        if (!owned[r]) CHECK(psdn[2 * np + r] == 0 && psdn[3 * np + r] == 0);
    }
    // the challenge from the ordinary run's roots: PRE_ROOT of the first row, ROOT of the last
    uint64_t roots[8], beta = 0;
    for (size_t w = 0; w < 4; w++) { roots[w] = st[(1 + w) * ns]; roots[4 + w] = st[(5 + w) * ns + ns - 1]; }
    CHECK(ola_tracegen_program_beta(roots, &beta) == 0 && beta == betas[1]);
    CHECK(ola_tracegen_program_beta(nullptr, &beta) == -1 && ola_tracegen_program_beta(roots, nullptr) == -1);
    for (uint32_t t = 0; t < 12; t++) {
        uint32_t c0, l0, c1, l1, c2, l2;
        const uint64_t *d0, *d1, *d2;
        CHECK(ola_tracegen_table(full, t, &c0, &l0, &d0) == 0 && ola_tracegen_table(lean, t, &c1, &l1, &d1) == 0 && ola_tracegen_table(cells, t, &c2, &l2, &d2) == 0);
        CHECK(c0 == c1 && l0 == l1 && c0 == c2 && l0 == l2 && d0);
        if (t == 5 || t == 7) CHECK(!d1 && d2 && std::memcmp(d0, d2, ((size_t)c0 << l0) * 8) == 0);
        else if (t == 0 || t == 1 || t == 3 || t == 4 || t == 10) CHECK(!d1 && !d2);
        else CHECK(d1 && std::memcmp(d0, d1, ((size_t)c0 << l0) * 8) == 0);
    }
    ola_tracegen_free(full);
    ola_tracegen_free(lean);
    ola_tracegen_free(cells);
    ola_tracegen_free(fixed);
    std::printf("ok: %llu accesses\n", (unsigned long long)n_access);
    return 0;
}
