// The C++ host layer's ola_host::check_constraints (include/ola_host.hpp) on an instance the test hands over as a file of u64 words:
//   [airset_words, airset..., n_params, params..., n_tables, (log_n, n_words, words...)*]
// Prints one line per failure: "table section index kind first_row rows_failing".  Without arguments: usage, exit 2, no device touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "ola_host.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: host_check_constraints <instance> [table_mask]\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint64_t> w;
    for (uint64_t x; f.read(reinterpret_cast<char*>(&x), 8);) w.push_back(x);
    size_t p = 0;
    auto take = [&](size_t n) { std::vector<uint64_t> v(w.begin() + (long)p, w.begin() + (long)(p + n)); p += n; return v; };
    const std::vector<uint64_t> airset = take(w.at(p++));
    const std::vector<uint64_t> params = take(w.at(p++));
    const size_t nt = w.at(p++);
    std::vector<std::vector<uint64_t>> traces;
    std::vector<uint32_t> log_n;
    for (size_t t = 0; t < nt; t++) {
        log_n.push_back((uint32_t)w.at(p++));
        traces.push_back(take(w.at(p++)));
    }
    const uint32_t mask = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 0) : 0xFFFFFFFFu;
    try {
        ola_host::Gpu gpu(0);
        // twice: with the library's own challenges and with supplied ones -- the AIR and permutation sections do not depend on them
        const auto a = ola_host::check_constraints(gpu, airset, traces, log_n, params, mask);
        const auto b = ola_host::check_constraints(gpu, airset, traces, log_n, params, mask, {{{3, 5}}, {{7, 11}}});
        if (a.size() != b.size()) { std::printf("reports differ in length: %zu %zu\n", a.size(), b.size()); return 1; }
        for (size_t i = 0; i < a.size(); i++) {
            const OlaConstraintFailure &x = a[i], &y = b[i];
            if (x.table != y.table || x.section != y.section || x.index != y.index || x.kind != y.kind || x.first_row != y.first_row ||
                x.rows_failing != y.rows_failing) { std::printf("reports differ at entry %zu\n", i); return 1; }
            std::printf("%u %u %u %u %llu %llu\n", x.table, x.section, x.index, x.kind, (unsigned long long)x.first_row, (unsigned long long)x.rows_failing);
        }
    } catch (const ola_host::Error& e) {
        std::printf("error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
