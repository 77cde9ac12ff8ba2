// The C++ host layer's ola_host::check_lookup (include/ola_host.hpp) on an instance the test hands over as a file of u64 words:
//   [airset_words, airset..., n_tables, (log_n, n_words, words...)*]      (a table the lookup does not name may have 0 words)
// Prints the report's text (ola_host::LookupReport::text, the lines of olavm_amd.backend.format_lookup_report).  Without arguments:
// usage, exit 2, no device touched.  With "--args": the argument checks the library makes before it looks for a device (what a host
// without a GPU can exercise; also the stand-alone program for a sanitizer build of the host-side code), exit 0 when all hold.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "ola_host.hpp"

static int argument_checks(const std::vector<uint64_t>& airset, const std::vector<std::vector<uint64_t>>& traces, const std::vector<uint32_t>& log_n) {
    std::vector<std::vector<const uint64_t*>> cols(traces.size());
    std::vector<const uint64_t* const*> tabs;
    for (size_t t = 0; t < traces.size(); t++) {
        const size_t n = (size_t)1 << log_n[t];
        for (size_t c = 0; c * n < traces[t].size(); c++) cols[t].push_back(traces[t].data() + c * n);
        tabs.push_back(cols[t].empty() ? nullptr : cols[t].data());
    }
    std::vector<OlaLookupMismatch> out(4);
    uint32_t n = 77, width = 0;
    uint64_t totals[4] = {0, 0, 0, 0};
    int bad = 0;
    auto expect = [&](const char* what, int32_t rc, int32_t want) {
        if (rc != want) { std::printf("%s: returned %d, expected %d (%s)\n", what, rc, want, ola_gpu_last_error()); bad++; }
    };
    expect("lookup out of range", ola_check_lookup(nullptr, airset.data(), airset.size(), tabs.data(), log_n.data(), 1000, out.data(), 4, &n, totals, &width), OLA_E_INVALID_ARG);
    expect("n_out NULL", ola_check_lookup(nullptr, airset.data(), airset.size(), tabs.data(), log_n.data(), 0, out.data(), 4, nullptr, totals, &width), OLA_E_INVALID_ARG);
    expect("cap without out", ola_check_lookup(nullptr, airset.data(), airset.size(), tabs.data(), log_n.data(), 0, nullptr, 4, &n, totals, &width), OLA_E_INVALID_ARG);
    expect("truncated blob", ola_check_lookup(nullptr, airset.data(), airset.size() - 1, tabs.data(), log_n.data(), 0, out.data(), 4, &n, totals, &width), OLA_E_INVALID_ARG);
    const int32_t rc = ola_check_lookup(nullptr, airset.data(), airset.size(), tabs.data(), log_n.data(), 0, out.data(), 4, &n, totals, &width);
    if (rc != OLA_E_NO_DEVICE && rc != OLA_E_INVALID_ARG) { std::printf("ctx NULL: returned %d\n", rc); bad++; }
    if (n != 77) { std::printf("a refused call wrote n_out\n"); bad++; }
    std::printf("argument checks: %d failed\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: host_check_lookup <instance> <lookup> [max_tuples] | host_check_lookup <instance> --args\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint64_t> w;
    for (uint64_t x; f.read(reinterpret_cast<char*>(&x), 8);) w.push_back(x);
    size_t p = 0;
    auto take = [&](size_t n) { std::vector<uint64_t> v(w.begin() + (long)p, w.begin() + (long)(p + n)); p += n; return v; };
    const std::vector<uint64_t> airset = take(w.at(p++));
    const size_t nt = w.at(p++);
    std::vector<std::vector<uint64_t>> traces;
    std::vector<uint32_t> log_n;
    for (size_t t = 0; t < nt; t++) {
        log_n.push_back((uint32_t)w.at(p++));
        traces.push_back(take(w.at(p++)));
    }
    if (!std::strcmp(argv[2], "--args")) return argument_checks(airset, traces, log_n);
    const uint32_t lookup = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    const uint32_t max_tuples = argc > 3 ? (uint32_t)std::strtoul(argv[3], nullptr, 0) : 0;
    try {
        ola_host::Gpu gpu(0);
        std::printf("%s\n", ola_host::check_lookup(gpu, airset, traces, log_n, lookup, max_tuples).text().c_str());
    } catch (const ola_host::Error& e) {
        std::printf("error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
