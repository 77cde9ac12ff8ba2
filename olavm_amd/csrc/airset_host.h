// The AIR-set description as the host reads it: tables (constraint programs, permutation pairs) and cross-table lookups, parsed from
// the u64 blob olavm_amd/air/dsl.py writes.  Host only (no HIP): the prover (stark.hip), the constraint check (check.hip) and the
// verifier's host stage (verify_host.h) share it.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/ola_gpu.h"
#include "gl.cuh"
#include "ola_error.h"

namespace ola {

// ------------------------------------------------------------------------------------------------ AIR-set (host)
enum { AOP_LOCAL = 0, AOP_NEXT, AOP_CONST, AOP_PARAM, AOP_ADD, AOP_SUB, AOP_MUL, AOP_EMIT, AOP_ISZERO };
enum { AK_ALL = 0, AK_TRANSITION, AK_FIRST, AK_LAST };

struct HLinCol { std::vector<std::pair<u64, u64>> terms; u64 constant = 0; };
struct HTwc { int table = 0; std::vector<HLinCol> columns; bool has_filter = false; HLinCol filter; };
struct HCtl { std::vector<HTwc> looking; HTwc looked; };
struct HTable {
    int ncols = 0, constraint_degree = 0, n_regs = 0, n_params = 0;
    std::vector<std::vector<std::pair<u64, u64>>> perm_pairs;
    std::vector<u64> ops;  // 2 words per op
    int quotient_degree_factor() const { return std::max(1, constraint_degree - 1); }
    int permutation_batch_size() const { return quotient_degree_factor(); }
    int num_permutation_batches(int nch) const {
        const int inst = (int)perm_pairs.size() * nch;
        return inst ? (inst + permutation_batch_size() - 1) / permutation_batch_size() : 0;
    }
};
struct HAirSet { std::vector<HTable> tables; std::vector<HCtl> ctls; };

inline HAirSet parse_airset(const u64* w, size_t n) {
    size_t p = 0;
    auto next = [&]() -> u64 {
        if (p >= n) throw OlaError(OLA_E_INVALID_ARG, "AIR-set blob truncated");
        return w[p++];
    };
    if (next() != 0x4F4C41414952ull || next() != 1) throw OlaError(OLA_E_INVALID_ARG, "AIR-set blob: bad magic/version");
    const size_t nt = next(), nc = next();
    HAirSet s;
    for (size_t t = 0; t < nt; t++) {
        HTable a;
        a.ncols = (int)next(); a.constraint_degree = (int)next(); a.n_regs = (int)next(); a.n_params = (int)next();
        const size_t np = next();
        for (size_t i = 0; i < np; i++) {
            const size_t len = next();
            std::vector<std::pair<u64, u64>> pr;
            for (size_t k = 0; k < len; k++) { const u64 l = next(); const u64 r = next(); pr.push_back({l, r}); }
            a.perm_pairs.push_back(pr);
        }
        const size_t nops = next();
        for (size_t i = 0; i < 2 * nops; i++) a.ops.push_back(next());
        s.tables.push_back(a);
    }
    auto col = [&]() { HLinCol c; const size_t k = next(); for (size_t i = 0; i < k; i++) { const u64 cc = next(); const u64 f = next(); c.terms.push_back({cc, f}); } c.constant = next(); return c; };
    auto twc = [&]() { HTwc t; t.table = (int)next(); const size_t k = next(); for (size_t i = 0; i < k; i++) t.columns.push_back(col()); t.has_filter = next() != 0; if (t.has_filter) t.filter = col(); return t; };
    for (size_t c = 0; c < nc; c++) {
        HCtl ctl;
        const size_t nl = next();
        for (size_t i = 0; i < nl; i++) ctl.looking.push_back(twc());
        ctl.looked = twc();
        for (auto& t : ctl.looking) if (t.table < 0 || t.table >= (int)nt) throw OlaError(OLA_E_INVALID_ARG, "CTL table index");
        if (ctl.looked.table < 0 || ctl.looked.table >= (int)nt) throw OlaError(OLA_E_INVALID_ARG, "CTL table index");
        s.ctls.push_back(ctl);
    }
    if (p != n) throw OlaError(OLA_E_INVALID_ARG, "AIR-set blob has trailing words");
    return s;
}

}  // namespace ola
