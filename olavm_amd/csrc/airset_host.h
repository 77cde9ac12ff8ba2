// The AIR-set description as the host reads it: tables (constraint programs, permutation pairs) and cross-table lookups, parsed from
// the u64 blob olavm_amd/air/dsl.py writes.  Host only (no HIP): the prover (stark.hip), the constraint check (check.hip) and the
// verifier's host stage (verify_host.h) share it.
// parse_airset is the only way from a blob to an HAirSet, and it returns only sets that are safe to run: every register, column and
// parameter an op, a permutation pair or a lookup column names lies inside its table (validate_airset), so no reader checks again.
// air_op is the one decoder of an op word, for the host and for the device interpreter (air_interp.cuh).
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ola_gpu.h"
#include "gl.cuh"
#include "ola_error.h"

namespace ola {

// ------------------------------------------------------------------------------------------------ AIR-set (host)
enum { AOP_LOCAL = 0, AOP_NEXT, AOP_CONST, AOP_PARAM, AOP_ADD, AOP_SUB, AOP_MUL, AOP_EMIT, AOP_ISZERO };
enum { AK_ALL = 0, AK_TRANSITION, AK_FIRST, AK_LAST };

// one op of a constraint program: w0 = op | kind << 8 | dst << 16 | a << 32 | b << 48, w1 = the immediate of AOP_CONST
struct AirOp { int op, kind; u32 dst, a, b; u64 imm; };
GL_HD AirOp air_op(u64 w0, u64 w1) {
    return AirOp{(int)(w0 & 0xff), (int)((w0 >> 8) & 0xff), (u32)((w0 >> 16) & 0xffff), (u32)((w0 >> 32) & 0xffff), (u32)((w0 >> 48) & 0xffff), w1};
}

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

// Everything a kernel or the verifier indexes with, held to its table: what the constraint programs, the permutation pairs and the
// lookup columns name.  (That the two sides of a lookup are equally wide is check_lookup's own need: check.hip.)
inline void validate_airset(const HAirSet& s) {
    auto require = [](bool ok, const char* what) { if (!ok) throw OlaError(OLA_E_INVALID_ARG, std::string("AIR-set blob: ") + what); };
    for (const HTable& t : s.tables) {
        const u32 ncols = (u32)t.ncols, n_regs = (u32)t.n_regs, n_params = (u32)t.n_params;
        for (size_t k = 0; k + 1 < t.ops.size(); k += 2) {
            const AirOp o = air_op(t.ops[k], t.ops[k + 1]);
            const bool reads_b = o.op == AOP_ADD || o.op == AOP_SUB || o.op == AOP_MUL, reads_a = reads_b || o.op == AOP_EMIT || o.op == AOP_ISZERO;
            require(o.op <= AOP_ISZERO && o.kind <= AK_LAST, "unknown constraint operation or kind");
            require((o.op == AOP_EMIT || o.dst < n_regs) && (!reads_a || o.a < n_regs) && (!reads_b || o.b < n_regs), "a constraint program names a register beyond n_regs");
            require((o.op != AOP_LOCAL && o.op != AOP_NEXT) || o.a < ncols, "a constraint program names a column beyond its table");
            require(o.op != AOP_PARAM || o.a < n_params, "a constraint program names a parameter beyond n_params");
        }
        for (const auto& pairs : t.perm_pairs)
            for (const auto& lr : pairs) require(lr.first < ncols && lr.second < ncols, "a permutation pair names a column beyond its table");
    }
    auto side = [&](const HTwc& t) {
        require(t.table >= 0 && t.table < (int)s.tables.size(), "a lookup names a table beyond the set");
        const u64 ncols = (u64)s.tables[(size_t)t.table].ncols;
        for (const HLinCol& c : t.columns) for (const auto& term : c.terms) require(term.first < ncols, "a lookup names a column beyond its table");
        if (t.has_filter) for (const auto& term : t.filter.terms) require(term.first < ncols, "a lookup's filter names a column beyond its table");
    };
    for (const HCtl& c : s.ctls) { for (const HTwc& t : c.looking) side(t); side(c.looked); }
}

inline HAirSet parse_airset(const u64* w, size_t n) {
    size_t p = 0;
    auto next = [&]() -> u64 {
        if (p >= n) throw OlaError(OLA_E_INVALID_ARG, "AIR-set blob truncated");
        return w[p++];
    };
    // a table's dimensions: at most what the 16-bit operand fields of an op can name, so the cast to int is exact
    auto dim = [&]() -> int { const u64 v = next(); if (v > 0x10000) throw OlaError(OLA_E_INVALID_ARG, "AIR-set blob: a table dimension is out of range"); return (int)v; };
    if (next() != 0x4F4C41414952ull || next() != 1) throw OlaError(OLA_E_INVALID_ARG, "AIR-set blob: bad magic/version");
    const size_t nt = next(), nc = next();
    HAirSet s;
    for (size_t t = 0; t < nt; t++) {
        HTable a;
        a.ncols = dim(); a.constraint_degree = dim(); a.n_regs = dim(); a.n_params = dim();
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
        s.ctls.push_back(ctl);
    }
    if (p != n) throw OlaError(OLA_E_INVALID_ARG, "AIR-set blob has trailing words");
    validate_airset(s);
    return s;
}

}  // namespace ola
