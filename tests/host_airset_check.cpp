// The AIR-set parser (olavm_amd/csrc/airset_host.h) by itself, without a device and without the library: a stand-alone program that
// tests/test_airset_host.py builds with g++ (a second time with -fsanitize=address,undefined) and runs.
//
//   host_airset_check BLOBS
//
// BLOBS is a file of little-endian 64-bit words: a count, then per blob its length and its words.  The first blob is the one the
// mutations are applied to.  Every blob must parse.  Then, with a walker of its own (not the product's parser) that finds the words:
//   ops         per table with a program and per opcode, the first op with that opcode: each field set to its first out-of-range value
//               (dst / a / b = n_regs, a = ncols of LOCAL / NEXT, a = n_params of PARAM, op = AOP_ISZERO + 1, kind = AK_LAST + 1) is
//               refused, and set to its last in-range value still parses
//   pairs       per table with permutation pairs: the first left and the first right column = ncols are refused
//   lookups     per lookup, on the looked and the first looking side: the first data-column term and the first filter term = ncols are refused
//   dimensions  per table: ncols, n_regs, n_params = 2^63 are refused
//   framing     magic, truncated by one word, two trailing words are refused
// "refused" is OlaError with OLA_E_INVALID_ARG.  Prints the number of mutations tried per class.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../olavm_amd/csrc/airset_host.h"

using namespace ola;

static int failures = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            failures++;                                     \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
        }                                                   \
    } while (0)

static const size_t NONE = ~(size_t)0;
struct TableAt { size_t header = 0, first_pair = NONE, ops = 0, n_ops = 0; };   // first_pair: the (left, right) words of the first pair
struct SideAt { size_t table = 0, data_term = NONE, filter_term = NONE; };      // the column word of the first term
struct CtlAt { SideAt looking, looked; bool has_looking = false; };

struct Walker {
    const std::vector<u64>& w; size_t p = 4; std::vector<TableAt> tables; std::vector<CtlAt> ctls;
    explicit Walker(const std::vector<u64>& blob) : w(blob) {}
    size_t lincol() { const size_t k = (size_t)w.at(p++), first = k ? p : NONE; p += 2 * k + 1; return first; }
    SideAt side() {
        SideAt s;
        s.table = (size_t)w.at(p++);
        const size_t k = (size_t)w.at(p++);
        for (size_t i = 0; i < k; i++) { const size_t f = lincol(); if (s.data_term == NONE) s.data_term = f; }
        if (w.at(p++)) s.filter_term = lincol();
        return s;
    }
    void all() {
        const size_t nt = (size_t)w.at(2), nc = (size_t)w.at(3);
        for (size_t t = 0; t < nt; t++) {
            TableAt a;
            a.header = p; p += 4;
            const size_t np = (size_t)w.at(p++);
            for (size_t i = 0; i < np; i++) { const size_t len = (size_t)w.at(p++); if (len && a.first_pair == NONE) a.first_pair = p; p += 2 * len; }
            a.n_ops = (size_t)w.at(p++); a.ops = p; p += 2 * a.n_ops;
            tables.push_back(a);
        }
        for (size_t c = 0; c < nc; c++) {
            CtlAt a;
            const size_t nl = (size_t)w.at(p++);
            for (size_t i = 0; i < nl; i++) { const SideAt s = side(); if (!a.has_looking) { a.looking = s; a.has_looking = true; } }
            a.looked = side();
            ctls.push_back(a);
        }
    }
};

// 0: parses, 1: refused as the caller's error, 2: anything else
static int outcome(const std::vector<u64>& blob) {
    try { (void)parse_airset(blob.data(), blob.size()); return 0; }
    catch (const OlaError& e) { return e.code == OLA_E_INVALID_ARG && std::string(e.what()).rfind("AIR-set blob", 0) == 0 ? 1 : 2; }
    catch (...) { return 2; }
}
static int with_word(std::vector<u64> blob, size_t at, u64 value) { blob.at(at) = value; return outcome(blob); }

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: host_airset_check BLOBS\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    auto word = [&]() { u64 x = 0; in.read(reinterpret_cast<char*>(&x), 8); return x; };
    std::vector<std::vector<u64>> blobs((size_t)word());
    for (auto& b : blobs) { b.resize((size_t)word()); for (u64& x : b) x = word(); }
    if (!in || blobs.empty()) { fprintf(stderr, "short file\n"); return 2; }
    for (size_t i = 0; i < blobs.size(); i++) CHECK(outcome(blobs[i]) == 0, "blob %zu does not parse", i);
    if (failures) return 1;

    const std::vector<u64>& blob = blobs[0];
    Walker wk(blob);
    wk.all();
    CHECK(wk.p == blob.size(), "the walker ends at %zu of %zu words", wk.p, blob.size());
    size_t n_ops = 0, n_pairs = 0, n_lookups = 0, n_dims = 0, n_framing = 0;

    // ---- ops: the field `mask << shift` of op word `at` set to `bad` (refused) and to `bad - 1` (parses)
    for (size_t t = 0; t < wk.tables.size(); t++) {
        const TableAt& a = wk.tables[t];
        const u64 ncols = blob[a.header], n_regs = blob[a.header + 2], n_params = blob[a.header + 3];
        auto field = [&](size_t at, int shift, u64 mask, u64 bad, const char* what) {
            const u64 w0 = blob[at] & ~(mask << shift);
            CHECK(bad <= mask && bad > 0, "table %zu: %s = %llu does not fit its field", t, what, bad);
            CHECK(with_word(blob, at, w0 | bad << shift) == 1, "table %zu, op word %zu: %s = %llu is not refused", t, at, what, bad);
            CHECK(with_word(blob, at, w0 | (bad - 1) << shift) == 0, "table %zu, op word %zu: %s = %llu does not parse", t, at, what, bad - 1);
            n_ops++;
        };
        bool seen[AOP_ISZERO + 1] = {};
        for (size_t k = 0; k < a.n_ops; k++) {
            const size_t at = a.ops + 2 * k;
            const int op = (int)(blob[at] & 0xff);
            if (op > AOP_ISZERO || seen[op]) continue;
            seen[op] = true;
            const bool binary = op == AOP_ADD || op == AOP_SUB || op == AOP_MUL;
            if (op != AOP_EMIT) field(at, 16, 0xffff, n_regs, "dst");
            if (binary || op == AOP_EMIT || op == AOP_ISZERO) field(at, 32, 0xffff, n_regs, "a (register)");
            if (op == AOP_LOCAL || op == AOP_NEXT) field(at, 32, 0xffff, ncols, "a (column)");
            if (op == AOP_PARAM) field(at, 32, 0xffff, n_params, "a (parameter)");
            if (binary) field(at, 48, 0xffff, n_regs, "b");
            field(at, 8, 0xff, AK_LAST + 1, "kind");
            // the opcode: the last in-range one, AOP_ISZERO, reads a as a register, whatever this op read it as
            CHECK(with_word(blob, at, (blob[at] & ~0xffull) | (AOP_ISZERO + 1)) == 1, "table %zu, op word %zu: opcode %d is not refused", t, at, AOP_ISZERO + 1);
            const bool iszero_fits = ((blob[at] >> 32) & 0xffff) < n_regs && ((blob[at] >> 16) & 0xffff) < n_regs;
            CHECK(with_word(blob, at, (blob[at] & ~0xffull) | AOP_ISZERO) == (iszero_fits ? 0 : 1), "table %zu, op word %zu: as opcode %d", t, at, AOP_ISZERO);
            n_ops++;
        }
        // ---- pairs
        if (a.first_pair != NONE) {
            CHECK(with_word(blob, a.first_pair, ncols) == 1, "table %zu: left column %llu of a permutation pair is not refused", t, ncols);
            CHECK(with_word(blob, a.first_pair + 1, ncols) == 1, "table %zu: right column %llu of a permutation pair is not refused", t, ncols);
            CHECK(with_word(blob, a.first_pair, ncols - 1) == 0 && with_word(blob, a.first_pair + 1, ncols - 1) == 0, "table %zu: a pair of column %llu does not parse", t, ncols - 1);
            n_pairs += 2;
        }
        // ---- dimensions
        for (size_t f : {0, 2, 3}) { CHECK(with_word(blob, a.header + f, 1ull << 63) == 1, "table %zu: header word %zu = 2^63 is not refused", t, f); n_dims++; }
    }
    // ---- lookups
    for (size_t c = 0; c < wk.ctls.size(); c++) {
        auto side = [&](const SideAt& s, const char* which) {
            const u64 ncols = blob[wk.tables.at(s.table).header];
            for (size_t at : {s.data_term, s.filter_term}) {
                if (at == NONE) continue;
                CHECK(with_word(blob, at, ncols) == 1, "lookup %zu, %s side: column %llu (word %zu) is not refused", c, which, ncols, at);
                CHECK(with_word(blob, at, ncols - 1) == 0, "lookup %zu, %s side: column %llu (word %zu) does not parse", c, which, ncols - 1, at);
                n_lookups++;
            }
        };
        side(wk.ctls[c].looked, "looked");
        if (wk.ctls[c].has_looking) side(wk.ctls[c].looking, "first looking");
    }
    // ---- framing
    auto framing = [&](const std::vector<u64>& b, const char* what) { CHECK(outcome(b) == 1, "%s is not refused", what); n_framing++; };
    { std::vector<u64> b = blob; b[0] ^= 1; framing(b, "a bad magic"); }
    framing(std::vector<u64>(blob.begin(), blob.end() - 1), "a blob truncated by one word");
    { std::vector<u64> b = blob; b.push_back(blob[0]); b.push_back(blob[1]); framing(b, "a blob with two trailing words"); }

    printf("mutations: ops %zu pairs %zu lookups %zu dimensions %zu framing %zu\n", n_ops, n_pairs, n_lookups, n_dims, n_framing);
    printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
