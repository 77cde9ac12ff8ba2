// The verifier's host stage (olavm_amd/csrc/verify_host.h) by itself, without a device and without the library: a stand-alone program
// that tests/test_verify_host.py builds with g++ (a second time with -fsanitize=address,undefined) and runs on the committed proofs
// of tests/golden/ref_verified/.
//
//   host_verify_check CASES [STRIDE]
//
// STRIDE (default 1): take every STRIDE-th of the truncations and of the length prefixes -- the sanitizer build, several times slower, runs with 8.
// CASES is a text file of whitespace-separated words (written by the test from the AIR set and the fixture's .json):
//   hasher H
//   proof PATH
//   blob N w0 .. wN-1
//   ctl 4 words                                         the lookup challenges the reference derived
//   tables T, then per table: nperm words.. | alpha0 alpha1 | zeta.a zeta.b | fri_alpha.a fri_alpha.b | nbetas (a b).. | pow_response | nidx idx..
//   cases K, then per case: byte bit where reason table query kind which
//       where 0: the host stage must reject with (reason, table)
//       where 1: the host stage must pass and keep the Merkle job (table, query, kind, which)
//       where 2: the host stage must pass and keep the query job (table, query)
// It checks: the host stage accepts the proof and derives the recorded challenges; every case; truncation at 2000 seeded lengths and
// every length prefix set to all ones are refused as malformed (a path length of 0xFF: refused) -- without reading out of bounds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../olavm_amd/csrc/verify_host.h"

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

// the offsets of the length prefixes of an AllProof, found with a walker of its own (not the product's reader)
struct Walker {
    const std::vector<uint8_t>& b; size_t off = 0; std::vector<size_t> u32_at, u8_at;
    uint32_t len32() { u32_at.push_back(off); uint32_t x = 0; for (int i = 0; i < 4; i++) x |= (uint32_t)b.at(off + i) << (8 * i); off += 4; return x; }
    void vec(size_t each) { const uint32_t l = len32(); off += each * l; }
    void path() { u8_at.push_back(off); const uint8_t l = b.at(off); off += 1 + 32 * (size_t)l; }
    void all() {
        const uint32_t np = len32();
        for (uint32_t t = 0; t < np; t++) {
            for (int c = 0; c < 3; c++) vec(32);
            vec(16); vec(16); vec(16); vec(16); vec(8); vec(16);
            const uint32_t nc = len32();
            for (uint32_t i = 0; i < nc; i++) vec(32);
            const uint32_t nq = len32();
            for (uint32_t q = 0; q < nq; q++) {
                const uint32_t ni = len32();
                for (uint32_t i = 0; i < ni; i++) { vec(8); path(); }
                const uint32_t ns = len32();
                for (uint32_t i = 0; i < ns; i++) { vec(16); path(); }
            }
            vec(16);
            off += 8;
        }
        vec(8);
    }
};

int main(int argc, char** argv) {
    if (argc != 2 && argc != 3) { printf("usage: host_verify_check CASES [STRIDE]\n"); return 2; }
    const size_t stride = argc == 3 ? (size_t)std::max(1, atoi(argv[2])) : 1;
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string word, proof_path;
    vfy::Config cfg;
    std::vector<u64> blob;
    size_t n = 0;
    in >> word >> cfg.hasher >> word >> proof_path >> word >> n;
    blob.resize(n);
    for (u64& w : blob) in >> w;
    std::vector<uint8_t> proof;
    {
        std::ifstream pf(proof_path, std::ios::binary);
        proof.assign(std::istreambuf_iterator<char>(pf), std::istreambuf_iterator<char>());
    }
    if (!in || proof.empty()) { fprintf(stderr, "bad case file or proof\n"); return 2; }

    // ---- the proof as it is
    const vfy::Stage st = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, proof.data(), proof.size());
    CHECK(!st.host.failed(), "the host stage rejects the committed proof: reason %u table %d", st.host.reason, st.host.table);
    u64 ctl[4];
    in >> word;
    for (u64& c : ctl) in >> c;
    CHECK(st.ctl_challenges.size() == 4, "lookup challenges");
    for (size_t i = 0; i < 4 && i < st.ctl_challenges.size(); i++) CHECK(st.ctl_challenges[i] == ctl[i], "lookup challenge %zu", i);
    size_t nt = 0;
    in >> word >> nt;
    CHECK(st.challenges.size() == nt, "tables");
    size_t want_merkle = 0;
    for (size_t t = 0; t < nt; t++) {
        const vfy::Challenges none;
        const vfy::Challenges& c = t < st.challenges.size() ? st.challenges[t] : none;
        size_t k = 0;
        u64 x = 0, y = 0;
        in >> k;
        CHECK(c.perm.size() == k, "table %zu: permutation challenges", t);
        for (size_t i = 0; i < k; i++) { in >> x; CHECK(i < c.perm.size() && c.perm[i] == x, "table %zu: permutation challenge %zu", t, i); }
        for (size_t i = 0; i < 2; i++) { in >> x; CHECK(i < c.alphas.size() && c.alphas[i] == x, "table %zu: alpha %zu", t, i); }
        in >> x >> y; CHECK(c.zeta.a == x && c.zeta.b == y, "table %zu: zeta", t);
        in >> x >> y; CHECK(c.fri_alpha.a == x && c.fri_alpha.b == y, "table %zu: fri_alpha", t);
        in >> k;
        CHECK(c.fri_betas.size() == k, "table %zu: betas", t);
        for (size_t i = 0; i < k; i++) { in >> x >> y; CHECK(i < c.fri_betas.size() && c.fri_betas[i].a == x && c.fri_betas[i].b == y, "table %zu: beta %zu", t, i); }
        want_merkle += 28 * (3 + k);
        in >> x; CHECK(c.pow_response == x, "table %zu: proof-of-work response", t);
        in >> k;
        CHECK(c.query_indices.size() == k, "table %zu: query indices", t);
        for (size_t i = 0; i < k; i++) { in >> x; CHECK(i < c.query_indices.size() && c.query_indices[i] == x, "table %zu: query index %zu", t, i); }
    }
    CHECK(st.merkle.size() == want_merkle && st.queries.size() == 28 * nt, "job counts: %zu Merkle, %zu query", st.merkle.size(), st.queries.size());
    // the job lists lie behind the data, every job points into the data, and a wave's Merkle jobs share leaf length and depth
    CHECK(st.merkle_off <= st.query_off && st.query_off + vfy::QJ_WORDS * st.queries.size() == st.image.size(), "image layout");
    for (size_t j = 0; j < st.merkle.size(); j++) {
        const vfy::MerkleJob& m = st.merkle[j];
        CHECK(m.leaf_off + m.leaf_len <= st.merkle_off && m.sib_off + 4 * (size_t)m.depth <= st.merkle_off && m.cap_off + 4 * (size_t)m.cap_len <= st.merkle_off, "Merkle job %zu out of bounds", j);
        if (j) CHECK(st.merkle[j - 1].leaf_len < m.leaf_len || (st.merkle[j - 1].leaf_len == m.leaf_len && st.merkle[j - 1].depth <= m.depth), "Merkle job %zu out of order", j);
    }
    // all flags clear: accepted; the flags of one job set: that job's place
    {
        std::vector<uint32_t> flags(st.flags(), 0);
        CHECK(!vfy::resolve(st, flags.data()).failed(), "resolve with clear flags");
    }

    // ---- the corruptions
    size_t ncases = 0;
    in >> word >> ncases;
    for (size_t c = 0; c < ncases; c++) {
        size_t byte = 0;
        int bit = 0, where = 0, table = 0, query = 0, kind = 0, which = 0;
        uint32_t reason = 0;
        in >> byte >> bit >> where >> reason >> table >> query >> kind >> which;
        if (!in) { fprintf(stderr, "case file ends early\n"); return 2; }
        std::vector<uint8_t> bad = proof;
        bad.at(byte) ^= (uint8_t)(1u << bit);
        const vfy::Stage s = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, bad.data(), bad.size());
        if (where == 0) {
            CHECK(s.host.reason == reason && s.host.table == table, "case %zu (byte %zu): host stage says reason %u table %d, want %u / %d", c, byte, s.host.reason, s.host.table, reason, table);
            // only the tables before the failing one reached the job lists
            for (const vfy::QueryJob& q : s.queries) CHECK(q.table < table, "case %zu: a job of table %d behind the failure", c, q.table);
        } else {
            CHECK(!s.host.failed(), "case %zu (byte %zu): the host stage rejects (reason %u) what only the device can see", c, byte, s.host.reason);
            bool found = false;
            std::vector<uint32_t> flags(s.flags(), 0);
            if (where == 1) {
                for (size_t j = 0; j < s.merkle.size(); j++) {
                    const vfy::MerkleJob& m = s.merkle[j];
                    if (m.table == table && m.query == query && m.kind == kind && m.which == which) { found = true; flags[j] = vfy::MF_MISMATCH; }
                }
            } else {
                for (size_t j = 0; j < s.queries.size(); j++)
                    if (s.queries[j].table == table && s.queries[j].query == query) { found = true; flags[s.merkle.size() + j] = vfy::QF_CONSISTENCY | ((uint32_t)which << 8); }
            }
            CHECK(found, "case %zu: no job for table %d query %d kind %d which %d", c, table, query, kind, which);
            if (found) {
                const vfy::Verdict v = vfy::resolve(s, flags.data());
                CHECK(v.reason == reason && v.table == table && v.query == query && v.oracle_or_layer == which, "case %zu: resolve gives reason %u at (%d, %d, %d)", c, v.reason, v.table, v.query, v.oracle_or_layer);
            }
        }
    }

    // ---- malformed bytes: truncation at 2000 seeded lengths (and the empty proof), trailing bytes
    u64 seed = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < 2000; i += stride) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        const size_t cut = i == 0 ? 0 : (size_t)((seed >> 20) % proof.size());
        std::vector<uint8_t> part(proof.begin(), proof.begin() + (long)cut);   // an exact-size copy: a read past `cut` is a read out of bounds
        const vfy::Stage s = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, part.data(), part.size());
        CHECK(s.host.reason == OLA_VERIFY_MALFORMED && s.merkle.empty(), "truncated to %zu bytes: reason %u", cut, s.host.reason);
    }
    {
        std::vector<uint8_t> more = proof;
        more.push_back(0);
        CHECK(vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, more.data(), more.size()).host.reason == OLA_VERIFY_MALFORMED, "a trailing byte");
    }
    // ---- every length prefix all ones
    Walker wk{proof, 0, {}, {}};
    wk.all();
    CHECK(wk.off == proof.size(), "the walker does not reach the end of the proof");
    for (size_t k = 0; k < wk.u32_at.size(); k += stride) {
        const size_t at = wk.u32_at[k];
        std::vector<uint8_t> bad = proof;
        for (int i = 0; i < 4; i++) bad[at + (size_t)i] = 0xFF;
        const vfy::Stage s = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, bad.data(), bad.size());
        CHECK(s.host.reason == OLA_VERIFY_MALFORMED, "length prefix at %zu set to 0xFFFFFFFF: reason %u", at, s.host.reason);
    }
    for (size_t k = 0; k < wk.u8_at.size(); k += 7) {      // every seventh path: they are all read by the same code
        std::vector<uint8_t> bad = proof;
        bad[wk.u8_at[k]] = 0xFF;
        const vfy::Stage s = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, bad.data(), bad.size());
        CHECK(s.host.failed(), "path length at %zu set to 0xFF is accepted", wk.u8_at[k]);
    }
    // a field word >= p (the first opening of table 0) is malformed
    {
        std::vector<uint8_t> bad = proof;
        const size_t at = 4 + 3 * (4 + 16 * 32) + 4;
        for (int i = 0; i < 8; i++) bad[at + (size_t)i] = 0xFF;
        CHECK(vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, bad.data(), bad.size()).host.reason == OLA_VERIFY_MALFORMED, "a word >= p");
    }
    // a blob that is not an AIR set is the caller's error, not a verdict
    try {
        (void)vfy::all_proof_stage(cfg, blob.data(), blob.size() - 1, nullptr, proof.data(), proof.size());
        CHECK(false, "a truncated AIR-set blob is taken");
    } catch (const OlaError& e) {
        CHECK(e.code == OLA_E_INVALID_ARG, "a truncated AIR-set blob: code %d", e.code);
    }
    printf("host_verify_check: %zu length prefixes, %zu cases, %d failed\n", wk.u32_at.size() + wk.u8_at.size(), ncases, failures);
    return failures ? 1 : 0;
}
