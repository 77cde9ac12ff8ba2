// tests/host_verify_check.cpp for a StarkConfig::num_challenges other than two: the verifier's host stage (olavm_amd/csrc/verify_host.h)
// by itself, built with g++ alone by tests/test_ref_verdict_nch.py and run on tests/golden/ref_verified/wide_program_nch3.proof.
//
//   host_verify_check_nch CASES
//
// CASES is a text file of whitespace-separated words (written by the test from the AIR set and the fixture's .json):
//   hasher H
//   challenges C                                        config.num_challenges
//   proof PATH
//   blob N w0 .. wN-1
//   ctl 2C words                                        the lookup challenges the reference derived
//   tables T, then per table: nperm words.. | C alphas | zeta.a zeta.b | fri_alpha.a fri_alpha.b | nbetas (a b).. | pow_response | nidx idx..
//   cases K, then per case: byte bit where reason table query kind which        (as in host_verify_check.cpp)
// It checks: the host stage accepts the proof under C challenges and derives the recorded challenges; refuses it under two; and every case.
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

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: host_verify_check_nch CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string word, proof_path;
    vfy::Config cfg;
    std::vector<u64> blob;
    size_t n = 0;
    in >> word >> cfg.hasher >> word >> cfg.num_challenges >> word >> proof_path >> word >> n;
    blob.resize(n);
    for (u64& w : blob) in >> w;
    std::vector<uint8_t> proof;
    {
        std::ifstream pf(proof_path, std::ios::binary);
        proof.assign(std::istreambuf_iterator<char>(pf), std::istreambuf_iterator<char>());
    }
    if (!in || proof.empty() || cfg.num_challenges < 1) { fprintf(stderr, "bad case file or proof\n"); return 2; }
    const size_t nch = (size_t)cfg.num_challenges, nq = (size_t)cfg.num_queries;

    // ---- the proof as it is
    const vfy::Stage st = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, proof.data(), proof.size());
    CHECK(!st.host.failed(), "the host stage rejects the committed proof: reason %u table %d", st.host.reason, st.host.table);
    {
        vfy::Config two = cfg;
        two.num_challenges = 2;
        const vfy::Stage s2 = vfy::all_proof_stage(two, blob.data(), blob.size(), nullptr, proof.data(), proof.size());
        CHECK(s2.host.failed() && s2.host.table == 0, "two challenges: the host stage must refuse the proof at the first table's shape (reason %u table %d)", s2.host.reason, s2.host.table);
    }
    in >> word;
    CHECK(st.ctl_challenges.size() == 2 * nch, "lookup challenges: %zu", st.ctl_challenges.size());
    for (size_t i = 0; i < 2 * nch; i++) { u64 c = 0; in >> c; CHECK(i < st.ctl_challenges.size() && st.ctl_challenges[i] == c, "lookup challenge %zu", i); }
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
        CHECK(c.alphas.size() == nch, "table %zu: %zu alphas", t, c.alphas.size());
        for (size_t i = 0; i < nch; i++) { in >> x; CHECK(i < c.alphas.size() && c.alphas[i] == x, "table %zu: alpha %zu", t, i); }
        in >> x >> y; CHECK(c.zeta.a == x && c.zeta.b == y, "table %zu: zeta", t);
        in >> x >> y; CHECK(c.fri_alpha.a == x && c.fri_alpha.b == y, "table %zu: fri_alpha", t);
        in >> k;
        CHECK(c.fri_betas.size() == k, "table %zu: betas", t);
        for (size_t i = 0; i < k; i++) { in >> x >> y; CHECK(i < c.fri_betas.size() && c.fri_betas[i].a == x && c.fri_betas[i].b == y, "table %zu: beta %zu", t, i); }
        want_merkle += nq * (3 + k);
        in >> x; CHECK(c.pow_response == x, "table %zu: proof-of-work response", t);
        in >> k;
        CHECK(c.query_indices.size() == k, "table %zu: query indices", t);
        for (size_t i = 0; i < k; i++) { in >> x; CHECK(i < c.query_indices.size() && c.query_indices[i] == x, "table %zu: query index %zu", t, i); }
    }
    CHECK(st.merkle.size() == want_merkle && st.queries.size() == nq * nt, "job counts: %zu Merkle, %zu query", st.merkle.size(), st.queries.size());
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
            continue;
        }
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
    printf("%zu cases, %d failed\n", ncases, failures);
    return failures ? 1 : 0;
}
