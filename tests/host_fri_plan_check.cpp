// The FRI reduction planner (olavm_amd/csrc/fri_plan.h) and the verifier's host stage under a plan with an arity per layer
// (olavm_amd/csrc/verify_host.h), without a device and without the library: a stand-alone program that tests/test_fri_plan.py builds
// with g++ (a second time with -fsanitize=address,undefined) and runs directly.
//
//   host_fri_plan_check PLANS [PROOF_CASE]
//
// PLANS is a text file of whitespace-separated numbers, one plan per line (written by the test from tests/golden/ref_fri_plans.json):
//   strategy n args[0..n) arity_bits final_poly_bits rate_bits num_queries cap_height degree_bits len plan[0..len)
// PROOF_CASE (a proof made under MinSize(None)), whitespace-separated words:
//   hasher H
//   proof PATH
//   blob N w0 .. wN-1
//   tables T, then per table: zeta.a zeta.b | fri_alpha.a fri_alpha.b | nbetas (a b).. | pow_response | nidx idx..
// It checks: every plan; what fri_plan_spec_check refuses; with a PROOF_CASE that the host stage accepts the proof under MinSize(None)
// and derives the recorded challenges, lays every layer's evaluations out at their own width inside the image, and refuses the proof
// with a shape reason under the default strategy.
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

static size_t check_plans(const char* path) {
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    size_t count = 0;
    uint32_t strategy = 0, n = 0;
    while (in >> strategy >> n) {
        std::vector<uint32_t> args(n);
        for (uint32_t& a : args) in >> a;
        int ab = 0, fpb = 0, rate = 0, cap = 0, degree = 0;
        size_t nq = 0, len = 0;
        in >> ab >> fpb >> rate >> nq >> cap >> degree >> len;
        std::vector<int> want(len);
        for (int& w : want) in >> w;
        if (!in) { fprintf(stderr, "bad plan file at entry %zu\n", count); exit(2); }
        const char* bad = fri_plan_spec_check(strategy, args.data(), n);
        CHECK(!bad, "entry %zu: refused: %s", count, bad ? bad : "");
        if (bad) continue;
        const std::vector<int> got = fri_plan_arity_bits(fri_plan_spec(strategy, args.data(), n), ab, fpb, degree, rate, cap, nq);
        CHECK(got == want, "entry %zu: strategy %u degree_bits %d rate_bits %d queries %zu: %zu layers, expected %zu", count, strategy, degree, rate, nq,
              got.size(), want.size());
        // the verifier's Config gives the same plan
        vfy::Config cfg;
        cfg.plan = fri_plan_spec(strategy, args.data(), n);
        cfg.arity_bits = ab; cfg.final_poly_bits = fpb; cfg.rate_bits = rate; cfg.cap_height = cap; cfg.num_queries = (int)nq;
        CHECK(vfy::fri_layers(cfg, degree) == want, "entry %zu: vfy::fri_layers", count);
        count++;
    }
    return count;
}

static void check_refusals() {
    const uint32_t zero[3] = {4, 0, 3}, five[1] = {5}, two[2] = {3, 3};
    std::vector<uint32_t> many(33, 1);
    CHECK(fri_plan_spec_check(OLA_FRI_FIXED, zero, 3) != nullptr, "an entry of 0");
    CHECK(fri_plan_spec_check(OLA_FRI_FIXED, five, 1) != nullptr, "an entry of 5");
    CHECK(fri_plan_spec_check(OLA_FRI_FIXED, many.data(), 33) != nullptr, "33 layers");
    CHECK(fri_plan_spec_check(OLA_FRI_FIXED, many.data(), 32) == nullptr, "32 layers");
    CHECK(fri_plan_spec_check(OLA_FRI_FIXED, nullptr, 0) == nullptr, "no layer");
    CHECK(fri_plan_spec_check(OLA_FRI_FIXED, nullptr, 1) != nullptr, "NULL arguments");
    CHECK(fri_plan_spec_check(OLA_FRI_MIN_SIZE, two, 2) != nullptr, "MinSize with two arguments");
    CHECK(fri_plan_spec_check(OLA_FRI_MIN_SIZE, five, 1) != nullptr, "MinSize(Some(5))");
    CHECK(fri_plan_spec_check(OLA_FRI_MIN_SIZE, nullptr, 0) == nullptr, "MinSize(None)");
    CHECK(fri_plan_spec_check(OLA_FRI_CONSTANT_ARITY_BITS, five, 1) != nullptr, "ConstantArityBits with an argument");
    CHECK(fri_plan_spec_check(3, nullptr, 0) != nullptr, "an unknown strategy");
    // a plan that does not fit: more than the tree above the cap holds, and more than the degree
    CHECK(!fri_plan_fits({4, 4, 4}, 8, 3, 4), "12 bits of 8 + 3 - 4");
    CHECK(!fri_plan_fits({4, 4}, 7, 3, 0), "8 bits of degree 7");
    CHECK(fri_plan_fits({4, 3}, 8, 3, 4), "7 bits of 8 + 3 - 4");
    CHECK(fri_plan_fits({}, 0, 1, 0), "no layer");
    // the verifier refuses such a plan as the caller's mistake, before it touches the proof's queries
    vfy::Config cfg;
    const uint32_t big[3] = {4, 4, 4};
    cfg.plan = fri_plan_spec(OLA_FRI_FIXED, big, 3);
    vfy::require_config(cfg);
    cfg.plan.args[1] = 9;
    bool threw = false;
    try { vfy::require_config(cfg); } catch (const OlaError& e) { threw = e.code == OLA_E_INVALID_ARG; }
    CHECK(threw, "require_config takes a malformed plan");
}

static void check_proof(const char* path) {
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
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
    if (!in || proof.empty()) { fprintf(stderr, "bad case file or proof\n"); exit(2); }
    const vfy::Config deflt = cfg;
    cfg.plan = fri_plan_spec(OLA_FRI_MIN_SIZE, nullptr, 0);

    const vfy::Stage st = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, proof.data(), proof.size());
    CHECK(!st.host.failed(), "the host stage rejects the committed proof under MinSize(None): reason %u table %d", st.host.reason, st.host.table);
    size_t nt = 0;
    in >> word >> nt;
    CHECK(st.challenges.size() == nt, "tables");
    size_t want_merkle = 0, mixed = 0;
    for (size_t t = 0; t < nt; t++) {
        const vfy::Challenges none;
        const vfy::Challenges& c = t < st.challenges.size() ? st.challenges[t] : none;
        size_t k = 0;
        u64 x = 0, y = 0;
        in >> x >> y; CHECK(c.zeta.a == x && c.zeta.b == y, "table %zu: zeta", t);
        in >> x >> y; CHECK(c.fri_alpha.a == x && c.fri_alpha.b == y, "table %zu: fri_alpha", t);
        in >> k;
        CHECK(c.fri_betas.size() == k, "table %zu: %zu betas, recorded %zu", t, c.fri_betas.size(), k);
        for (size_t i = 0; i < k; i++) { in >> x >> y; CHECK(i < c.fri_betas.size() && c.fri_betas[i].a == x && c.fri_betas[i].b == y, "table %zu: beta %zu", t, i); }
        want_merkle += 28 * (3 + k);
        in >> x; CHECK(c.pow_response == x, "table %zu: proof-of-work response", t);
        in >> k;
        CHECK(c.query_indices.size() == k, "table %zu: query indices", t);
        for (size_t i = 0; i < k; i++) { in >> x; CHECK(i < c.query_indices.size() && c.query_indices[i] == x, "table %zu: query index %zu", t, i); }
    }
    if (!in) { fprintf(stderr, "bad case file\n"); exit(2); }
    CHECK(st.merkle.size() == want_merkle && st.queries.size() == 28 * nt, "job counts: %zu Merkle, %zu query", st.merkle.size(), st.queries.size());
    // every job points into the data; a query's layers lie one behind the other at their own widths, as the table's list says
    for (const vfy::MerkleJob& m : st.merkle)
        CHECK(m.leaf_off + m.leaf_len <= st.merkle_off && m.sib_off + 4 * (size_t)m.depth <= st.merkle_off && m.cap_off + 4 * (size_t)m.cap_len <= st.merkle_off, "a Merkle job out of bounds");
    for (const vfy::QueryJob& q : st.queries) {
        const u64* tab = st.image.data() + q.tab_off;
        const u64 layers = tab[vfy::TH_LAYERS], at = tab[vfy::TH_ARITIES_OFF];
        CHECK((int)layers == q.layers && at + layers <= st.merkle_off, "table %d: the list of arity bits", q.table);
        size_t off = q.steps_off, widths = 0;
        for (u64 i = 0; i < layers; i++) {
            const u64 ab = st.image[at + i];
            CHECK(ab >= 1 && ab <= (u64)vfy::MAX_ARITY_BITS, "table %d layer %zu: arity bits", q.table, (size_t)i);
            bool found = false;
            for (const vfy::MerkleJob& m : st.merkle)
                if (m.table == q.table && m.query == q.query && m.kind == 1 && m.which == (int)i) { found = m.leaf_off == off && m.leaf_len == (2u << ab); break; }
            CHECK(found, "table %d query %d layer %zu: the evaluations are not where the plan puts them", q.table, q.query, (size_t)i);
            off += (size_t)2 << ab;
            if (i && ab != st.image[at]) widths++;
        }
        CHECK(off <= st.merkle_off, "layer evaluations out of bounds");
        mixed += widths ? 1 : 0;
    }
    CHECK(mixed > 0, "no table of the proof has layers of two widths");
    {
        std::vector<uint32_t> flags(st.flags(), 0);
        CHECK(!vfy::resolve(st, flags.data()).failed(), "resolve with clear flags");
    }
    // the default strategy plans other layers: a shape refusal, not an error
    const vfy::Stage d = vfy::all_proof_stage(deflt, blob.data(), blob.size(), nullptr, proof.data(), proof.size());
    CHECK(d.host.failed() && d.host.reason >= OLA_VERIFY_SHAPE_CAP_HEIGHT && d.host.reason <= OLA_VERIFY_SHAPE_FINAL_POLY_LEN,
          "the default strategy on the MinSize proof: reason %u", d.host.reason);
}

int main(int argc, char** argv) {
    if (argc != 2 && argc != 3) { printf("usage: host_fri_plan_check PLANS [PROOF_CASE]\n"); return 2; }
    const size_t count = check_plans(argv[1]);
    check_refusals();
    if (argc == 3) check_proof(argv[2]);
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("%zu entries agree%s\n", count, argc == 3 ? ", the proof is accepted under its plan" : "");
    return 0;
}
