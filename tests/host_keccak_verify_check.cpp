// The verifier's host stage (olavm_amd/csrc/verify_host.h) on a proof with 25-byte digests, without a device: a stand-alone program
// that tests/test_keccak.py builds with g++ (a second time with -fsanitize=address,undefined) and runs on the committed Keccak proof
// with what the reference's verifier, interpreted from its source, recorded of it.  The case file is the one tests/test_verify_host.py
// writes for tests/host_verify_check.cpp (whose walker knows 32-byte digests only):
//   hasher H  proof PATH  blob N w...  ctl 4 words  tables T, per table the challenges  cases C, per case byte bit where reason table query kind which
// usage: host_keccak_verify_check CASES [STRIDE]     all checks under the file's hasher
//        host_keccak_verify_check CASES as H         only: does the host stage under hasher H accept the proof?  prints the verdict
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// the offsets of the length prefixes of an AllProof whose digests are `db` bytes, found with a walker of its own (not the product's reader)
struct Walker {
    const std::vector<uint8_t>& b; size_t db; size_t off = 0; std::vector<size_t> u32_at, u8_at;
    uint32_t len32() { u32_at.push_back(off); uint32_t x = 0; for (int i = 0; i < 4; i++) x |= (uint32_t)b.at(off + i) << (8 * i); off += 4; return x; }
    void vec(size_t each) { const uint32_t l = len32(); off += each * l; }
    void path() { u8_at.push_back(off); const uint8_t l = b.at(off); off += 1 + db * (size_t)l; }
    void all() {
        const uint32_t np = len32();
        for (uint32_t t = 0; t < np; t++) {
            for (int c = 0; c < 3; c++) vec(db);
            vec(16); vec(16); vec(16); vec(16); vec(8); vec(16);
            const uint32_t nc = len32();
            for (uint32_t i = 0; i < nc; i++) vec(db);
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
    if (argc < 2 || argc > 4) { printf("usage: host_keccak_verify_check CASES [STRIDE | as HASHER]\n"); return 2; }
    const bool as_other = argc == 4 && !strcmp(argv[2], "as");
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
    if (as_other) {
        cfg.hasher = (uint32_t)atoi(argv[3]);
        const vfy::Stage s = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, proof.data(), proof.size());
        printf("hasher %u: %s reason %u table %d\n", cfg.hasher, s.host.failed() ? "rejected" : "accepted", s.host.reason, s.host.table);
        return 0;
    }
    CHECK(cfg.hasher == OLA_HASH_KECCAK, "the case file is not of the Keccak configuration");

    // ---- the proof as it is: accepted, and every challenge of the record
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
    // every digest the stage kept is in the in-memory layout: word 3 holds byte 24 only
    for (const vfy::MerkleJob& m : st.merkle) {
        CHECK(m.leaf_off + m.leaf_len <= st.merkle_off && m.sib_off + 4 * (size_t)m.depth <= st.merkle_off && m.cap_off + 4 * (size_t)m.cap_len <= st.merkle_off, "a Merkle job out of bounds");
        for (size_t d = 0; d < m.depth; d++) CHECK(st.image[m.sib_off + 4 * d + 3] <= 0xFF, "a sibling's word 3 above one byte");
        for (size_t d = 0; d < m.cap_len; d++) CHECK(st.image[m.cap_off + 4 * d + 3] <= 0xFF, "a cap digest's word 3 above one byte");
    }
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

    // ---- malformed bytes: truncation at 2000 seeded lengths (and the empty proof), a trailing byte, every length prefix all ones
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
    Walker wk{proof, (size_t)KECCAK_DIGEST_BYTES, 0, {}, {}};
    wk.all();
    CHECK(wk.off == proof.size(), "the walker does not reach the end of the proof: digests are not 25 bytes");
    for (size_t k = 0; k < wk.u32_at.size(); k += stride) {
        const size_t at = wk.u32_at[k];
        std::vector<uint8_t> bad = proof;
        for (int i = 0; i < 4; i++) bad[at + (size_t)i] = 0xFF;
        const vfy::Stage s = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, bad.data(), bad.size());
        CHECK(s.host.reason == OLA_VERIFY_MALFORMED, "length prefix at %zu set to 0xFFFFFFFF: reason %u", at, s.host.reason);
    }
    for (size_t k = 0; k < wk.u8_at.size(); k += 7) {
        std::vector<uint8_t> bad = proof;
        bad[wk.u8_at[k]] = 0xFF;
        const vfy::Stage s = vfy::all_proof_stage(cfg, blob.data(), blob.size(), nullptr, bad.data(), bad.size());
        CHECK(s.host.failed(), "path length at %zu set to 0xFF is accepted", wk.u8_at[k]);
    }
    printf("host_keccak_verify_check: %zu length prefixes, %zu cases, %d failed\n", wk.u32_at.size() + wk.u8_at.size(), ncases, failures);
    return failures ? 1 : 0;
}
