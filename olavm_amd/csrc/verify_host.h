// Host stage of the verifier (ola_verify_all_proof / ola_verify_opening): everything of the reference's `verify_proof` that is
// sequential or small, in plain C++ (no HIP: this header compiles with g++ alone, tests/host_verify_check.cpp).
//
// Follows (reference paths relative to circuits/src/stark and plonky2/plonky2/src):
//   serialization.rs read_all_proof / read_proof / read_opening_set / read_fri_proof   -> Reader (bounds-checked, canonical words only)
//   get_challenges.rs:16-49,95-149, fri/challenges.rs:25-73                            -> the transcript replay (challenger_host.h)
//   verifier.rs:35-206   verify_proof: challenges, CtlCheckVars::from_proofs, per table verify_stark_proof_with_challenges,
//                        verify_cross_table_lookups last
//   verifier.rs:220-324  validate_proof_shape, eval_vanishing_poly over F_p[X]/(X^2 - 7) at zeta, the quotient identity
//   verifier.rs:381-388  eval_l_0_and_l_last
//   vanishing_poly.rs:20-45, permutation.rs:302-360, cross_table_lookup.rs:380-421,551-584
//   fri/validate_shape.rs:11-67, fri/verifier.rs:59-73 (proof of work)
// What is left for the device (verify.hip) is the bulk: one Merkle path per (table, query, oracle) and (table, query, layer), and the
// FRI algebra of every (table, query).  The host stage writes ONE flat u64 image that holds every word those checks read -- table
// headers, challenges, caps, opened rows, sibling lists, layer evaluations -- followed by the two job lists in structure-of-arrays
// form, so that a call is one upload, two launches and one read-back whatever the number of tables, queries and layers.
//
// Order of the verdict (the reference returns at the first failing check): tables in order; within a table shape, quotient
// identity, proof of work, then the queries in order; within a query the initial trees in oracle order, then per layer the
// consistency check before that layer's Merkle path, then the final polynomial; the lookup products last.  A host-level failure
// at table T therefore still needs the device's answer for the tables before T: the stage stops reading at T, keeps T's verdict,
// and resolve() reports the earliest device failure of the tables before it, if there is one.
//
// A field word >= p is refused as malformed: an honest serializer never writes one (serialization.rs:50-52 writes canonical
// words), and it lets the kernels assume canonical input.  Digest words of a Blake3 configuration are bytes and may be anything.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/ola_gpu.h"
#include "airset_host.h"
#include "challenger_host.h"
#include "fri_plan.h"
#include "gl.cuh"
#include "ola_error.h"

namespace ola {
namespace vfy {

struct Config {
    int rate_bits = 3, cap_height = 4, pow_bits = 16, arity_bits = 4, final_poly_bits = 5, num_queries = 28, num_challenges = 2;
    uint32_t hasher = OLA_HASH_POSEIDON;
    FriPlanSpec plan;      // FriReductionStrategy; the default is ConstantArityBits(arity_bits, final_poly_bits)
};
inline Config config_of(const OlaGpuConfig& c, const FriPlanSpec& plan = FriPlanSpec()) {
    Config v;
    v.plan = plan;
    v.rate_bits = (int)c.rate_bits; v.cap_height = (int)c.cap_height; v.pow_bits = (int)c.proof_of_work_bits; v.arity_bits = (int)c.fri_arity_bits;
    v.final_poly_bits = (int)c.fri_final_poly_bits; v.num_queries = (int)c.num_query_rounds; v.num_challenges = (int)c.num_challenges;
    v.hasher = c.hasher;
    return v;
}
// the kernels keep one coset of a layer in registers
enum { MAX_ARITY_BITS = 4, MAX_LDE_BITS = 32 };

// ------------------------------------------------------------------------------------------------ wire format
typedef std::array<u64, 4> Digest;
struct WStep { std::vector<u64> evals; std::vector<Digest> path; };                       // evals: (a, b) pairs, as the leaf is hashed
struct WInitial { std::vector<u64> row; std::vector<Digest> path; };
struct WQuery { std::vector<WInitial> initial; std::vector<WStep> steps; };
struct WFri { std::vector<std::vector<Digest>> commit_caps; std::vector<WQuery> queries; std::vector<u64> final_poly; u64 pow_witness = 0; };
struct WOpenings { std::vector<u64> local, next, zs, zs_next, ctl_last, quotient; };     // extension vectors as (a, b) pairs; ctl_last is base
struct WProof { std::vector<Digest> trace_cap, zs_cap, quotient_cap; WOpenings op; WFri fri; };

// Every length prefix is checked against the bytes that are left BEFORE anything is allocated for it.
struct Reader {
    const uint8_t* p; size_t n, off = 0; bool ok = true; int digest_bytes;   // digest_wire_bytes: 32 (Blake3) or 25 (Keccak) bytes, never reduced; 0: four field words
    Reader(const uint8_t* bytes, size_t len, uint32_t hasher) : p(bytes), n(len), digest_bytes(digest_wire_bytes(hasher)) {}
    size_t left() const { return n - off; }
    bool need(size_t count, size_t each) {
        if (!ok) return false;
        if (each != 0 && count > left() / each) { ok = false; return false; }
        return true;
    }
    uint8_t u8() { if (!need(1, 1)) return 0; return p[off++]; }
    uint32_t u32() { if (!need(1, 4)) return 0; uint32_t x = 0; for (int i = 0; i < 4; i++) x |= (uint32_t)p[off + i] << (8 * i); off += 4; return x; }
    u64 raw64() { if (!need(1, 8)) return 0; u64 x = 0; for (int i = 0; i < 8; i++) x |= (u64)p[off + i] << (8 * i); off += 8; return x; }
    u64 field() { const u64 x = raw64(); if (x >= GL_P) ok = false; return x; }
    void words(std::vector<u64>& v, size_t count) { if (!need(count, 8)) return; v.reserve(count); for (size_t i = 0; i < count && ok; i++) v.push_back(field()); }
    void field_vec(std::vector<u64>& v) { const uint32_t l = u32(); words(v, l); }
    void ext_vec(std::vector<u64>& v) { const uint32_t l = u32(); if (!need(l, 16)) return; words(v, 2 * (size_t)l); }
    Digest digest() {
        Digest h = {0, 0, 0, 0};
        if (digest_bytes == KECCAK_DIGEST_BYTES) { for (int i = 0; i < 3; i++) h[i] = raw64(); h[3] = u8(); return h; }   // the in-memory layout: word 3 is byte 24
        for (int i = 0; i < 4; i++) h[i] = digest_bytes ? raw64() : field();
        return h;
    }
    void digests(std::vector<Digest>& v, size_t count) { if (!need(count, digest_bytes ? (size_t)digest_bytes : 32)) return; v.reserve(count); for (size_t i = 0; i < count && ok; i++) v.push_back(digest()); }
    void cap(std::vector<Digest>& v) { const uint32_t l = u32(); digests(v, l); }
    void merkle_proof(std::vector<Digest>& v) { const uint8_t l = u8(); digests(v, l); }
    void opening_set(WOpenings& o) {
        ext_vec(o.local); ext_vec(o.next); ext_vec(o.zs); ext_vec(o.zs_next); field_vec(o.ctl_last); ext_vec(o.quotient);
    }
    void fri_proof(WFri& f) {
        const uint32_t nc = u32();
        if (!need(nc, 4)) return;
        f.commit_caps.resize(nc);
        for (uint32_t i = 0; i < nc && ok; i++) cap(f.commit_caps[i]);
        const uint32_t nq = u32();
        if (!need(nq, 8)) return;                     // a query is at least its two counts
        f.queries.resize(nq);
        for (uint32_t q = 0; q < nq && ok; q++) {
            WQuery& r = f.queries[q];
            const uint32_t ni = u32();
            if (!need(ni, 5)) return;                 // a row count and a path length
            r.initial.resize(ni);
            for (uint32_t i = 0; i < ni && ok; i++) { field_vec(r.initial[i].row); merkle_proof(r.initial[i].path); }
            const uint32_t ns = u32();
            if (!need(ns, 5)) return;
            r.steps.resize(ns);
            for (uint32_t i = 0; i < ns && ok; i++) { ext_vec(r.steps[i].evals); merkle_proof(r.steps[i].path); }
        }
        ext_vec(f.final_poly);
        f.pow_witness = field();
    }
    void proof(WProof& s) { cap(s.trace_cap); cap(s.zs_cap); cap(s.quotient_cap); opening_set(s.op); fri_proof(s.fri); }
};
enum { MIN_PROOF_BYTES = 3 * 4 + 6 * 4 + 4 + 4 + 4 + 8 };   // three caps, six opening vectors, cap / query / final-polynomial counts, the witness

// ------------------------------------------------------------------------------------------------ verdicts
struct Verdict {
    uint32_t reason = OLA_VERIFY_OK;
    int table = -1, query = -1, oracle_or_layer = -1;
    const char* words = nullptr;      // the oracle's words where one reason has several (malformed bytes / wrong table count)
    bool failed() const { return reason != OLA_VERIFY_OK; }
};
// the oracle's words for a reason (oracle/stark.cpp:456-529, oracle/fri.cpp:250-323)
inline const char* reason_text(uint32_t r) {
    switch (r) {
        case OLA_VERIFY_OK: return "";
        case OLA_VERIFY_MALFORMED: return "malformed proof bytes";
        case OLA_VERIFY_EMPTY_FRI: return "empty FRI proof";
        case OLA_VERIFY_SHAPE_OPENING_WIDTH: return "opening width";
        case OLA_VERIFY_SHAPE_ZS_WIDTH: return "zs width";
        case OLA_VERIFY_SHAPE_CTL_ZS_LAST_WIDTH: return "ctl_zs_last width";
        case OLA_VERIFY_SHAPE_QUOTIENT_WIDTH: return "quotient width";
        case OLA_VERIFY_QUOTIENT_IDENTITY: return "Mismatch between evaluation and opening of quotient polynomial";
        case OLA_VERIFY_SHAPE_CAP_HEIGHT: return "cap height";
        case OLA_VERIFY_SHAPE_QUERY_ROUNDS: return "number of query rounds";
        case OLA_VERIFY_SHAPE_INITIAL_PROOFS: return "initial proofs";
        case OLA_VERIFY_SHAPE_LEAF_LEN: return "leaf len";
        case OLA_VERIFY_SHAPE_INITIAL_PATH_LEN: return "initial merkle proof len";
        case OLA_VERIFY_SHAPE_STEPS: return "steps";
        case OLA_VERIFY_SHAPE_EVALS_LEN: return "evals len";
        case OLA_VERIFY_SHAPE_STEP_PATH_LEN: return "step merkle proof len";
        case OLA_VERIFY_SHAPE_FINAL_POLY_LEN: return "final poly len";
        case OLA_VERIFY_POW: return "Invalid proof of work witness.";
        case OLA_VERIFY_MERKLE_INITIAL: return "Invalid Merkle proof (initial tree).";
        case OLA_VERIFY_FRI_CONSISTENCY: return "FRI consistency check failed";
        case OLA_VERIFY_MERKLE_COMMIT: return "Invalid Merkle proof (commit phase).";
        case OLA_VERIFY_FINAL_POLY: return "Final polynomial evaluation is invalid.";
        case OLA_VERIFY_CTL: return "Cross-table lookup verification failed.";
        default: return "unknown reason";
    }
}

// ------------------------------------------------------------------------------------------------ the image and the job lists
// Table header, TAB_WORDS words at tab_off (all offsets are word offsets into the image):
enum {
    TH_LDE_BITS = 0, TH_LAYERS, TH_ARITIES_OFF /* `layers` words: each layer's arity bits */, TH_FINAL_OFF, TH_FINAL_LEN, TH_ALPHA /* 2 */, TH_BETAS_OFF = 7, TH_N0, TH_N1, TH_N2, TH_NPERM,
    TH_ZETA /* 2 */, TH_ZETA_NEXT = 14 /* 2 */, TH_G_INV = 16, TH_REDUCED = 17 /* 3 x 2: reduced openings per batch */,
    TH_ALPHA_POW = 23 /* 3 x 2: alpha^(batch length) */, TAB_WORDS = 32
};
// Merkle job, MJ_WORDS words; job j's word k sits at merkle_off + k * n_merkle + j (a wave reads consecutive addresses)
enum { MJ_LEAF_OFF = 0, MJ_SIB_OFF, MJ_CAP_OFF, MJ_LEN_DEPTH /* leaf_len | depth << 32 */, MJ_INDEX, MJ_CAP_LEN, MJ_WORDS };
// query job, QJ_WORDS words, the same arrangement at query_off
enum { QJ_TAB_OFF = 0, QJ_X_INDEX, QJ_ROW0, QJ_ROW1, QJ_ROW2, QJ_STEPS_OFF, QJ_WORDS };
// flags the kernels write: one u32 per Merkle job, then one per query job
enum { MF_OK = 0, MF_MISMATCH = 1, MF_BOUNDS = 2 };
enum { QF_OK = 0, QF_CONSISTENCY = 1, QF_FINAL_POLY = 2, QF_BOUNDS = 3 };   // kind | layer << 8

struct MerkleJob {
    u64 leaf_off = 0, sib_off = 0, cap_off = 0, index = 0;
    uint32_t leaf_len = 0, depth = 0, cap_len = 0;
    int table = 0, query = 0, kind = 0 /* 0 initial tree, 1 commit phase */, which = 0 /* oracle or layer */;
};
struct QueryJob { u64 tab_off = 0, x_index = 0, row_off[3] = {0, 0, 0}, steps_off = 0; int table = 0, query = 0, layers = 0; };

struct Challenges {          // of one table, as get_challenges.rs derives them (kept for the tests)
    std::vector<u64> perm;   // (beta, gamma) pairs, permutation_batch_size x num_challenges
    std::vector<u64> alphas;
    Ext2 zeta = {0, 0}, fri_alpha = {0, 0};
    std::vector<Ext2> fri_betas;
    u64 pow_response = 0;
    std::vector<u64> query_indices;
};

struct Stage {
    std::vector<u64> image;
    std::vector<MerkleJob> merkle;     // sorted by (leaf length, depth) by pack()
    std::vector<QueryJob> queries;
    size_t merkle_off = 0, query_off = 0;   // set by pack()
    Verdict host;                      // the first failure the host stage met (reason OK: none)
    std::vector<u64> ctl_challenges;   // (beta, gamma) x num_challenges (all-proof only)
    std::vector<Challenges> challenges;
    OlaChallenger transcript;          // after the last table read
    size_t flags() const { return merkle.size() + queries.size(); }
};

inline Ext2 ext_from(u64 x) { return ext_make(x, 0); }
inline Ext2 ext_at(const std::vector<u64>& v, size_t i) { return ext_make(v[2 * i], v[2 * i + 1]); }

// fri/reduction_strategies.rs:30-57 under the configuration's strategy: the arity bits of every layer (fri_plan.h)
inline std::vector<int> fri_layers(const Config& c, int degree_bits) {
    return fri_plan_arity_bits(c.plan, c.arity_bits, c.final_poly_bits, degree_bits, c.rate_bits, c.cap_height, (size_t)c.num_queries);
}

// fri/challenges.rs:25-73
inline void fri_challenges(OlaChallenger& ch, const Config& cfg, const WFri& fri, int degree_bits, Challenges& out) {
    out.fri_alpha = challenger_get_ext(ch);
    for (const auto& cap : fri.commit_caps) {
        challenger_observe_cap(ch, cap.empty() ? nullptr : cap[0].data(), cap.size());
        out.fri_betas.push_back(challenger_get_ext(ch));
    }
    challenger_observe(ch, fri.final_poly.data(), fri.final_poly.size());
    u64 s[12] = {0};
    for (int i = 0; i < 4; i++) s[i] = challenger_get(ch);
    s[4] = fri.pow_witness;
    // C::InnerHasher::hash_no_pad of five elements is one permutation of the InnerHasher (a sponge in every configuration)
    hasher_row(hasher_row(cfg.hasher).inner).permute(s);
    out.pow_response = s[0];
    const u64 lde_size = (u64)1 << (degree_bits + cfg.rate_bits);
    for (int i = 0; i < cfg.num_queries; i++) out.query_indices.push_back(challenger_get(ch) % lde_size);
}

inline size_t push_words(std::vector<u64>& image, const u64* w, size_t n) {
    const size_t at = image.size();
    image.insert(image.end(), w, w + n);
    return at;
}
inline size_t push_digests(std::vector<u64>& image, const std::vector<Digest>& d) {
    const size_t at = image.size();
    for (const Digest& h : d) image.insert(image.end(), h.begin(), h.end());
    return at;
}

// plonky2's verify_fri_proof up to the queries (shape, proof of work), and the table's share of the image and of the job lists.
// caps: the three initial caps; num_polys: what the instance expects of the three oracles; openings as the prover observed them.
inline Verdict fri_stage(Stage& st, const Config& cfg, int table, const std::vector<Digest>* const caps[3], const int num_polys[3],
                         int num_permutation_zs, int degree_bits, Ext2 zeta, const WOpenings& op, const WFri& fri, const Challenges& fc) {
    Verdict v;
    v.table = table;
    auto fail = [&](uint32_t reason, int query = -1, int which = -1) { v.reason = reason; v.query = query; v.oracle_or_layer = which; return v; };
    const std::vector<int> arities = fri_layers(cfg, degree_bits);
    const int lde_bits = degree_bits + cfg.rate_bits, layers = (int)arities.size();
    if (layers > 64) throw OlaError(OLA_E_INVALID_ARG, "the verifier supports FRI plans of at most 64 layers");
    int total_bits = 0;
    for (int a : arities) {
        if (a < 1 || a > MAX_ARITY_BITS) throw OlaError(OLA_E_INVALID_ARG, "the verifier supports FRI arities of 2 to 16");
        total_bits += a;
    }
    const size_t cap_len = (size_t)1 << cfg.cap_height;
    // validate_fri_proof_shape
    for (size_t i = 0; i < fri.commit_caps.size(); i++)
        if (fri.commit_caps[i].size() != cap_len) return fail(OLA_VERIFY_SHAPE_CAP_HEIGHT, -1, (int)i);
    if ((int)fri.queries.size() != cfg.num_queries) return fail(OLA_VERIFY_SHAPE_QUERY_ROUNDS);
    for (size_t r = 0; r < fri.queries.size(); r++) {
        const WQuery& q = fri.queries[r];
        if (q.initial.size() != 3) return fail(OLA_VERIFY_SHAPE_INITIAL_PROOFS, (int)r);
        for (int o = 0; o < 3; o++) {
            if ((int)q.initial[o].row.size() != num_polys[o]) return fail(OLA_VERIFY_SHAPE_LEAF_LEN, (int)r, o);
            if ((int)q.initial[o].path.size() + cfg.cap_height != lde_bits) return fail(OLA_VERIFY_SHAPE_INITIAL_PATH_LEN, (int)r, o);
        }
        if ((int)q.steps.size() != layers) return fail(OLA_VERIFY_SHAPE_STEPS, (int)r);
        int bits = lde_bits;
        for (int i = 0; i < layers; i++) {
            bits -= arities[(size_t)i];
            if (q.steps[i].evals.size() != ((size_t)2 << arities[(size_t)i])) return fail(OLA_VERIFY_SHAPE_EVALS_LEN, (int)r, i);
            if ((int)q.steps[i].path.size() + cfg.cap_height != bits) return fail(OLA_VERIFY_SHAPE_STEP_PATH_LEN, (int)r, i);
        }
    }
    // a plan that does not fit the table is the caller's configuration, not the proof's fault (as in the prover)
    if (!fri_plan_fits(arities, degree_bits, cfg.rate_bits, cfg.cap_height)) throw OlaError(OLA_E_INVALID_ARG, "FRI total reduction arity is too large.");
    if (fri.final_poly.size() != 2 * ((size_t)1 << (degree_bits - total_bits))) return fail(OLA_VERIFY_SHAPE_FINAL_POLY_LEN);
    if (cfg.pow_bits > 0 && (fc.pow_response >> (64 - cfg.pow_bits)) != 0) return fail(OLA_VERIFY_POW);
    // one beta was drawn per commit cap, one is used per layer: with caps to spare the transcript is not the prover's (the proof of
    // work has just caught that, up to 2^-pow_bits), with too few there is no beta to fold by
    if ((int)fri.commit_caps.size() != layers) return fail(OLA_VERIFY_SHAPE_STEPS);

    // ---- the table's header
    std::vector<u64>& im = st.image;
    const size_t tab_off = im.size();
    im.resize(tab_off + TAB_WORDS, 0);
    const u64 g = gl_root_of_unity(degree_bits);
    const Ext2 zeta_next = ext_scalar_mul(zeta, g);
    // to_fri_openings (proof.rs:235-265): [local, zs, quotient] at zeta, [next, zs_next] at g zeta, [ctl_zs_last] at g^-1
    auto reduce = [&](std::initializer_list<const std::vector<u64>*> parts, bool base) {
        std::vector<Ext2> all;
        for (const std::vector<u64>* p : parts) {
            if (base) for (u64 x : *p) all.push_back(ext_from(x));
            else for (size_t i = 0; i < p->size() / 2; i++) all.push_back(ext_at(*p, i));
        }
        Ext2 acc = ext_make(0, 0);
        for (size_t i = all.size(); i-- > 0;) acc = ext_add(ext_mul(acc, fc.fri_alpha), all[i]);
        return acc;
    };
    const Ext2 red[3] = {reduce({&op.local, &op.zs, &op.quotient}, false), reduce({&op.next, &op.zs_next}, false), reduce({&op.ctl_last}, true)};
    // the device reduces the opened ROWS batch by batch: n0 + n1 + n2, n0 + n1 and n1 - num_permutation_zs values
    const size_t row_len[3] = {(size_t)num_polys[0] + num_polys[1] + num_polys[2], (size_t)num_polys[0] + num_polys[1],
                               (size_t)(num_polys[1] - num_permutation_zs)};
    {
        u64* h = im.data() + tab_off;
        h[TH_LDE_BITS] = (u64)lde_bits; h[TH_LAYERS] = (u64)layers;
        h[TH_FINAL_LEN] = fri.final_poly.size() / 2;
        h[TH_ALPHA] = fc.fri_alpha.a; h[TH_ALPHA + 1] = fc.fri_alpha.b;
        h[TH_N0] = (u64)num_polys[0]; h[TH_N1] = (u64)num_polys[1]; h[TH_N2] = (u64)num_polys[2]; h[TH_NPERM] = (u64)num_permutation_zs;
        h[TH_ZETA] = zeta.a; h[TH_ZETA + 1] = zeta.b; h[TH_ZETA_NEXT] = zeta_next.a; h[TH_ZETA_NEXT + 1] = zeta_next.b;
        h[TH_G_INV] = gl_inv(g);
        for (int b = 0; b < 3; b++) {
            h[TH_REDUCED + 2 * b] = red[b].a; h[TH_REDUCED + 2 * b + 1] = red[b].b;
            const Ext2 ap = ext_pow(fc.fri_alpha, (u64)row_len[b]);
            h[TH_ALPHA_POW + 2 * b] = ap.a; h[TH_ALPHA_POW + 2 * b + 1] = ap.b;
        }
    }
    {
        const size_t betas_off = im.size();
        for (const Ext2& b : fc.fri_betas) { im.push_back(b.a); im.push_back(b.b); }
        const size_t arities_off = im.size();
        for (int a : arities) im.push_back((u64)a);
        const size_t final_off = push_words(im, fri.final_poly.data(), fri.final_poly.size());
        im[tab_off + TH_BETAS_OFF] = betas_off; im[tab_off + TH_ARITIES_OFF] = arities_off; im[tab_off + TH_FINAL_OFF] = final_off;
    }
    size_t cap_off[3], commit_cap_off[64];
    for (int o = 0; o < 3; o++) cap_off[o] = push_digests(im, *caps[o]);
    for (int i = 0; i < layers; i++) commit_cap_off[i] = push_digests(im, fri.commit_caps[i]);
    // ---- the queries: rows, layer evaluations (contiguous, each layer at its own width 2 * 2^arity_bits), sibling lists
    for (size_t r = 0; r < fri.queries.size(); r++) {
        const WQuery& q = fri.queries[r];
        QueryJob qj;
        qj.tab_off = tab_off; qj.x_index = fc.query_indices[r]; qj.table = table; qj.query = (int)r; qj.layers = layers;
        for (int o = 0; o < 3; o++) qj.row_off[o] = push_words(im, q.initial[o].row.data(), q.initial[o].row.size());
        qj.steps_off = im.size();
        for (int i = 0; i < layers; i++) push_words(im, q.steps[i].evals.data(), q.steps[i].evals.size());
        u64 x_index = qj.x_index;
        for (int o = 0; o < 3; o++) {
            MerkleJob m;
            m.leaf_off = qj.row_off[o]; m.leaf_len = (uint32_t)num_polys[o]; m.sib_off = push_digests(im, q.initial[o].path);
            m.depth = (uint32_t)q.initial[o].path.size(); m.cap_off = cap_off[o]; m.cap_len = (uint32_t)caps[o]->size(); m.index = x_index;
            m.table = table; m.query = (int)r; m.kind = 0; m.which = o;
            st.merkle.push_back(m);
        }
        size_t step_off = qj.steps_off;
        for (int i = 0; i < layers; i++) {
            const size_t width = (size_t)2 << arities[(size_t)i];
            x_index >>= arities[(size_t)i];
            MerkleJob m;
            m.leaf_off = step_off; m.leaf_len = (uint32_t)width;
            step_off += width; m.sib_off = push_digests(im, q.steps[i].path);
            m.depth = (uint32_t)q.steps[i].path.size(); m.cap_off = commit_cap_off[i]; m.cap_len = (uint32_t)cap_len; m.index = x_index;
            m.table = table; m.query = (int)r; m.kind = 1; m.which = i;
            st.merkle.push_back(m);
        }
        st.queries.push_back(qj);
    }
    return Verdict();
}

// The job lists behind the data, structure of arrays; Merkle jobs ordered so that a wave's jobs share leaf length and depth.
inline void pack(Stage& st) {
    std::stable_sort(st.merkle.begin(), st.merkle.end(), [](const MerkleJob& a, const MerkleJob& b) {
        return a.leaf_len != b.leaf_len ? a.leaf_len < b.leaf_len : a.depth < b.depth;
    });
    std::vector<u64>& im = st.image;
    const size_t nm = st.merkle.size(), nq = st.queries.size();
    st.merkle_off = im.size();
    im.resize(im.size() + MJ_WORDS * nm, 0);
    for (size_t j = 0; j < nm; j++) {
        const MerkleJob& m = st.merkle[j];
        u64* w = im.data() + st.merkle_off + j;
        w[MJ_LEAF_OFF * nm] = m.leaf_off; w[MJ_SIB_OFF * nm] = m.sib_off; w[MJ_CAP_OFF * nm] = m.cap_off;
        w[MJ_LEN_DEPTH * nm] = (u64)m.leaf_len | ((u64)m.depth << 32); w[MJ_INDEX * nm] = m.index; w[MJ_CAP_LEN * nm] = m.cap_len;
    }
    st.query_off = im.size();
    im.resize(im.size() + QJ_WORDS * nq, 0);
    for (size_t j = 0; j < nq; j++) {
        const QueryJob& q = st.queries[j];
        u64* w = im.data() + st.query_off + j;
        w[QJ_TAB_OFF * nq] = q.tab_off; w[QJ_X_INDEX * nq] = q.x_index; w[QJ_ROW0 * nq] = q.row_off[0]; w[QJ_ROW1 * nq] = q.row_off[1];
        w[QJ_ROW2 * nq] = q.row_off[2]; w[QJ_STEPS_OFF * nq] = q.steps_off;
    }
}

// The final verdict from the host stage's own and the flags the kernels wrote (flags: merkle.size() + queries.size() words).
inline Verdict resolve(const Stage& st, const uint32_t* flags) {
    // position of a check within the proof: (table, query, stage); stage = oracle 0..2, 3 + 2 layer (consistency), 4 + 2 layer (path),
    // 3 + 2 layers (final polynomial)
    bool found = false;
    long best[3] = {0, 0, 0};
    Verdict v;
    auto consider = [&](long table, long query, long stage, uint32_t reason, int which) {
        const long key[3] = {table, query, stage};
        if (found && !std::lexicographical_compare(key, key + 3, best, best + 3)) return;
        found = true;
        std::copy(key, key + 3, best);
        v.reason = reason; v.table = (int)table; v.query = (int)query; v.oracle_or_layer = which;
    };
    for (size_t j = 0; j < st.merkle.size(); j++) {
        const MerkleJob& m = st.merkle[j];
        if (flags[j] == MF_OK) continue;
        if (flags[j] != MF_MISMATCH) throw OlaError(OLA_E_INTERNAL, "verifier: a Merkle job points outside the image");
        if (m.kind == 0) consider(m.table, m.query, m.which, OLA_VERIFY_MERKLE_INITIAL, m.which);
        else consider(m.table, m.query, 4 + 2 * m.which, OLA_VERIFY_MERKLE_COMMIT, m.which);
    }
    for (size_t j = 0; j < st.queries.size(); j++) {
        const QueryJob& q = st.queries[j];
        const uint32_t f = flags[st.merkle.size() + j], kind = f & 0xff;
        const int layer = (int)(f >> 8);
        if (kind == QF_OK) continue;
        if (kind == QF_CONSISTENCY && layer < q.layers) consider(q.table, q.query, 3 + 2 * layer, OLA_VERIFY_FRI_CONSISTENCY, layer);
        else if (kind == QF_FINAL_POLY) consider(q.table, q.query, 3 + 2 * q.layers, OLA_VERIFY_FINAL_POLY, -1);
        else throw OlaError(OLA_E_INTERNAL, "verifier: a query job points outside the image");
    }
    return found ? v : st.host;
}

inline void describe(const Verdict& v, char* out, size_t cap) {
    if (!v.failed()) { snprintf(out, cap, "accepted"); return; }
    char where[64] = "";
    size_t k = 0;
    if (v.table >= 0) k += (size_t)snprintf(where + k, sizeof(where) - k, " table %d", v.table);
    if (v.query >= 0) k += (size_t)snprintf(where + k, sizeof(where) - k, " query %d", v.query);
    if (v.oracle_or_layer >= 0)
        k += (size_t)snprintf(where + k, sizeof(where) - k, " %s %d", v.reason == OLA_VERIFY_MERKLE_INITIAL || v.reason == OLA_VERIFY_SHAPE_LEAF_LEN || v.reason == OLA_VERIFY_SHAPE_INITIAL_PATH_LEN ? "oracle" : "layer", v.oracle_or_layer);
    snprintf(out, cap, "%s%s%s%s", v.words ? v.words : reason_text(v.reason), k ? " [" : "", k ? where + 1 : "", k ? "]" : "");
}

// ------------------------------------------------------------------------------------------------ the constraint program at zeta
// ConstraintConsumer (constraint_consumer.rs:34-78) over the extension field
struct Consumer {
    std::vector<Ext2> alphas, accs;
    Ext2 z_last, lagrange_first, lagrange_last;
    void emit(int kind, Ext2 c) {
        if (kind == AK_TRANSITION) c = ext_mul(c, z_last);
        else if (kind == AK_FIRST) c = ext_mul(c, lagrange_first);
        else if (kind == AK_LAST) c = ext_mul(c, lagrange_last);
        for (size_t i = 0; i < alphas.size(); i++) accs[i] = ext_add(ext_mul(accs[i], alphas[i]), c);
    }
};
struct GpChallenge { u64 beta, gamma; };
struct CtlVar { GpChallenge ch; const HTwc* twc; };

inline Ext2 eval_lincol(const HLinCol& c, const std::vector<u64>& v) {
    Ext2 s = ext_make(0, 0);
    for (const auto& t : c.terms) {
        s = ext_add(s, ext_scalar_mul(ext_at(v, (size_t)t.first), gl_canon(t.second)));
    }
    return ext_add(s, ext_from(gl_canon(c.constant)));
}

// eval_vanishing_poly (vanishing_poly.rs:20-45): the table's constraint program, the permutation checks, the lookup checks
inline void eval_vanishing_poly(const HTable& air, int num_challenges, const WOpenings& op, const u64* params, const std::vector<u64>& perm_challenges,
                                const std::vector<CtlVar>& ctl_vars, Consumer& consumer) {
    const Ext2 zero = ext_make(0, 0), one = ext_make(1, 0);
    std::vector<Ext2> reg((size_t)air.n_regs, zero);
    for (size_t i = 0; i + 1 < air.ops.size(); i += 2) {
        const AirOp o = air_op(air.ops[i], air.ops[i + 1]);      // validated by parse_airset: what it names exists
        switch (o.op) {
            case AOP_LOCAL: reg[o.dst] = ext_at(op.local, o.a); break;
            case AOP_NEXT: reg[o.dst] = ext_at(op.next, o.a); break;
            case AOP_CONST: reg[o.dst] = ext_from(gl_canon(o.imm)); break;
            case AOP_PARAM: reg[o.dst] = ext_from(gl_canon(params[o.a])); break;
            case AOP_ADD: reg[o.dst] = ext_add(reg[o.a], reg[o.b]); break;
            case AOP_SUB: reg[o.dst] = ext_sub(reg[o.a], reg[o.b]); break;
            case AOP_MUL: reg[o.dst] = ext_mul(reg[o.a], reg[o.b]); break;
            case AOP_EMIT: consumer.emit(o.kind, reg[o.a]); break;
            case AOP_ISZERO: reg[o.dst] = (reg[o.a].a == 0 && reg[o.a].b == 0) ? one : zero; break;
        }
    }
    const int nperm = air.num_permutation_batches(num_challenges);
    if (nperm > 0) {
        for (int i = 0; i < nperm; i++) consumer.emit(AK_FIRST, ext_sub(ext_at(op.zs, (size_t)i), one));
        // get_permutation_batches: (pair, challenge) instances chunked by the batch size; instance i of a chunk takes challenge set i
        const int bs = air.permutation_batch_size(), total = (int)air.perm_pairs.size() * num_challenges;
        int inst = 0;
        for (int b = 0; b < nperm; b++) {
            Ext2 prod_l = one, prod_r = one;
            for (int i = 0; i < bs && inst < total; i++, inst++) {
                const auto& pair = air.perm_pairs[(size_t)(inst / num_challenges)];
                const u64* ch = perm_challenges.data() + 2 * ((size_t)i * num_challenges + (size_t)(inst % num_challenges));
                Ext2 l = zero, r = zero;
                for (size_t k = pair.size(); k-- > 0;) {
                    l = ext_add(ext_scalar_mul(l, ch[0]), ext_at(op.local, (size_t)pair[k].first));
                    r = ext_add(ext_scalar_mul(r, ch[0]), ext_at(op.local, (size_t)pair[k].second));
                }
                prod_l = ext_mul(prod_l, ext_add(l, ext_from(ch[1])));
                prod_r = ext_mul(prod_r, ext_add(r, ext_from(ch[1])));
            }
            consumer.emit(AK_ALL, ext_sub(ext_mul(ext_at(op.zs_next, (size_t)b), prod_r), ext_mul(ext_at(op.zs, (size_t)b), prod_l)));
        }
    }
    for (size_t i = 0; i < ctl_vars.size(); i++) {
        const GpChallenge ch = ctl_vars[i].ch;
        const HTwc& twc = *ctl_vars[i].twc;
        auto combine = [&](const std::vector<u64>& v) {
            Ext2 acc = zero;
            for (size_t k = twc.columns.size(); k-- > 0;) acc = ext_add(ext_scalar_mul(acc, ch.beta), eval_lincol(twc.columns[k], v));
            return ext_add(acc, ext_from(ch.gamma));
        };
        auto filter = [&](const std::vector<u64>& v) { return twc.has_filter ? eval_lincol(twc.filter, v) : one; };
        auto select = [&](Ext2 f, Ext2 x) { return ext_sub(ext_add(ext_mul(f, x), one), f); };
        const Ext2 lz = ext_at(op.zs, (size_t)nperm + i), nz = ext_at(op.zs_next, (size_t)nperm + i);
        consumer.emit(AK_FIRST, ext_sub(lz, select(filter(op.local), combine(op.local))));
        consumer.emit(AK_TRANSITION, ext_sub(nz, ext_mul(lz, select(filter(op.next), combine(op.next)))));
    }
}

inline void observe_openings(OlaChallenger& ch, const WOpenings& op) {
    // observe_openings(&openings.to_fri_openings()) (fri/challenges.rs:16-23): batch by batch, ctl_zs_last as extension elements
    for (const std::vector<u64>* v : {&op.local, &op.zs, &op.quotient, &op.next, &op.zs_next}) challenger_observe(ch, v->data(), v->size());
    for (u64 x : op.ctl_last) { const u64 e[2] = {x, 0}; challenger_observe(ch, e, 2); }
}

inline void require_config(const Config& cfg) {
    if (cfg.plan.strategy == OLA_FRI_CONSTANT_ARITY_BITS && (cfg.arity_bits < 1 || cfg.arity_bits > MAX_ARITY_BITS))
        throw OlaError(OLA_E_INVALID_ARG, "the verifier supports FRI arities of 2 to 16");
    if (fri_plan_spec_check(cfg.plan.strategy, cfg.plan.args, cfg.plan.n)) throw OlaError(OLA_E_INVALID_ARG, "the FRI reduction strategy is malformed");
    if (cfg.rate_bits < 1 || cfg.rate_bits > 8 || cfg.cap_height < 0 || cfg.cap_height > 16 || cfg.pow_bits < 0 || cfg.pow_bits > 40 ||
        cfg.num_queries < 1 || cfg.num_queries > 1024 || cfg.num_challenges < 1 || cfg.num_challenges > 8 || cfg.final_poly_bits < 0)
        throw OlaError(OLA_E_INVALID_ARG, "configuration out of range for the verifier");
}

// degree_bits as the reference's verifier derives it: from the length of the first query's first Merkle path (verifier.rs:60-66)
inline bool degree_bits_of(const Config& cfg, const WFri& fri, int& degree_bits) {
    if (fri.queries.empty() || fri.queries[0].initial.empty()) return false;
    degree_bits = cfg.cap_height + (int)fri.queries[0].initial[0].path.size() - cfg.rate_bits;
    return true;
}

// ------------------------------------------------------------------------------------------------ verify_proof, host stage
// params: concatenated per-table parameters as for ola_prove_with_traces, or NULL: every parameter of table t is then the proof's
// compress_challenges[t], as the reference's verifier takes them (verifier.rs:75-92).
inline Stage all_proof_stage(const Config& cfg, const u64* airset, size_t airset_words, const u64* params, const uint8_t* bytes, size_t len) {
    require_config(cfg);
    const HAirSet set = parse_airset(airset, airset_words);
    const size_t nt = set.tables.size();
    Stage st;
    challenger_init(st.transcript, cfg.hasher);
    auto fail = [&](uint32_t reason, int table = -1) { st.host.reason = reason; st.host.table = table; pack(st); return st; };

    Reader r(bytes, len, cfg.hasher);
    const uint32_t np = r.u32();
    if (!r.need(np, MIN_PROOF_BYTES)) return fail(OLA_VERIFY_MALFORMED);
    std::vector<WProof> proofs(np);
    for (uint32_t i = 0; i < np && r.ok; i++) r.proof(proofs[i]);
    std::vector<u64> compress;
    r.field_vec(compress);
    if (!r.ok || r.off != len) return fail(OLA_VERIFY_MALFORMED);
    if (proofs.size() != nt || compress.size() != nt) { st.host.words = "wrong number of table proofs"; return fail(OLA_VERIFY_MALFORMED); }

    OlaChallenger& ch = st.transcript;
    for (const WProof& p : proofs) challenger_observe_cap(ch, p.trace_cap.empty() ? nullptr : p.trace_cap[0].data(), p.trace_cap.size());
    for (int i = 0; i < 2 * cfg.num_challenges; i++) st.ctl_challenges.push_back(challenger_get(ch));
    // CtlCheckVars::from_proofs: the opened lookup Zs in cross_table_lookup order, looking sides before the looked side, challenge-minor
    std::vector<std::vector<CtlVar>> ctl_vars(nt);
    for (const HCtl& ctl : set.ctls)
        for (int c = 0; c < cfg.num_challenges; c++) {
            const GpChallenge g = {st.ctl_challenges[2 * (size_t)c], st.ctl_challenges[2 * (size_t)c + 1]};
            for (const HTwc& twc : ctl.looking) ctl_vars[(size_t)twc.table].push_back({g, &twc});
            ctl_vars[(size_t)ctl.looked.table].push_back({g, &ctl.looked});
        }
    size_t poff = 0;
    st.challenges.resize(nt);
    for (size_t t = 0; t < nt; t++) {
        const HTable& air = set.tables[t];
        const WProof& p = proofs[t];
        Challenges& tc = st.challenges[t];
        std::vector<u64> tp((size_t)std::max(air.n_params, 0));
        for (size_t k = 0; k < tp.size(); k++) tp[k] = params ? params[poff + k] : compress[t];
        poff += tp.size();
        challenger_compact(ch);
        int degree_bits = 0;
        if (!degree_bits_of(cfg, p.fri, degree_bits)) return fail(OLA_VERIFY_EMPTY_FRI, (int)t);
        // a path length no tree of this field can have: the reference would reject it at the shape check of the first query
        if (degree_bits < 0 || degree_bits + cfg.rate_bits > MAX_LDE_BITS) {
            st.host.query = 0; st.host.oracle_or_layer = 0;
            return fail(OLA_VERIFY_SHAPE_INITIAL_PATH_LEN, (int)t);
        }
        const int nperm = air.num_permutation_batches(cfg.num_challenges), num_ctl = (int)ctl_vars[t].size();
        if (nperm > 0) for (int i = 0; i < 2 * air.permutation_batch_size() * cfg.num_challenges; i++) tc.perm.push_back(challenger_get(ch));
        challenger_observe_cap(ch, p.zs_cap.empty() ? nullptr : p.zs_cap[0].data(), p.zs_cap.size());
        for (int i = 0; i < cfg.num_challenges; i++) tc.alphas.push_back(challenger_get(ch));
        challenger_observe_cap(ch, p.quotient_cap.empty() ? nullptr : p.quotient_cap[0].data(), p.quotient_cap.size());
        tc.zeta = challenger_get_ext(ch);
        observe_openings(ch, p.op);
        fri_challenges(ch, cfg, p.fri, degree_bits, tc);
        // validate_proof_shape (verifier.rs:326-379)
        const int q = air.quotient_degree_factor();
        // the three caps at the configuration's height (verifier.rs:363-365): a proof made under another cap_height stops here, as in
        // the reference, not at whatever the wrong degree_bits breaks later
        const size_t cap_len = (size_t)1 << cfg.cap_height;
        if (p.trace_cap.size() != cap_len || p.zs_cap.size() != cap_len || p.quotient_cap.size() != cap_len) return fail(OLA_VERIFY_SHAPE_CAP_HEIGHT, (int)t);
        if ((int)p.op.local.size() != 2 * air.ncols || (int)p.op.next.size() != 2 * air.ncols) return fail(OLA_VERIFY_SHAPE_OPENING_WIDTH, (int)t);
        if ((int)p.op.zs.size() != 2 * (nperm + num_ctl) || (int)p.op.zs_next.size() != 2 * (nperm + num_ctl)) return fail(OLA_VERIFY_SHAPE_ZS_WIDTH, (int)t);
        if ((int)p.op.ctl_last.size() != num_ctl) return fail(OLA_VERIFY_SHAPE_CTL_ZS_LAST_WIDTH, (int)t);
        if ((int)p.op.quotient.size() != 2 * q * cfg.num_challenges) return fail(OLA_VERIFY_SHAPE_QUOTIENT_WIDTH, (int)t);
        if (nperm + num_ctl == 0) throw OlaError(OLA_E_INVALID_ARG, "a table without permutation or lookup columns has no Z commitment to verify");
        // the constraints at zeta against the quotient opening (verifier.rs:258-296)
        const u64 g = gl_root_of_unity(degree_bits);
        const Ext2 one = ext_make(1, 0);
        const Ext2 zeta_pow_deg = ext_pow(tc.zeta, (u64)1 << degree_bits);
        const Ext2 z_x = ext_sub(zeta_pow_deg, one);
        const u64 nn = ((u64)1 << degree_bits) % GL_P;
        Consumer consumer;
        for (u64 a : tc.alphas) consumer.alphas.push_back(ext_from(a));
        consumer.accs.assign(tc.alphas.size(), ext_make(0, 0));
        consumer.z_last = ext_sub(tc.zeta, ext_from(gl_inv(g)));
        consumer.lagrange_first = ext_mul(z_x, ext_inv(ext_scalar_mul(ext_sub(tc.zeta, one), nn)));
        consumer.lagrange_last = ext_mul(z_x, ext_inv(ext_scalar_mul(ext_sub(ext_scalar_mul(tc.zeta, g), one), nn)));
        eval_vanishing_poly(air, cfg.num_challenges, p.op, tp.data(), tc.perm, ctl_vars[t], consumer);
        for (size_t i = 0; i < tc.alphas.size(); i++) {
            Ext2 acc = ext_make(0, 0);
            for (int k = q; k-- > 0;) acc = ext_add(ext_mul(acc, zeta_pow_deg), ext_at(p.op.quotient, i * (size_t)q + (size_t)k));
            if (!ext_eq(consumer.accs[i], ext_mul(z_x, acc))) return fail(OLA_VERIFY_QUOTIENT_IDENTITY, (int)t);
        }
        const std::vector<Digest>* caps[3] = {&p.trace_cap, &p.zs_cap, &p.quotient_cap};
        const int num_polys[3] = {air.ncols, nperm + num_ctl, q * cfg.num_challenges};
        const Verdict v = fri_stage(st, cfg, (int)t, caps, num_polys, nperm, degree_bits, tc.zeta, p.op, p.fri, tc);
        if (v.failed()) { st.host = v; pack(st); return st; }
    }
    // verify_cross_table_lookups (cross_table_lookup.rs:551-584); the extra looking products are all one (verifier.rs:152)
    std::vector<size_t> pos(nt, 0);
    bool ctl_ok = true;
    for (const HCtl& ctl : set.ctls)
        for (int c = 0; c < cfg.num_challenges && ctl_ok; c++) {
            u64 prod = 1;
            for (const HTwc& twc : ctl.looking) prod = gl_mul(prod, proofs[(size_t)twc.table].op.ctl_last[pos[(size_t)twc.table]++]);
            const u64 looked = proofs[(size_t)ctl.looked.table].op.ctl_last[pos[(size_t)ctl.looked.table]++];
            if (prod != looked) ctl_ok = false;
        }
    if (!ctl_ok) st.host.reason = OLA_VERIFY_CTL;
    pack(st);
    return st;
}

// ------------------------------------------------------------------------------------------------ the opening level
// The verifier's side of ola_open_and_prove: bytes = write_opening_set || write_fri_proof; caps: the three commitments' caps, 2^cap_height
// digests each; the transcript continues from `ch`, which on return stands where the prover's stands after ola_open_and_prove.
inline Stage opening_stage(const Config& cfg, const u64* caps, const uint32_t num_polys_in[3], uint32_t degree_bits, uint32_t num_permutation_zs,
                           const uint8_t* bytes, size_t len, const OlaChallenger& ch_in) {
    require_config(cfg);
    if ((int)degree_bits + cfg.rate_bits > MAX_LDE_BITS) throw OlaError(OLA_E_INVALID_ARG, "degree_bits");
    if (num_polys_in[0] == 0 || num_polys_in[1] == 0 || num_polys_in[2] == 0 || num_polys_in[0] > 4096 || num_polys_in[1] > 4096 || num_polys_in[2] > 4096)
        throw OlaError(OLA_E_INVALID_ARG, "num_polys: 1..4096 polynomials per commitment");
    if (num_permutation_zs > num_polys_in[1]) throw OlaError(OLA_E_INVALID_ARG, "num_permutation_zs");
    Stage st;
    st.transcript = ch_in;
    auto fail = [&](uint32_t reason) { st.host.reason = reason; pack(st); return st; };
    Reader r(bytes, len, cfg.hasher);
    WOpenings op;
    WFri fri;
    r.opening_set(op);
    r.fri_proof(fri);
    if (!r.ok || r.off != len) return fail(OLA_VERIFY_MALFORMED);
    const int num_polys[3] = {(int)num_polys_in[0], (int)num_polys_in[1], (int)num_polys_in[2]};
    const int num_ctl = num_polys[1] - (int)num_permutation_zs;
    OlaChallenger& ch = st.transcript;
    st.challenges.resize(1);
    Challenges& tc = st.challenges[0];
    tc.zeta = challenger_get_ext(ch);
    observe_openings(ch, op);
    fri_challenges(ch, cfg, fri, (int)degree_bits, tc);
    // the opening set must be the instance's: the batches the device reduces are cut from the rows by these widths
    if ((int)op.local.size() != 2 * num_polys[0] || (int)op.next.size() != 2 * num_polys[0]) return fail(OLA_VERIFY_SHAPE_OPENING_WIDTH);
    if ((int)op.zs.size() != 2 * num_polys[1] || (int)op.zs_next.size() != 2 * num_polys[1]) return fail(OLA_VERIFY_SHAPE_ZS_WIDTH);
    if ((int)op.ctl_last.size() != num_ctl) return fail(OLA_VERIFY_SHAPE_CTL_ZS_LAST_WIDTH);
    if ((int)op.quotient.size() != 2 * num_polys[2]) return fail(OLA_VERIFY_SHAPE_QUOTIENT_WIDTH);
    const size_t cap_len = (size_t)1 << cfg.cap_height;
    const HasherInfo& hasher = hasher_row(cfg.hasher);
    std::vector<Digest> cap[3];
    for (int o = 0; o < 3; o++)
        for (size_t i = 0; i < cap_len; i++) {
            Digest d;
            for (int k = 0; k < 4; k++) {
                d[(size_t)k] = caps[((size_t)o * cap_len + i) * 4 + (size_t)k];
                if (k == 3 && d[3] > hasher.cap_word3_max) throw OlaError(OLA_E_INVALID_ARG, "caps: word 3 of a Keccak digest holds byte 24 only");
                if (hasher.cap_canonical && d[(size_t)k] >= GL_P) throw OlaError(OLA_E_INVALID_ARG, "caps: a digest word is not canonical");
            }
            cap[o].push_back(d);
        }
    const std::vector<Digest>* capp[3] = {&cap[0], &cap[1], &cap[2]};
    const Verdict v = fri_stage(st, cfg, -1, capp, num_polys, (int)num_permutation_zs, (int)degree_bits, tc.zeta, op, fri, tc);
    if (v.failed()) st.host = v;
    st.host.table = -1;
    pack(st);
    return st;
}

}  // namespace vfy
}  // namespace ola
