// GPU check of the verifying half of the C++ host layer (include/ola_host.hpp): the reference's unit tests for this path end in
// `verify_proof` (circuits/src/stark/ola_stark.rs tests: prove_with_traces, then verify_proof), and so does this program.  Built with
// g++ and run by tests/test_gpu_host_verify_api.py, which supplies the fixture (an AIR-set blob with traces, the format of
// tests/host_api_check.cpp) and holds what this program prints about the tampered proof to the oracle's verdict on the same bytes.
//
//   host_verify_api_check <fixture> <proof-out> <tampered-out>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>

#include "ola_host.hpp"

using namespace ola_host;

static int failures = 0;
#define EXPECT(cond)                                                                     \
    do {                                                                                 \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static std::vector<std::vector<F>> read_sections(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::printf("cannot open %s\n", path); std::exit(2); }
    auto rd = [&]() { F w = 0; f.read(reinterpret_cast<char*>(&w), 8); return w; };
    const F magic = rd(), count = rd();
    if (magic != 0x4F4C41484F5354ULL) { std::printf("bad fixture magic\n"); std::exit(2); }
    std::vector<std::vector<F>> s(count);
    for (auto& sec : s) { sec.resize(rd()); f.read(reinterpret_cast<char*>(sec.data()), (std::streamsize)sec.size() * 8); }
    return s;
}
static void write_bytes(const char* path, const std::vector<uint8_t>& b) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(b.data()), (std::streamsize)b.size());
}

int main(int argc, char** argv) {
    if (argc < 4) { std::printf("usage: host_verify_api_check <fixture> <proof-out> <tampered-out>\n"); return 2; }
    const auto sec = read_sections(argv[1]);      // [unused, blob, log_n, params, compress, n_params, trace 0 ..]
    Gpu gpu;
    const std::vector<F>& airset = sec[1];
    std::vector<uint32_t> log_n(sec[2].begin(), sec[2].end());
    std::vector<std::vector<F>> traces(sec.begin() + 6, sec.end());

    // ---- prove_with_traces, then verify_proof
    const std::vector<uint8_t> proof = prove_with_traces(gpu, airset, traces, log_n, sec[3], sec[4]);
    write_bytes(argv[2], proof);
    OlaVerifyReport rep = verify_proof(gpu, airset, proof, sec[3]);
    EXPECT(rep.accepted == 1 && rep.reason == OLA_VERIFY_OK && rep.table == -1 && rep.query == -1 && rep.oracle_or_layer == -1);
    EXPECT(rep.kernel_launches == 2 && rep.query_jobs == 28 * traces.size() && rep.merkle_jobs >= 3 * rep.query_jobs);
    EXPECT(std::strcmp(rep.message, "accepted") == 0);
    rep = verify_proof(gpu, airset, proof);        // the parameters from the proof's compress challenges, as the reference takes them
    EXPECT(rep.accepted == 1);
    // ---- one bit flipped: rejected, and the report says where; the driver compares with the oracle
    std::vector<uint8_t> bad = proof;
    bad[bad.size() / 3] ^= 0x10;
    write_bytes(argv[3], bad);
    rep = verify_proof(gpu, airset, bad, sec[3]);
    EXPECT(rep.accepted == 0 && rep.reason != OLA_VERIFY_OK);
    std::printf("tampered: reason %u table %d query %d oracle_or_layer %d message %s\n", rep.reason, rep.table, rep.query, rep.oracle_or_layer, rep.message);
    // the verdict is a report; a call that cannot run throws
    bool threw = false;
    try { auto blob = airset; blob.pop_back(); (void)verify_proof(gpu, blob, proof); } catch (const Error& e) { threw = e.code == OLA_E_INVALID_ARG; }
    EXPECT(threw);
    EXPECT(verify_proof(gpu, airset, proof).accepted == 1);         // and the context goes on verifying

    // ---- the opening level: open_and_prove, then verify_stark_proof_opening on the same transcript
    {
        std::mt19937_64 rng(7);
        const uint32_t degree_bits = 9;
        auto cols = [&](size_t k) { std::vector<PolynomialValues> v(k, PolynomialValues((size_t)1 << degree_bits)); for (auto& c : v) for (auto& x : c) x = rng() % 0xFFFFFFFF00000001ULL; return v; };
        PolynomialBatch trace = PolynomialBatch::from_values(gpu, cols(5)), zs = PolynomialBatch::from_values(gpu, cols(3)), quotient = PolynomialBatch::from_coeffs(gpu, cols(2));
        Challenger prover(gpu), verifier(gpu);
        for (const PolynomialBatch* b : {&trace, &zs, &quotient}) { prover.observe_cap(b->merkle_cap()); verifier.observe_cap(b->merkle_cap()); }
        const auto parts = open_and_prove(gpu, trace, zs, quotient, 1, prover);
        const std::array<MerkleCap, 3> caps = {trace.merkle_cap(), zs.merkle_cap(), quotient.merkle_cap()};
        OlaVerifyReport r = verify_stark_proof_opening(gpu, caps, {5, 3, 2}, degree_bits, 1, parts.first, parts.second, verifier);
        EXPECT(r.accepted == 1 && r.query_jobs == 28 && r.table == -1);
        EXPECT(std::memcmp(&prover.raw(), &verifier.raw(), sizeof(OlaChallenger)) == 0);
        EXPECT(prover.get_challenge() == verifier.get_challenge());
        auto fri = parts.second;
        fri[fri.size() - 9] ^= 1;                                   // the last word of the final polynomial
        Challenger again(gpu);
        for (const PolynomialBatch* b : {&trace, &zs, &quotient}) again.observe_cap(b->merkle_cap());
        r = verify_stark_proof_opening(gpu, caps, {5, 3, 2}, degree_bits, 1, parts.first, fri, again);
        EXPECT(r.accepted == 0 && r.reason == OLA_VERIFY_POW);       // the final polynomial is in the transcript the witness was ground for
    }
    if (failures == 0) std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
