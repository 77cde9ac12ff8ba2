// Host instantiation of olavm_amd/csrc/keccak.cuh -- the source the kernels are compiled from -- against cases computed by
// tests/keccak_ref.py.  A stand-alone program: tests/test_keccak.py builds it with g++ alone (a second time with
// -fsanitize=address,undefined), writes the case file and runs it.  No HIP, no library.
//
// Case file, one case per line, every number in hexadecimal:
//   hash <n> <n words> <4 digest words>          KeccakHash<25>::hash_no_pad of n words (n = 0 allowed)
//   full <n> <n words> <4 words>                 all 32 bytes of Keccak-256 of n words
//   node <4 left> <4 right> <4 digest words>     two_to_one
//   perm <12 state> <12 new state>               KeccakPermutation::permute
//   onion <k> <k stream words> <12 state>        the permutation's selection rule fed a word stream directly
//   elems <4 digest words> <4 elements>          BytesHash<25>::to_vec
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "keccak.cuh"

using ola::u64;

static bool read_words(std::istringstream& in, size_t n, std::vector<u64>& v) {
    v.resize(n);
    for (size_t i = 0; i < n; i++) {
        std::string t;
        if (!(in >> t)) return false;
        v[i] = std::stoull(t, nullptr, 16);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: host_keccak_check <cases>\n"); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int cases = 0, failures = 0;
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        std::vector<u64> a, want, got;
        bool parsed = false;
        if (kind == "hash" || kind == "full") {
            size_t n = 0;
            in >> std::hex >> n;
            parsed = read_words(in, n, a) && read_words(in, 4, want);
            if (parsed) {
                got.resize(4);
                if (kind == "full") {
                    ola::keccak256_words_host(a.data(), (ola::u32)n, got.data());
                } else {
                    u64 d[4];
                    ola::keccak_hash_words([&](ola::u32 i) { return a[i]; }, (ola::u32)n, d);
                    got.assign(d, d + 4);
                }
            }
        } else if (kind == "node") {
            parsed = read_words(in, 8, a) && read_words(in, 4, want);
            if (parsed) { got.resize(4); ola::keccak_node(a.data(), got.data()); }
        } else if (kind == "perm") {
            parsed = read_words(in, 12, a) && read_words(in, 12, want);
            if (parsed) { got = a; ola::keccak_permutation_host(got.data()); }
        } else if (kind == "onion") {
            size_t k = 0;
            in >> std::hex >> k;
            parsed = read_words(in, k, a) && read_words(in, 12, want);
            if (parsed) {
                size_t at = 0;
                bool overrun = false;
                got.assign(12, 0);
                ola::keccak_onion_collect([&]() -> u64 { if (at >= a.size()) { overrun = true; return 0; } return a[at++]; }, got.data());
                if (overrun || at != a.size()) got.assign(12, ~0ull);   // the stream is cut where the twelfth word is taken: all of it is read, no more
            }
        } else if (kind == "elems") {
            parsed = read_words(in, 4, a) && read_words(in, 4, want);
            if (parsed) { got.resize(4); ola::keccak_digest_elements(a.data(), got.data()); }
        }
        if (!parsed) { std::printf("unreadable case: %.60s\n", line.c_str()); return 2; }
        cases++;
        if (got != want) {
            failures++;
            std::printf("MISMATCH %.40s...\n  got ", line.c_str());
            for (u64 x : got) std::printf(" %016llx", x);
            std::printf("\n  want");
            for (u64 x : want) std::printf(" %016llx", x);
            std::printf("\n");
        }
    }
    std::printf("host_keccak_check: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
