// Finds the first i for which the challenger state (i, 0, ..., 0) makes KeccakPermutation::permute reject a word: h1 = Keccak-256 of
// the state's 96 bytes has a word >= p = 2^64 - 2^32 + 1, that is, high half 0xFFFFFFFF and a non-zero low half.  About 2^30 hashes
// (probability 2^-32 per word, four words per hash).  The host instantiation of olavm_amd/csrc/keccak.cuh does the search only;
// tests/golden/make_keccak_vectors.py records i and computes the twelve expected outputs with tests/keccak_ref.py.
//
//   g++ -O2 -std=c++17 -pthread -Wno-unknown-pragmas -Iolavm_amd/csrc tools/find_keccak_reject.cpp -o find_keccak_reject && ./find_keccak_reject [threads]
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "keccak.cuh"

using ola::u64;

int main(int argc, char** argv) {
    const unsigned threads = argc > 1 ? (unsigned)std::atoi(argv[1]) : 16u;
    const u64 chunk = 1ull << 20;
    std::atomic<u64> next{0}, best{~0ull};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; t++) {
        pool.emplace_back([&]() {
            for (;;) {
                const u64 start = next.fetch_add(chunk);
                if (start >= best.load()) return;   // chunks are handed out in increasing order: everything below `best` is already taken
                for (u64 i = start; i < start + chunk; i++) {
                    u64 s[12] = {i, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, h[4];
                    ola::keccak256_words_host(s, 12, h);
                    if (h[0] >= ola::GL_P || h[1] >= ola::GL_P || h[2] >= ola::GL_P || h[3] >= ola::GL_P) {
                        u64 b = best.load();
                        while (i < b && !best.compare_exchange_weak(b, i)) {}
                        break;
                    }
                }
            }
        });
    }
    for (auto& th : pool) th.join();
    std::printf("%llu\n", (unsigned long long)best.load());
    return 0;
}
