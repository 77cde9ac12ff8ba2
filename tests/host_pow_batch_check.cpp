// The batch size of the proof-of-work search (olavm_amd/csrc/pow_batch.h) for every proof_of_work_bits a configuration may hold,
// 1..40, without a device and without the library: a stand-alone program that tests/test_pow_batch.py builds with g++ (a second time
// with -fsanitize=address,undefined) and runs directly.  Searches of 37 bits and more are never run on a device by the suite -- an
// expected search takes minutes to hours -- so the launch geometry they would get is checked here.
#include <cstdio>

#include "../olavm_amd/csrc/pow_batch.h"

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

int main() {
    for (uint32_t bits = 1; bits <= 40; bits++) {
        const uint64_t batch = pow_batch(bits), before = ((uint64_t)4 << bits) > ((uint64_t)1 << 14) ? (uint64_t)4 << bits : (uint64_t)1 << 14;
        const uint64_t blocks = batch / 256;
        CHECK(batch >= ((uint64_t)1 << 14), "%u bits: a batch of %llu nonces", bits, (unsigned long long)batch);
        CHECK(batch % 256 == 0 && (batch & (batch - 1)) == 0, "%u bits: %llu nonces are no whole number of workgroups", bits, (unsigned long long)batch);
        // fits a grid: at least one workgroup, at most 2^30, and the 32-bit number handed to the launch is that number
        CHECK(blocks >= 1 && blocks <= ((uint64_t)1 << 30), "%u bits: %llu workgroups", bits, (unsigned long long)blocks);
        CHECK((uint64_t)pow_batch_blocks(batch) == blocks, "%u bits: the grid truncates %llu workgroups to %u", bits, (unsigned long long)blocks, pow_batch_blocks(batch));
        // every thread of the launch has a 32-bit global index
        CHECK(blocks * 256 < ((uint64_t)1 << 32), "%u bits: %llu threads", bits, (unsigned long long)(blocks * 256));
        if (bits <= 28) CHECK(batch == before, "%u bits: %llu nonces, %llu before", bits, (unsigned long long)batch, (unsigned long long)before);
        CHECK(batch <= before, "%u bits: the batch grew", bits);
        // the search's loop advances by one batch from 0: the first 2^40 nonces are covered without a gap and without a wrap
        CHECK(batch != 0 && (((uint64_t)1 << 42) % batch) == 0, "%u bits: batches do not tile the nonces", bits);
        if (bits > 1) CHECK(batch >= pow_batch(bits - 1), "%u bits: smaller than for %u", bits, bits - 1);
    }
    // what the suite runs on the device: the sizes of 1, 8, 12, 16 and 20 bits
    CHECK(pow_batch(1) == 16384 && pow_batch(8) == 16384 && pow_batch(12) == 16384 && pow_batch(16) == 262144 && pow_batch(20) == 4194304, "the small sizes");
    CHECK(pow_batch(28) == ((uint64_t)1 << 30) && pow_batch(29) == ((uint64_t)1 << 31) && pow_batch(37) == ((uint64_t)1 << 31) && pow_batch(40) == ((uint64_t)1 << 31), "the large sizes");
    // as the code stood: (unsigned)((4 << bits) / 256) for 37..40 bits is 2^31 (refused) or 0 (nothing launched)
    for (uint32_t bits = 37; bits <= 40; bits++) {
        const uint64_t old_blocks = ((uint64_t)4 << bits) / 256;
        CHECK((uint32_t)old_blocks == 0 || old_blocks > 0x7FFFFFFFull, "%u bits: the old size was launchable after all", bits);
    }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("bits 1..40: every batch fits a grid\n");
    return 0;
}
