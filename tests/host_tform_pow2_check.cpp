// CPU check of the multiplication-free 64-point closing block of the transform passes (olavm_amd/csrc/tform.cuh: tf_mul_pow2,
// tf_round6_pair; the kernel is ntt2t.cuh's 6-bit closing pass), on a RANGE-CHECKED limb type: tform.cuh is compiled with
// OLA_TF_LIMB = Limb, a class that does the limb arithmetic in 64 bits and fails the run as soon as a limb's magnitude reaches
// 2^31 - 2^8, the bound of tf_to_u64 that the header's signed 32-bit limbs must keep; the tighter bounds the header states per
// function are asserted where the functions return.  Checked:
//   * for every e in 0..63, forward and inverse, tf_mul_pow2<39 e mod 192> (inverse: <153 e mod 192>) against canonical
//     multiplication by the REFERENCE's w_64^e (plonky2/field/src/types.rs:240-244), against
//     tf_sub_mul_pow2<S>(x, 0), and its magnitudes on inputs that sit on the 2^28 bound;
//   * a full 64-point block as the pass runs it -- load multiplication, tf_dft<4>, the shift twiddles of each m_low written as
//     exchange words, tf_dft<2>, canonical fold -- against a naive DFT in the reference's order (cfft/serial.rs:89-152);
//   * inputs random and tiled from {0, 1, p-1, p, 2^32-1, 2^32, 0xFFFFFFFF00000000, 2^64-1}.
// Built and run by tests/test_host_tform_pow2.py (no GPU needed).
//   g++ -std=c++17 -O1 -Wno-unknown-pragmas -Iolavm_amd/csrc tests/host_tform_pow2_check.cpp -o check && ./check
#include <cstdio>
#include <cstdlib>

static int fails = 0;
#define CHECK(cond, what) do { if (!(cond)) { if (fails < 10) fprintf(stderr, "FAIL: %s (line %d)\n", what, __LINE__); fails++; } } while (0)

struct Limb {
    long long v;
    static constexpr long long LIMIT = (1ll << 31) - (1ll << 8);
    static Limb mk(long long x) {
        CHECK(x < LIMIT && x > -LIMIT, "a limb left the signed 32-bit bound");
        Limb l;
        l.v = x;
        return l;
    }
    Limb() : v(0) {}
    Limb(int x) : v(x) {}
    explicit operator unsigned() const { return (unsigned)(int)v; }
    explicit operator int() const { return (int)v; }
    explicit operator long long() const { return v; }
    friend Limb operator+(Limb a, Limb b) { return mk(a.v + b.v); }
    friend Limb operator-(Limb a, Limb b) { return mk(a.v - b.v); }
    friend Limb operator-(Limb a) { return mk(-a.v); }
    friend Limb operator&(Limb a, Limb b) { return mk(a.v & b.v); }
    friend Limb operator>>(Limb a, int s) { return mk(a.v >> s); }
    friend Limb operator<<(Limb a, int s) { return mk(a.v * (1ll << s)); }
};
#define OLA_TF_LIMB Limb
#include "tform.cuh"

using namespace ola;

static u64 rng_state = 0x243F6A8885A308D3ull;
static u64 rnd() {
    u64 x = (rng_state += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static const u64 SPECIAL[8] = {0, 1, GL_P - 1, GL_P, 0xFFFFFFFFull, 0x100000000ull, 0xFFFFFFFF00000000ull, ~0ull};

static u64 tf_value(const T4& x) {   // sum v_i 2^(24 i) mod p, the slow way
    u64 r = 0;
    for (int i = 3; i >= 0; --i) {
        r = gl_mul(r, 1ull << 24);
        const long long v = x.v[i].v;
        r = v >= 0 ? gl_add(r, (u64)v) : gl_sub(r, (u64)(-v));
    }
    return r;
}
static long long mag(const T4& x) {
    long long m = 0;
    for (int i = 0; i < 4; i++) m = x.v[i].v < 0 ? (m > -x.v[i].v ? m : -x.v[i].v) : (m > x.v[i].v ? m : x.v[i].v);
    return m;
}
static int limb_of(int shape, int bound) {   // |result| <= bound, sitting on it in shapes 1 and 2
    const u64 h = rnd();
    switch (shape % 6) {
        case 0: return (int)(h % (2ull * bound + 1)) - bound;
        case 1: return bound - (int)(h & 0xFF);
        case 2: return -bound + (int)(h & 0xFF);
        case 3: return (int)(h & 0xFFFFFF) % (bound + 1);
        case 4: return -((int)(h & 0xFFFFFF) % (bound + 1));
        default: return (int)(h & 3) - 1;
    }
}
static T4 vec(int bound) {
    T4 x;
    const u64 h = rnd();
    for (int i = 0; i < 4; i++) x.v[i] = limb_of((int)(h >> (8 * i)), bound);
    return x;
}

// ---- every exponent: tf_mul_pow2<tf_root_exp(6) * E mod 192> is multiplication by the reference's w_64^E
template <int E, bool INV>
static void check_exp(long n) {
    constexpr int S = (tf_root_exp(6, INV) * E) % 192;
    u64 w = gl_root_of_unity(6);
    if (INV) w = gl_inv(w);
    const u64 we = gl_pow(w, E);
    CHECK(gl_pow(2, S) == we, "2^S is not the reference's w_64^e");
    constexpr long long in_bound = (1ll << 28) - 1;   // what tf_dft<4> returns on loaded elements (header of tf_round6_pair)
    for (long it = 0; it < n + 8; it++) {
        T4 x;
        if (it < 8) {   // a loaded special word, grown by the four doublings of a radix-16 block
            x = tf_from_u64(SPECIAL[it]);
            for (int i = 0; i < 4; i++) x.v[i] = x.v[i] << 4;
        } else {
            x = vec((int)in_bound);
        }
        const T4 y = tf_mul_pow2<S>(x);
        CHECK(tf_value(y) == gl_mul(tf_value(x), we), "tf_mul_pow2 value");
        const T4 zero = {};
        const T4 z = tf_sub_mul_pow2<S>(x, zero);
        // the same value; the same limbs too unless the shift both negates and carries (tf_sub_mul_pow2 then splits -x, tf_mul_pow2 x)
        CHECK(tf_value(y) == tf_value(z), "tf_mul_pow2 differs from tf_sub_mul_pow2<S>(x, 0)");
        if (S < 96 || S % 24 == 0)
            for (int i = 0; i < 4; i++) CHECK(y.v[i].v == z.v[i].v, "tf_mul_pow2's limbs differ from tf_sub_mul_pow2<S>(x, 0)'s");
        const long long out_bound = (S % 24) ? (1ll << 24) + ((mag(x) >> (24 - S % 24)) + 1) : mag(x);
        CHECK(mag(y) <= out_bound, "tf_mul_pow2 magnitude");
        CHECK(mag(y) < (1ll << 28), "tf_mul_pow2 output above 2^28: the radix-4 block would leave 2^30");
    }
    if constexpr (E + 1 < 64) check_exp<E + 1, INV>(n);
}

// ---- a 64-point block as the 6-bit closing pass runs it
template <bool INV, int H>
static void round6(int m_low, const T4* x, u64* out) {
    switch (m_low) {
        case 0: tf_round6_pair<0, INV, H>(x, out, 1); break;
        case 1: tf_round6_pair<1, INV, H>(x, out, 1); break;
        case 2: tf_round6_pair<2, INV, H>(x, out, 1); break;
        default: tf_round6_pair<3, INV, H>(x, out, 1); break;
    }
}
static int rev(int x, int bits) {
    int r = 0;
    for (int i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
    return r;
}
template <bool INV>
static void check_block(const u64* in, const u64* mult) {
    u64 a[64];   // what the block transforms: the loaded words times their load multipliers
    for (int m = 0; m < 64; m++) a[m] = gl_mul(gl_canon(in[m]), gl_canon(mult[m]));
    T4 ex[64];   // the exchange buffer, indexed by m
    for (int m_low = 0; m_low < 4; m_low++) {
        T4 x[16];
        for (int j = 0; j < 16; j++) {
            u64 lo, hi;
            mul_wide(in[m_low + 4 * j], mult[m_low + 4 * j], lo, hi);
            x[j] = tf_from_u128(lo, hi);
        }
        tf_dft<4, INV>(x);
        for (int j = 0; j < 16; j++) CHECK(mag(x[j]) < (1ll << 28), "radix-16 output above 2^28");
        u64 w01[16], w23[16];
        round6<INV, 0>(m_low, x, w01);
        round6<INV, 1>(m_low, x, w23);
        for (int j = 0; j < 16; j++) {
            T4& e = ex[m_low + 4 * j];
            e.v[0] = (i32)(u32)w01[j];
            e.v[1] = (i32)(u32)(w01[j] >> 32);
            e.v[2] = (i32)(u32)w23[j];
            e.v[3] = (i32)(u32)(w23[j] >> 32);
        }
    }
    u64 w = gl_root_of_unity(6);
    if (INV) w = gl_inv(w);
    for (int m_hi = 0; m_hi < 16; m_hi++) {
        T4 y[4];
        for (int j2 = 0; j2 < 4; j2++) y[j2] = ex[4 * m_hi + j2];
        tf_dft<2, INV>(y);
        for (int j2 = 0; j2 < 4; j2++) {
            CHECK(mag(y[j2]) <= (1ll << 30), "radix-4 output above 2^30");
            const int q = rev(j2, 2) * 16 + rev(m_hi, 4);
            u64 acc = 0;
            for (int m = 0; m < 64; m++) acc = gl_add(acc, gl_mul(a[m], gl_pow(w, (u64)m * q)));
            CHECK(tf_to_u64<true>(y[j2]) == acc, "64-point block differs from the naive DFT");
        }
    }
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 2000;
    check_exp<0, false>(n);
    check_exp<0, true>(n);
    u64 in[64], mult[64];
    for (long it = 0; it < n / 4 + 80; it++) {
        for (int m = 0; m < 64; m++) {
            // it < 64: both tiled from the special words (every pairing of them meets in some slot), then mixed, then random
            in[m] = it < 72 ? SPECIAL[(m + it) % 8] : rnd();
            mult[m] = it < 64 ? SPECIAL[(m * (1 + it / 8) + it / 8) % 8] : (it < 80 && m % 3 == 0 ? SPECIAL[(m + it) % 8] : rnd());
        }
        if (it == 72) for (int m = 0; m < 64; m++) mult[m] = 1;
        check_block<false>(in, mult);
        check_block<true>(in, mult);
    }
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    printf("tform pow2 ok: %ld samples per exponent\n", n);
    return 0;
}
