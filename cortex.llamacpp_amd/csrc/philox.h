// philox.h — Philox4x32-10 from its published round function (Salmon et al., SC'11) as the device samplers draw from it (sample.hip, sample_vocab.hip):
// key = seed, counter words = (counter lo, counter hi, stream, 0), u = (word 0 >> 8) * 2^-24.
#pragma once
#include <hip/hip_runtime.h>

namespace mi355 {

struct Philox4 { unsigned w[4]; };
__host__ __device__ inline Philox4 philox4x32_10(unsigned long long key, unsigned long long ctr_lo, unsigned stream) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    unsigned c0 = (unsigned)ctr_lo, c1 = (unsigned)(ctr_lo >> 32), c2 = stream, c3 = 0u;
    unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)M0 * c0, p1 = (unsigned long long)M1 * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}
__host__ __device__ inline float philox_u(unsigned long long key, unsigned long long ctr, unsigned stream) {
    return (float)(philox4x32_10(key, ctr, stream).w[0] >> 8) * 5.9604644775390625e-08f;   // 2^-24: exact
}

}  // namespace mi355
