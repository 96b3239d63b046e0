// The integer core of the record-keyed noise source: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11; the Random123 constants) and the counter / key of a draw (Noise).  Plain C++: no HIP header, usable from
// host and device, and a host compiler can include it on its own (tools/philox_words.cpp checks it against the numpy reference).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CCN_PHILOX_FN __host__ __device__ inline
#else
#define CCN_PHILOX_FN inline
#endif

namespace ccn {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // key increments (Weyl sequence)

struct Philox4 { uint32_t v[4]; };

// ten rounds of Philox4x32 on counter (c0..c3) under key (k0, k1)
CCN_PHILOX_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// the four words of quad q of draw d of the record with seed `seed`: key (seed & 0xffffffff, seed >> 32), counter (q, d, 0, 0)
CCN_PHILOX_FN Philox4 draw_words(uint64_t seed, uint32_t draw, uint32_t q)
{
    return philox4x32_10(q, draw, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// elements per record a draw can address: q = j >> 2 is one 32-bit counter word
constexpr int64_t kDrawMaxPerRecord = (int64_t)1 << 34;

}  // namespace ccn
