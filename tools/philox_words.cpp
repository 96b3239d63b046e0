// Prints the Philox words of csrc/ccn_philox.h as a host compiler sees the header: one line "seed draw q : r0 r1 r2 r3" (hex) per
// triple read from the arguments, for tests/test_rng_host.py to compare with its numpy reference.  The header is the device's
// integer core; this is the only way to run it without a GPU.
//   c++ -std=c++17 -O1 -I clip-neural-image-conpression_amd/csrc tools/philox_words.cpp -o philox_words
//   philox_words kat                      the three Random123 known-answer vectors (counter and key as given there)
//   philox_words SEED DRAW Q0 NQ ...      quads Q0 .. Q0+NQ-1 of the draw, for each group of four arguments
#include "ccn_philox.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "kat")) {
        const uint32_t kat[3][6] = {{0u, 0u, 0u, 0u, 0u, 0u},
                                    {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                    {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
        for (const auto& k : kat) {
            const ccn::Philox4 r = ccn::philox4x32_10(k[0], k[1], k[2], k[3], k[4], k[5]);
            std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", r.v[0], r.v[1], r.v[2], r.v[3]);
        }
        return 0;
    }
    if (argc < 5 || (argc - 1) % 4) {
        std::fprintf(stderr, "usage: %s kat | SEED DRAW Q0 NQ [SEED DRAW Q0 NQ ...]\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 3 < argc; a += 4) {
        const uint64_t seed = std::strtoull(argv[a], nullptr, 0);
        const uint32_t draw = (uint32_t)std::strtoull(argv[a + 1], nullptr, 0), q0 = (uint32_t)std::strtoull(argv[a + 2], nullptr, 0);
        const uint32_t nq = (uint32_t)std::strtoull(argv[a + 3], nullptr, 0);
        for (uint32_t i = 0; i < nq; ++i) {
            const uint32_t q = q0 + i;                                  // wraps like the counter word
            const ccn::Philox4 r = ccn::draw_words(seed, draw, q);
            std::printf("%" PRIu64 " %" PRIu32 " %" PRIu32 " : %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", seed, draw, q, r.v[0],
                        r.v[1], r.v[2], r.v[3]);
        }
    }
    return 0;
}
