// The plant's generator (csrc/nmpc_rng.h) compiled for the host: for argv[1] counters derived from argv[2] by a 64-bit LCG, one line
// each of the counter, the key, the four Philox words and xi (its bits) for plant_xi(seed, id, row, channel) with seed = the key's two
// words, id, row and channel = the counter's first three.  tests/test_plant_mirror.py compares the lines with the NumPy mirror's.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "nmpc_rng.h"

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 10;
    uint64_t s = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1u;
    auto next = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); };
    for (int i = 0; i < n; ++i) {
        uint32_t c[4], k[2];
        for (uint32_t &w : c) w = next();
        for (uint32_t &w : k) w = next();
        uint32_t x[4] = {c[0], c[1], c[2], c[3]};
        nmpc::philox4x32_10(x, k[0], k[1]);
        const double xi = nmpc::plant_xi((uint64_t)k[0] | ((uint64_t)k[1] << 32), c[0], c[1], c[2]);
        uint64_t bits;
        std::memcpy(&bits, &xi, sizeof bits);
        std::printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32
                    " %08" PRIx32 " %016" PRIx64 "\n", c[0], c[1], c[2], c[3], k[0], k[1], x[0], x[1], x[2], x[3], bits);
    }
    return 0;
}
