// nmpc_rng.h -- the plant's disturbances: a counter-based generator, the same words and the same double on the host and on the device.
//
// Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): a 128-bit counter and a
// 64-bit key go through ten rounds of two 32 x 32 -> 64 bit multiplications, the key bumped between the rounds.  Plain C++: the high word
// is taken from a 64-bit product, nothing is kept between calls, and a draw is a pure function of its arguments, so the disturbance of
// robot `id` at trajectory row `row` on channel `channel` is the same whoever else is active, however the fleet is sharded and in
// whatever order the robots are launched (the rule that uses it: nmpc_loop.h).
//
// Known answers, counter || key -> output:
//   00000000 00000000 00000000 00000000 || 00000000 00000000 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
//   ffffffff ffffffff ffffffff ffffffff || ffffffff ffffffff -> 408f276d 41c83b0e a20bc7c6 6d5451fd
//   243f6a88 85a308d3 13198a2e 03707344 || a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define NMPC_RNG_FN __host__ __device__ inline
#else
#define NMPC_RNG_FN inline
#endif

namespace nmpc {

// c [4] <- Philox4x32-10 of the counter c under the key (k0, k1)
NMPC_RNG_FN void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// One variate: the counter is (id, row, channel, 0), the key (seed & 0xffffffff, seed >> 32).  S = the sum of the four output words
// (0 .. 2^34 - 4) and xi = double(S + 2 - 2^33) * C, C = the double nearest sqrt(3) scaled exactly by 2^-32.  Everything before the one
// multiplication is exact, so xi is the same double everywhere: Irwin-Hall of four, symmetric, mean 0, variance 1, |xi| <= 2 sqrt(3).
NMPC_RNG_FN double plant_xi(uint64_t seed, uint32_t id, uint32_t row, uint32_t channel)
{
    uint32_t c[4] = {id, row, channel, 0u};
    philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
    const uint64_t S = (uint64_t)c[0] + c[1] + c[2] + c[3];
    return (double)((int64_t)S + 2 - ((int64_t)1 << 33)) * 0x1.bb67ae8584caap-32;
}

}  // namespace nmpc
