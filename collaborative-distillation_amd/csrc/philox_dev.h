// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123), host and device: the one
// generator behind the seeded noise image (noise.hip) and the seeded rotation (rotate.hip); tests/synth_oracle.py restates it in numpy.
// Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;   // multipliers
constexpr unsigned PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;   // Weyl increments of the key

struct Philox4 { unsigned v[4]; };

__host__ __device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)PHILOX_M0 * c0, p1 = (unsigned long long)PHILOX_M1 * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
    k0 += PHILOX_W0; k1 += PHILOX_W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

}  // namespace
