// Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85.
// Counter based: the bits depend on (counter, key) only, never on the launch shape.  Users: classify.hip (dropout, first word),
// diffusion.hip (normal draws, all four words).
#pragma once
#include <hip/hip_runtime.h>

namespace srhip {

struct philox_words {
  unsigned x, y, z, w;
};

__device__ __forceinline__ philox_words philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
    const unsigned n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    const unsigned n3 = (unsigned)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return philox_words{c0, c1, c2, c3};
}

__device__ __forceinline__ unsigned philox_first(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  return philox4x32_10(c0, c1, c2, c3, k0, k1).x;
}

}  // namespace srhip
