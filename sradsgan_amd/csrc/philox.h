// Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85.
// Counter based: the bits depend on (counter, key) only, never on the launch shape.  Users: classify.hip (dropout, first word),
// diffusion.hip and augment.hip (normal draws, all four words: philox_normal4).
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

// four standard normals of counter `group` (= element index / 4) under key (seed, step): Box-Muller on the four words.  The one
// definition behind srhip_diff_randn and every kernel that draws "its values" in place (diffusion.hip, augment.hip).
__device__ __forceinline__ void philox_normal4(unsigned long long seed, unsigned long long step, unsigned long long group, float z[4]) {
  const philox_words w = philox4x32_10((unsigned)group, (unsigned)(group >> 32), (unsigned)step, (unsigned)(step >> 32), (unsigned)seed,
                                       (unsigned)(seed >> 32));
  const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float u1 = ((float)(u[2 * k] >> 9) + 0.5f) * 1.1920928955078125e-07f;       // (0, 1), 23 bits + 1/2: exact in fp32
    const float u2 = ((float)(u[2 * k + 1] >> 9) + 0.5f) * 1.1920928955078125e-07f;
    const float rad = sqrtf(-2.f * logf(u1));
    const float th = 6.283185307179586f * u2;
    z[2 * k] = rad * cosf(th);
    z[2 * k + 1] = rad * sinf(th);
  }
}

}  // namespace srhip
