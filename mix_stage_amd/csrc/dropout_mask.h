// The dropout mask of the ConvNormRelu blocks (layers.py:32-78, p > 0): ONE definition for every kernel of dropout.hip, for
// ms_dropout_mask and -- compiled for the host -- for the CPU test that holds it against the Python mirror
// (tests/helpers/philox_ref.py).  No mask tensor exists in memory: every pass regenerates the bits it needs.
//
//   generator  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
//   key        (seed_lo, seed_hi)
//   counter    (q, site, step, 0)             q = e >> 2, and element e takes word e & 3 of that call
//   e          element dropout: the index in the plain (B, C, HW) order;  channel dropout: b * C + c
//   keep       word >= thr,  thr = min(floor(p * 2^32 + 0.5), 0xffffffff)  (host, in double);  kept values x (float)(1 / (1 - p))
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MS_HD __host__ __device__ __forceinline__
#else
#define MS_HD inline
#endif

namespace ms {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

MS_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// word `w` (0..3) of Philox4x32-10(counter (c0, c1, c2, c3), key (k0, k1))
MS_HD uint32_t philox4x32_10_word(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, int w) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += PHILOX_W0; k1 += PHILOX_W1; }
    const uint32_t hi0 = philox_mulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = philox_mulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
  }
  return w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
}

// what a block's passes need to regenerate its mask: by-value kernel arguments but for the three state words
struct DropoutArgs {
  const int32_t* state;   // device: seed lo, seed hi, step, reserved 0
  uint32_t thr;           // keep iff word >= thr
  float scale;            // (float)(1 / (1 - p))
  uint32_t site;          // module_id + (visit << 20)
  int channelwise;        // 1: one draw per (b, c) plane (nn.Dropout2d)
};

// the factor of element index e: `scale` or 0
MS_HD float dropout_factor(uint64_t e, uint32_t thr, float scale, uint32_t site, uint32_t seed_lo, uint32_t seed_hi, uint32_t step) {
  const uint32_t word = philox4x32_10_word((uint32_t)(e >> 2), site, step, 0u, seed_lo, seed_hi, (int)(e & 3));
  return word >= thr ? scale : 0.f;
}

// thr of a probability 0 <= p < 1 (the callers have checked the range)
inline uint32_t dropout_threshold(double p) {
  const double t = p * 4294967296.0 + 0.5;
  return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;       // (the cast truncates: floor of a non-negative value)
}

}  // namespace ms
