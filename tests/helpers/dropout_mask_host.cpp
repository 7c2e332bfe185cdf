// csrc/dropout_mask.h compiled for the host (tests/test_dropout_cpu.py): the one definition of the dropout mask that every kernel
// of dropout.hip uses, printed for the Python mirror (tests/helpers/philox_ref.py) to compare with.
//   stdin lines:  "philox c0 c1 c2 c3 k0 k1"      -> the four words in hex
//                 "thr p"                          -> the keep threshold of p in hex
//                 "mask n p site step lo hi"       -> n float factors (hex of their bits)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "dropout_mask.h"

int main() {
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    if (!std::strcmp(cmd, "philox")) {
      uint32_t c[4], k[2];
      if (std::scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &c[0], &c[1], &c[2], &c[3], &k[0], &k[1]) != 6) return 2;
      for (int w = 0; w < 4; ++w) std::printf("%08" PRIx32 "%c", ms::philox4x32_10_word(c[0], c[1], c[2], c[3], k[0], k[1], w), w == 3 ? '\n' : ' ');
    } else if (!std::strcmp(cmd, "thr")) {
      double p;
      if (std::scanf("%lf", &p) != 1) return 2;
      std::printf("%08" PRIx32 "\n", ms::dropout_threshold(p));
    } else if (!std::strcmp(cmd, "mask")) {
      unsigned long long n;
      double p;
      uint32_t site, step, lo, hi;
      if (std::scanf("%llu %lf %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &n, &p, &site, &step, &lo, &hi) != 6) return 2;
      const uint32_t thr = ms::dropout_threshold(p);
      const float scale = (float)(1.0 / (1.0 - p));
      for (unsigned long long e = 0; e < n; ++e) {
        const float f = ms::dropout_factor(e, thr, scale, site, lo, hi, step);
        uint32_t bits;
        std::memcpy(&bits, &f, 4);
        std::printf("%08" PRIx32 "%c", bits, e + 1 == n ? '\n' : ' ');
      }
    } else {
      return 3;
    }
  }
  return 0;
}
