"""GPU: every elementwise / loss / optimizer entry point (launch labels `ew|ew_*`, tests/helpers/ew_table.py) against a float64
reference at the sizes production runs and at the edges of each launcher's grid arithmetic.

Each case runs under the launch timing, asserts that the launches it exists for took place (and that refused calls launched
nothing), builds its reference in float64 from plain torch or the oracle, and compares.  Seeds derive from the case id.

Bars (the kind is stated per case in the table):
  exact    pure data movement, skipped Adam segments, refused steps, index outputs: torch.equal
  round    to_cb8 / btc_to_cb8 of arbitrary fp32: equal to torch's own cast.  pack8 (conv16_kernel.h) converts with
           __builtin_convertvector, i.e. fptrunc: round to nearest even for bf16 and fp16, fp16 subnormals kept.  The velocity form is
           compared with the fp32 difference rounded once
  fp32     the bar the existing test of the entry point set (1e-5 softmax_mix and cross-entropy gradients, 1e-6 lerp / loss values /
           loss gradients / embedding gradient), unchanged for the larger sizes
  derived  no bar existed: the device error must be at most 4 x the error of torch's float32 CPU evaluation of the same formula
           against the same float64 reference (floored at 2 * 2^-24), measured in the test on the same inputs
Every fp32 / derived comparison is made in two metrics, both over all elements:
  max   max|got - ref| / max|ref|
  elem  max_i |got_i - ref_i| / (|ref_i| + rms(ref))      (small elements are held too; the derived yardstick is taken in the same metric)
Hyper-parameters that cross the C ABI as floats (betas, eps, lr, max_norm, slope, momentum, loss weights) enter the float64
references as the float32 values the library receives.

LeakyReLU kinks of the BatchNorm cases: as in test_gpu_dispatch_parity the float64 reference takes its slope mask from the sign of the
device output; the elements where that differs from the float64 sign must be few and within rounding of 0.

Shown to fail: the library was built with each of these numerics-only changes and this file run once per build (cases that went red):
  softmax-mix forward reads tile[r * FC + fl] instead of tile[r * (FC + 1) + fl]     all 11 mix_* cases (wrong for fc = 1 too: the
                                                                                     four cases of test_gpu_kernels.test_softmax_mix see it as well)
  softmax-mix forward stores with r = e / FC, fl = e % FC instead of e / nf            mix_headline, mix_t40, mix_m1, mix_prime67: the cases with a
                                                                                     short last chunk (test_gpu_kernels.py: all pass)
  cross-entropy forward, loop path, `den` loop started at c = 1                      ce_bct_c25_r2048, ce_bct_c25_r8192, ce_bct_c9_r150,
                                                                                     ce_nc_c25_r1000, ce_plain_acc_c25 (test_gpu_kernels.py: all pass)
  sq_partial_kernel without its `if (i < n4)` remainder vector                       sqnorm_n4, 5, 1023, 2047, 2049, 4095, 4097, 12289, 15000064
                                                                                     (test_gpu_kernels.py: all pass)
  adam_prep_seg_kernel with t = step - first + 2                                     all four adam_seg_* cases
  adam_seg_kernel: second vector updated with the first vector's step size           adam_seg_big_uneven
  ms_bn_bwd_apply with 1 / (B * HW) of the local shard                               the five bn_*_w2 cases
  cb8_from_btc: velocity as x[t + 1] - x[t]                                           all 14 cb8_* cases

Measured on one MI355X, every derived bar (yard = error of the float32 CPU evaluation, dev = error of this library, both against the
float64 reference, in the two metrics; the bar is 4 x max(yard, 1.2e-7)).  The kernels reduce in a fixed order, so a rerun prints the
same figures (pytest -s prints these and the fixed-bar figures of every case):

  MEASURED_TABLE_BEGIN
  case                       quantity                        yard max   dev max   yard elem  dev elem
  mix_configs3               dscore                           5.1e-07   9.8e-07     6.4e-06   1.4e-05
  ce_bct_c8_r8192            loss                             7.1e-08   9.7e-09     3.5e-08   4.8e-09
  ce_bct_c25_r8192           loss                             5.2e-09   8.9e-08     2.6e-09   4.5e-08
  sqnorm_n1                  aligned                          0.0e+00   0.0e+00     0.0e+00   0.0e+00
  sqnorm_n1                  offset by one float              0.0e+00   0.0e+00     0.0e+00   0.0e+00
  sqnorm_n3                  aligned                          4.6e-08   4.6e-08     2.3e-08   2.3e-08
  sqnorm_n3                  offset by one float              4.6e-08   4.6e-08     2.3e-08   2.3e-08
  sqnorm_n4                  aligned                          6.1e-09   6.1e-09     3.0e-09   3.0e-09
  sqnorm_n4                  offset by one float              6.1e-09   6.1e-09     3.0e-09   3.0e-09
  sqnorm_n5                  aligned                          1.9e-08   1.9e-08     9.6e-09   9.6e-09
  sqnorm_n5                  offset by one float              1.9e-08   1.9e-08     9.6e-09   9.6e-09
  sqnorm_n1023               aligned                          1.4e-08   1.4e-08     7.0e-09   7.0e-09
  sqnorm_n1023               offset by one float              1.4e-08   1.4e-08     7.0e-09   7.0e-09
  sqnorm_n2047               aligned                          2.0e-09   6.7e-08     1.0e-09   3.4e-08
  sqnorm_n2047               offset by one float              2.0e-09   2.0e-09     1.0e-09   1.0e-09
  sqnorm_n2049               aligned                          5.1e-08   1.3e-08     2.5e-08   6.5e-09
  sqnorm_n2049               offset by one float              5.1e-08   1.3e-08     2.5e-08   6.5e-09
  sqnorm_n4095               aligned                          2.4e-09   2.4e-09     1.2e-09   1.2e-09
  sqnorm_n4095               offset by one float              2.4e-09   2.4e-09     1.2e-09   1.2e-09
  sqnorm_n4097               aligned                          6.3e-08   6.3e-08     3.2e-08   3.2e-08
  sqnorm_n4097               offset by one float              6.3e-08   4.7e-08     3.2e-08   2.3e-08
  sqnorm_n12289              aligned                          5.2e-08   1.1e-08     2.6e-08   5.3e-09
  sqnorm_n12289              offset by one float              5.2e-08   1.1e-08     2.6e-08   5.3e-09
  sqnorm_n15000064           aligned                          3.1e-08   3.1e-08     1.5e-08   1.5e-08
  sqnorm_n15000064           offset by one float              3.1e-08   3.1e-08     1.5e-08   1.5e-08
  adam_seg_n64_one           p                                6.5e-08   6.5e-08     5.0e-08   5.0e-08
  adam_seg_n64_one           m                                6.5e-08   6.5e-08     6.8e-08   6.8e-08
  adam_seg_n64_one           v                                9.0e-08   8.2e-08     6.6e-08   6.3e-08
  adam_seg_n64_one           p offset                         6.5e-08   6.5e-08     5.0e-08   5.0e-08
  adam_seg_n64_one           m offset                         6.5e-08   6.5e-08     6.8e-08   6.8e-08
  adam_seg_n64_one           v offset                         9.0e-08   8.2e-08     6.6e-08   6.3e-08
  adam_seg_n64000_chunks     p                                8.6e-08   8.6e-08     1.0e-07   1.0e-07
  adam_seg_n64000_chunks     m                                5.3e-08   9.0e-08     1.3e-07   1.1e-07
  adam_seg_n64000_chunks     v                                3.9e-08   3.9e-08     1.4e-07   9.4e-08
  adam_seg_n64000_chunks     p offset                         8.6e-08   8.6e-08     1.0e-07   1.0e-07
  adam_seg_n64000_chunks     m offset                         5.3e-08   9.0e-08     1.3e-07   1.1e-07
  adam_seg_n64000_chunks     v offset                         3.9e-08   3.9e-08     1.4e-07   9.4e-08
  adam_seg_big_uneven        p                                7.3e-08   7.3e-08     1.2e-07   1.2e-07
  adam_seg_big_uneven        m                                8.1e-08   6.2e-08     2.6e-07   2.0e-07
  adam_seg_big_uneven        v                                9.9e-08   9.9e-08     2.0e-07   1.6e-07
  adam_seg_big_uneven        p offset                         7.3e-08   7.3e-08     1.2e-07   1.2e-07
  adam_seg_big_uneven        m offset                         8.1e-08   6.2e-08     2.6e-07   2.0e-07
  adam_seg_big_uneven        v offset                         9.9e-08   9.9e-08     2.0e-07   1.6e-07
  adam_seg_n64000_nonfinite  p                                6.2e-08   6.2e-08     8.1e-08   8.1e-08
  adam_seg_n64000_nonfinite  m                                7.6e-08   7.3e-08     1.5e-07   8.8e-08
  adam_seg_n64000_nonfinite  v                                1.2e-07   9.5e-08     1.2e-07   8.6e-08
  adam_plain_n64001          p                                8.6e-08   8.6e-08     1.1e-07   1.1e-07
  adam_plain_n64001          m                                4.8e-08   4.8e-08     1.7e-07   1.7e-07
  adam_plain_n64001          v                                8.1e-08   8.1e-08     1.4e-07   1.4e-07
  adam_plain_big             p                                8.6e-08   8.6e-08     1.2e-07   1.2e-07
  adam_plain_big             m                                7.7e-08   7.7e-08     4.3e-07   4.3e-07
  adam_plain_big             v                                1.3e-07   1.3e-07     2.2e-07   2.2e-07
  adam_plain_nonorm          p                                1.2e-07   1.2e-07     1.1e-07   1.1e-07
  adam_plain_nonorm          m                                6.5e-08   6.5e-08     1.2e-07   1.2e-07
  adam_plain_nonorm          v                                3.5e-08   3.5e-08     1.0e-07   1.0e-07
  bn_c1_b2047_hw1_w1         stats sum                        5.6e-08   2.1e-08     2.8e-08   1.0e-08
  bn_c1_b2047_hw1_w1         stats M2                         8.1e-08   1.9e-08     4.1e-08   9.3e-09
  bn_c1_b2047_hw1_w1         save mean                        6.8e-08   8.6e-09     3.4e-08   4.3e-09
  bn_c1_b2047_hw1_w1         save invstd                      1.2e-07   3.6e-08     5.9e-08   1.8e-08
  bn_c1_b2047_hw1_w1         y                                1.3e-07   4.1e-08     1.3e-07   4.3e-08
  bn_c1_b2047_hw1_w1         running_mean                     9.1e-08   1.0e-08     4.6e-08   5.1e-09
  bn_c1_b2047_hw1_w1         running_var                      2.7e-08   2.7e-08     1.4e-08   1.4e-08
  bn_c1_b2047_hw1_w1         sums dz (dbeta share)            7.2e-07   1.8e-08     3.6e-07   8.9e-09
  bn_c1_b2047_hw1_w1         sums dz*xhat (dgamma share)      2.1e-07   9.5e-09     1.1e-07   4.7e-09
  bn_c1_b2047_hw1_w1         dyr                              2.3e-07   1.1e-07     1.8e-07   1.1e-07
  bn_c1_b8_hw256_w2          stats sum                        1.9e-08   1.1e-07     1.1e-08   5.9e-08
  bn_c1_b8_hw256_w2          stats M2                         3.2e-08   5.4e-08     1.8e-08   3.1e-08
  bn_c1_b8_hw256_w2          save mean                        4.7e-08   7.3e-08     2.3e-08   3.7e-08
  bn_c1_b8_hw256_w2          save invstd                      7.4e-08   4.4e-08     3.7e-08   2.2e-08
  bn_c1_b8_hw256_w2          y                                7.7e-08   3.4e-08     1.5e-07   1.4e-07
  bn_c1_b8_hw256_w2          running_mean                     1.7e-08   1.7e-08     8.6e-09   8.6e-09
  bn_c1_b8_hw256_w2          running_var                      1.0e-08   1.0e-08     5.1e-09   5.1e-09
  bn_c1_b8_hw256_w2          sums dz (dbeta share)            1.1e-07   2.7e-08     5.8e-08   1.6e-08
  bn_c1_b8_hw256_w2          sums dz*xhat (dgamma share)      9.0e-08   3.9e-08     5.0e-08   3.0e-08
  bn_c1_b8_hw256_w2          dyr                              1.0e-07   1.0e-07     1.3e-07   1.4e-07
  bn_c64_b32_hw64_w1         stats sum                        1.3e-07   9.0e-08     1.3e-07   6.7e-08
  bn_c64_b32_hw64_w1         stats M2                         1.4e-07   7.9e-08     1.3e-07   5.4e-08
  bn_c64_b32_hw64_w1         save mean                        1.3e-07   9.0e-08     1.3e-07   6.7e-08
  bn_c64_b32_hw64_w1         save invstd                      1.4e-07   8.6e-08     9.1e-08   5.4e-08
  bn_c64_b32_hw64_w1         y                                1.9e-07   1.3e-07     2.4e-07   5.2e-07
  bn_c64_b32_hw64_w1         running_mean                     1.2e-07   9.6e-08     1.2e-07   8.8e-08
  bn_c64_b32_hw64_w1         running_var                      4.1e-08   5.6e-08     2.6e-08   3.7e-08
  bn_c64_b32_hw64_w1         sums dz (dbeta share)            1.8e-07   5.0e-08     3.0e-07   3.5e-08
  bn_c64_b32_hw64_w1         sums dz*xhat (dgamma share)      4.1e-07   4.3e-08     3.0e-07   8.4e-08
  bn_c64_b32_hw64_w1         dyr                              2.3e-07   1.3e-07     2.6e-07   2.0e-07
  bn_c64_b3_hw683_w2         stats sum                        5.0e-08   6.8e-08     5.7e-08   7.6e-08
  bn_c64_b3_hw683_w2         stats M2                         7.8e-08   7.8e-08     6.7e-08   6.7e-08
  bn_c64_b3_hw683_w2         save mean                        7.3e-08   5.5e-08     6.7e-08   4.6e-08
  bn_c64_b3_hw683_w2         save invstd                      8.5e-08   9.4e-08     5.8e-08   6.9e-08
  bn_c64_b3_hw683_w2         y                                1.3e-07   1.1e-07     2.7e-07   3.0e-07
  bn_c64_b3_hw683_w2         running_mean                     7.3e-08   6.2e-08     8.4e-08   6.5e-08
  bn_c64_b3_hw683_w2         running_var                      3.9e-08   8.4e-08     2.8e-08   5.8e-08
  bn_c64_b3_hw683_w2         sums dz (dbeta share)            1.1e-07   2.9e-08     2.1e-07   2.8e-08
  bn_c64_b3_hw683_w2         sums dz*xhat (dgamma share)      1.7e-07   9.9e-08     2.0e-07   1.5e-07
  bn_c64_b3_hw683_w2         dyr                              1.4e-07   8.3e-08     2.1e-07   1.8e-07
  bn_c256_b32_hw64_w2        stats sum                        1.2e-07   9.1e-08     1.4e-07   7.2e-08
  bn_c256_b32_hw64_w2        stats M2                         2.0e-07   8.6e-08     1.6e-07   7.5e-08
  bn_c256_b32_hw64_w2        save mean                        1.7e-07   7.6e-08     1.5e-07   5.8e-08
  bn_c256_b32_hw64_w2        save invstd                      1.2e-07   8.7e-08     9.5e-08   5.8e-08
  bn_c256_b32_hw64_w2        y                                1.6e-07   8.8e-08     7.3e-07   3.3e-07
  bn_c256_b32_hw64_w2        running_mean                     1.2e-07   6.2e-08     1.9e-07   7.5e-08
  bn_c256_b32_hw64_w2        running_var                      8.2e-08   8.0e-08     5.4e-08   5.4e-08
  bn_c256_b32_hw64_w2        sums dz (dbeta share)            2.3e-07   3.7e-08     3.6e-07   3.5e-08
  bn_c256_b32_hw64_w2        sums dz*xhat (dgamma share)      2.8e-07   1.4e-07     7.1e-07   1.6e-07
  bn_c256_b32_hw64_w2        dyr                              1.7e-07   1.3e-07     2.6e-07   2.1e-07
  bn_c256_b2_hw16_w1         stats sum                        7.3e-08   6.8e-08     8.1e-08   5.5e-08
  bn_c256_b2_hw16_w1         stats M2                         6.0e-08   5.0e-08     7.7e-08   6.0e-08
  bn_c256_b2_hw16_w1         save mean                        7.3e-08   6.8e-08     8.1e-08   5.5e-08
  bn_c256_b2_hw16_w1         save invstd                      1.0e-07   7.0e-08     7.7e-08   6.3e-08
  bn_c256_b2_hw16_w1         y                                1.1e-07   1.3e-07     4.5e-07   5.5e-07
  bn_c256_b2_hw16_w1         running_mean                     7.6e-08   8.1e-08     1.1e-07   1.1e-07
  bn_c256_b2_hw16_w1         running_var                      6.5e-08   7.7e-08     4.4e-08   5.0e-08
  bn_c256_b2_hw16_w1         sums dz (dbeta share)            8.4e-08   3.3e-08     1.4e-07   3.6e-08
  bn_c256_b2_hw16_w1         sums dz*xhat (dgamma share)      1.2e-07   1.3e-07     2.2e-07   1.8e-07
  bn_c256_b2_hw16_w1         dyr                              8.8e-08   1.2e-07     2.1e-07   3.7e-07
  bn_c1024_b32_hw4_w1        stats sum                        1.5e-07   7.1e-08     1.4e-07   6.5e-08
  bn_c1024_b32_hw4_w1        stats M2                         1.8e-07   8.8e-08     1.6e-07   7.9e-08
  bn_c1024_b32_hw4_w1        save mean                        1.5e-07   7.1e-08     1.4e-07   6.5e-08
  bn_c1024_b32_hw4_w1        save invstd                      1.6e-07   1.1e-07     1.2e-07   8.1e-08
  bn_c1024_b32_hw4_w1        y                                1.9e-07   1.2e-07     1.4e-06   4.8e-07
  bn_c1024_b32_hw4_w1        running_mean                     1.7e-07   7.1e-08     2.0e-07   1.2e-07
  bn_c1024_b32_hw4_w1        running_var                      6.0e-08   9.1e-08     4.9e-08   6.1e-08
  bn_c1024_b32_hw4_w1        sums dz (dbeta share)            1.9e-07   3.5e-08     2.6e-07   3.9e-08
  bn_c1024_b32_hw4_w1        sums dz*xhat (dgamma share)      2.4e-07   1.1e-07     3.7e-07   2.2e-07
  bn_c1024_b32_hw4_w1        dyr                              1.5e-07   1.3e-07     3.3e-07   2.3e-07
  bn_c1100_b5_hw7_w2         stats sum                        9.7e-08   7.0e-08     9.1e-08   8.7e-08
  bn_c1100_b5_hw7_w2         stats M2                         7.8e-08   6.1e-08     9.8e-08   9.2e-08
  bn_c1100_b5_hw7_w2         save mean                        8.9e-08   6.5e-08     1.1e-07   7.1e-08
  bn_c1100_b5_hw7_w2         save invstd                      1.2e-07   1.1e-07     8.3e-08   1.1e-07
  bn_c1100_b5_hw7_w2         y                                1.5e-07   1.6e-07     5.3e-07   5.1e-07
  bn_c1100_b5_hw7_w2         running_mean                     8.9e-08   8.2e-08     1.5e-07   1.7e-07
  bn_c1100_b5_hw7_w2         running_var                      6.2e-08   8.0e-08     4.4e-08   5.8e-08
  bn_c1100_b5_hw7_w2         sums dz (dbeta share)            8.7e-08   3.2e-08     1.7e-07   3.8e-08
  bn_c1100_b5_hw7_w2         sums dz*xhat (dgamma share)      2.1e-07   1.4e-07     4.2e-07   2.8e-07
  bn_c1100_b5_hw7_w2         dyr                              1.5e-07   1.4e-07     2.5e-07   2.4e-07
  bn_c64_b32_hw4096_w2       stats sum                        1.6e-07   8.1e-08     1.2e-07   8.9e-08
  bn_c64_b32_hw4096_w2       stats M2                         1.4e-07   7.3e-08     1.1e-07   5.2e-08
  bn_c64_b32_hw4096_w2       save mean                        1.7e-07   6.8e-08     1.7e-07   7.0e-08
  bn_c64_b32_hw4096_w2       save invstd                      9.7e-08   9.4e-08     8.7e-08   6.1e-08
  bn_c64_b32_hw4096_w2       y                                1.8e-07   9.0e-08     5.5e-07   2.0e-07
  bn_c64_b32_hw4096_w2       running_mean                     1.3e-07   6.4e-08     2.7e-07   1.2e-07
  bn_c64_b32_hw4096_w2       running_var                      6.4e-08   7.2e-08     4.7e-08   4.9e-08
  bn_c64_b32_hw4096_w2       sums dz (dbeta share)            1.8e-07   3.5e-08     2.7e-07   3.7e-08
  bn_c64_b32_hw4096_w2       sums dz*xhat (dgamma share)      2.3e-07   9.1e-08     3.8e-07   1.2e-07
  bn_c64_b32_hw4096_w2       dyr                              1.7e-07   1.3e-07     2.7e-07   1.9e-07
  bn_c7_b1_hw2049_w1         stats sum                        4.2e-08   4.2e-08     2.9e-08   3.0e-08
  bn_c7_b1_hw2049_w1         stats M2                         5.8e-08   1.1e-07     4.0e-08   6.9e-08
  bn_c7_b1_hw2049_w1         save mean                        8.6e-08   8.6e-08     6.0e-08   6.0e-08
  bn_c7_b1_hw2049_w1         save invstd                      1.3e-07   2.7e-08     7.7e-08   2.2e-08
  bn_c7_b1_hw2049_w1         y                                1.0e-07   5.9e-08     1.7e-07   2.4e-07
  bn_c7_b1_hw2049_w1         running_mean                     1.2e-07   8.3e-08     1.0e-07   7.1e-08
  bn_c7_b1_hw2049_w1         running_var                      3.6e-08   3.6e-08     2.1e-08   2.3e-08
  bn_c7_b1_hw2049_w1         sums dz (dbeta share)            7.3e-08   5.1e-08     1.1e-07   3.4e-08
  bn_c7_b1_hw2049_w1         sums dz*xhat (dgamma share)      7.2e-08   7.2e-08     7.8e-08   6.8e-08
  bn_c7_b1_hw2049_w1         dyr                              1.4e-07   7.5e-08     2.2e-07   1.3e-07
  MEASURED_TABLE_END
"""
import contextlib
import ctypes
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import metrics_oracle as MO
from oracle import mixstage_oracle as O
from oracle import prestep_oracle as PO
from helpers.ew_table import TABLE

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FLOOR = 2.0 * 2.0 ** -24
KINK_MAX = 8
BIG = 4_000_000               # elements above which the float64 reference runs on the device (float64 arithmetic either way)


def f32(v):
  return float(np.float32(v))


@contextlib.contextmanager
def _timed(labels):
  from mix_stage_amd import ops
  ops.timing_enable(True)
  try:
    yield
    torch.cuda.synchronize()
    labels.extend(r['label'] for r in ops.timing_report())
  finally:
    ops.timing_enable(False)


def _gen(e, salt=0):
  return torch.Generator().manual_seed((zlib.crc32(e['id'].encode()) + salt) % 100000)


def _two_metrics(got, ref):
  got = got.detach().to(DEV).double().reshape(-1)
  ref = ref.detach().to(DEV).double().reshape(-1)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  assert bool(torch.isfinite(got).all()), 'non-finite values in the device result'
  d = (got - ref).abs()
  rms = ref.pow(2).mean().sqrt()
  return (d.max() / (ref.abs().max() + 1e-30)).item(), (d / (ref.abs() + rms + 1e-30)).max().item()


class Checks:
  """Collects (name, measured, bar) rows; prints them; asserts at the end so that one run shows every figure."""

  def __init__(self, e):
    self.e, self.rows = e, []

  def fixed(self, name, got, ref, bar):
    mx, el = _two_metrics(got, ref)
    self.rows += [(name + ' max', mx, bar, None), (name + ' elem', el, bar, None)]

  def derived(self, name, got, ref, ref32):
    mx, el = _two_metrics(got, ref)
    ymx, yel = _two_metrics(ref32, ref)
    self.rows += [(name + ' max', mx, 4 * max(ymx, FLOOR), ymx), (name + ' elem', el, 4 * max(yel, FLOOR), yel)]

  def exact(self, name, got, ref):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    ok = got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(got, ref)
    self.rows.append((name + ' exact', 0.0 if ok else float('inf'), 0.0, None))

  def true(self, name, cond):
    self.rows.append((name, 0.0 if cond else float('inf'), 0.0, None))

  def atmost(self, name, value, bar):
    self.rows.append((name, float(value), float(bar), None))

  def finish(self):
    for name, v, bar, yard in self.rows:
      print('EW %-28s %-34s yardstick %-10s device %.3e bar %.3e' % (self.e['id'], name, '-' if yard is None else '%.3e' % yard, v, bar))
    bad = [(n, v, b) for n, v, b, _ in self.rows if not v <= b]
    assert not bad, '%s: (check, measured, bar) %s' % (self.e['id'], bad)


def _lib():
  from mix_stage_amd import _lib as L
  return L.lib()


def _p(t):
  return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ softmax mixture
def run_softmax_mix(e, ck, labels):
  from mix_stage_amd import ops
  B, M, P, T = (e['p'][k] for k in 'BMPT')
  gen = _gen(e)
  off = torch.randn(M * P, generator=gen) * 2                       # per-(m, f) offset: a swapped index changes the result by O(1)
  z = torch.randn(B, M * P, T, generator=gen) + off.reshape(1, -1, 1)
  sc = torch.randn(B, M, T, generator=gen) * 3 + torch.randn(M, 1, generator=gen) * 2     # far from uniform
  gy = torch.randn(B, T, P, generator=gen)

  def ref(dtype, dev):
    z_, s_ = z.to(dev, dtype).requires_grad_(), sc.to(dev, dtype).requires_grad_()
    soft = torch.softmax(s_.transpose(2, 1), dim=-1)
    out = O.mix_outputs(z_, soft, M)
    out.backward(gy.to(dev, dtype))
    return out.detach(), soft.detach(), z_.grad, s_.grad

  zh, sh = z.to(DEV).requires_grad_(), sc.to(DEV).requires_grad_()
  with _timed(labels):
    out, soft = ops.softmax_mix(zh, sh, P)
    out.backward(gy.to(DEV))
  r_out, r_soft, r_dz, r_ds = ref(torch.float64, DEV if z.numel() > BIG else 'cpu')
  ck.true('shapes', out.shape == (B, T, P) and soft.shape == (B, T, M))
  ck.fixed('out', out, r_out, 1e-5)
  ck.fixed('soft', soft, r_soft, 1e-5)
  ck.fixed('dz', zh.grad, r_dz, 1e-5)
  if e['bar'] == 'derived':
    ck.derived('dscore', sh.grad, r_ds, ref(torch.float32, 'cpu')[3])
  else:
    ck.fixed('dscore', sh.grad, r_ds, 1e-5)


# ------------------------------------------------------------------------------------------------ cross entropy
def run_cross_entropy(e, ck, labels):
  from mix_stage_amd import ops
  p = e['p']
  C, layout, shape = p['C'], p['layout'], p['shape']
  gen = _gen(e)
  rows = int(np.prod(shape))
  if layout == 'bct':
    sc = torch.randn(shape[0], C, shape[1], generator=gen) * 3 + torch.randn(1, C, 1, generator=gen) * 2
  else:
    sc = torch.randn(shape[0], C, generator=gen) * 3 + torch.randn(1, C, generator=gen) * 2
  tg = torch.randint(0, C, (rows,), generator=gen)
  tg[torch.randperm(rows, generator=gen)[:C]] = torch.arange(C)                 # every class is a target
  tg = tg.reshape(shape)
  assert len(torch.unique(tg)) == C
  dout = 0.7
  lam = torch.tensor([0.37], device=DEV)
  w = {'host': f32(0.37), 'dev': f32(0.37), 'none': 1.0}[p['scale']]
  d0 = torch.randn(sc.shape, generator=gen) * 0.01                               # what accumulate = 1 adds to

  def ref(dtype):
    s_ = sc.to(dtype).requires_grad_()
    l = w * F.cross_entropy(s_.transpose(2, 1).reshape(-1, C) if layout == 'bct' else s_, tg.reshape(-1))
    (l * f32(dout)).backward()
    return l.detach(), s_.grad + (d0.to(dtype) if p['accumulate'] else 0)

  with _timed(labels):
    if e['via'] == 'lib':
      L = _lib()
      s_d, t_d = sc.to(DEV), tg.to(DEV)
      dims = (shape[0], shape[1], C, C * shape[1], shape[1], 1) if layout == 'bct' else (rows, 1, C, C, 1, 1)
      loss = torch.empty((), device=DEV)
      gs = torch.tensor([dout], device=DEV)
      grad = d0.to(DEV)
      assert L.ms_cross_entropy_fwd(_p(s_d), _p(t_d), _p(loss), None, *dims, _stream()) == 0
      assert L.ms_cross_entropy_bwd(_p(s_d), _p(t_d), _p(gs), _p(grad), *dims, 1, _stream()) == 0
    else:
      sh = sc.to(DEV).requires_grad_()
      if p['scale'] == 'dev':
        loss = ops._CrossEntropyFn.apply(sh, tg.to(DEV), layout, lam[0])         # a device-resident weight (ms_loss_scale.scale_dev)
      else:
        loss = ops.cross_entropy(sh, tg.to(DEV), layout=layout, scale=0.37)
      (loss * dout).backward()
      grad = sh.grad
  r_l, r_g = ref(torch.float64)
  if e['bar'] == 'derived':
    y_l, _ = ref(torch.float32)
    ck.derived('loss', loss.reshape(1), r_l.reshape(1), y_l.reshape(1))
  else:
    ck.fixed('loss', loss.reshape(1), r_l.reshape(1), 1e-6)
  ck.fixed('dscore', grad, r_g, 1e-5)


# ------------------------------------------------------------------------------------------------ L1 / MSE
def run_lp_mean(e, ck, labels):
  from mix_stage_amd import ops
  n, sq = e['p']['n'], e['p']['squared']
  gen = _gen(e)
  a = torch.randn(n, generator=gen) * 2 + 0.5
  b = torch.randn(n, generator=gen)
  target = 0.75
  a[0] = b[0]                                   # a difference of exactly 0: sign(0) = 0 in the L1 gradient
  at = a.clone(); at[0] = target
  lam = torch.tensor([1.83], device=DEV)
  dout = 0.6
  fn = ops.l2_mean if sq else ops.l1_mean

  def ref(x, other, w):
    x_ = x.double().requires_grad_()
    d = x_ - other
    l = w * ((d * d).mean() if sq else d.abs().mean())
    (l * f32(dout)).backward()
    return l.detach(), x_.grad

  got = []
  with _timed(labels):
    if e['p']['plain']:
      L = _lib()
      nm = 'l2' if sq else 'l1'
      part = torch.empty(L.ms_reduce_partials_count(n), device=DEV)
      gs = torch.tensor([dout], device=DEV)
      for x, other in ((a, b), (at, None)):
        xd, od = x.to(DEV), (None if other is None else other.to(DEV))
        loss, da = torch.empty((), device=DEV), torch.empty(n, device=DEV)
        assert getattr(L, 'ms_%s_mean_fwd' % nm)(_p(xd), _p(od), target, _p(loss), _p(part), n, _stream()) == 0
        assert getattr(L, 'ms_%s_mean_bwd' % nm)(_p(xd), _p(od), target, _p(gs), _p(da), n, _stream()) == 0
        got.append((loss, da))
      ws = (1.0, 1.0)
    else:
      x1 = a.to(DEV).requires_grad_()
      l1 = fn(x1, b.to(DEV), scale=lam[0]); (l1 * dout).backward()
      x2 = at.to(DEV).requires_grad_()
      l2 = fn(x2, target=target, scale=1.7); (l2 * dout).backward()
      got = [(l1, x1.grad), (l2, x2.grad)]
      ws = (f32(1.83), f32(1.7))
  for name, (l, g), (x, other), w in zip(('with b', 'with target'), got, ((a, b.double()), (at, f32(target))), ws):
    r_l, r_g = ref(x, other, w)
    ck.fixed('loss ' + name, l.reshape(1), r_l.reshape(1), 1e-6)
    ck.fixed('grad ' + name, g, r_g, 1e-6)
    ck.true('grad at d == 0 is 0 ' + name, float(g[0]) == 0.0)


def run_lp_pair(e, ck, labels):
  from mix_stage_amd import ops
  n = e['p']['n']
  gen = _gen(e)
  a = torch.randn(2 * n, generator=gen) + 0.3
  a[0] = 0.0                                    # exactly on its target
  lam = torch.tensor([0.37], device=DEV)
  with _timed(labels):
    got = {}
    for sq in (False, True):
      x = a.to(DEV).requires_grad_()
      p0, p1 = ops.lp_mean_pair(x, (0.0, 1.0), (lam[0], 0.5), squared=sq)
      (p0 * 0.8 + p1 * 1.3).backward()
      got[sq] = (p0, p1, x.grad)
  for sq in (False, True):
    x_ = a.double().requires_grad_()
    d0, d1 = x_[:n] - 0.0, x_[n:] - 1.0
    r0 = f32(0.37) * ((d0 * d0).mean() if sq else d0.abs().mean())
    r1 = 0.5 * ((d1 * d1).mean() if sq else d1.abs().mean())
    (r0 * f32(0.8) + r1 * f32(1.3)).backward()
    nm = 'l2' if sq else 'l1'
    ck.fixed(nm + ' loss0', got[sq][0].reshape(1), r0.detach().reshape(1), 1e-6)
    ck.fixed(nm + ' loss1', got[sq][1].reshape(1), r1.detach().reshape(1), 1e-6)
    ck.fixed(nm + ' grad', got[sq][2], x_.grad, 1e-6)


def run_lp_pair_refused(e, ck, labels):
  L = _lib()
  from mix_stage_amd._lib import LossScale
  n = e['p']['n']
  a = torch.randn(2 * n, generator=_gen(e)).to(DEV)
  out = torch.full((2,), -7.0, device=DEV)
  da = torch.full((2 * n,), -7.0, device=DEV)
  g = torch.ones(1, device=DEV)
  tg = (ctypes.c_float * 2)(0.0, 1.0)
  ls = (LossScale * 2)(LossScale(1.0, None), LossScale(1.0, None))
  with _timed(labels):
    for sq in (0, 1):
      ck.true('fwd refused sq%d' % sq, L.ms_lp_mean_pair_fwd(sq, _p(a), tg, _p(out), n, _stream(), ls) != 0)
      ck.true('bwd refused sq%d' % sq, L.ms_lp_mean_pair_bwd(sq, _p(a), tg, _p(g), _p(g), _p(da), n, _stream(), ls) != 0)
  ck.true('outputs untouched', bool((out == -7.0).all()) and bool((da == -7.0).all()))


# ------------------------------------------------------------------------------------------------ gradient norm
def run_sqnorm(e, ck, labels):
  from mix_stage_amd import ops
  n = e['p']['n']
  gen = _gen(e)
  g = torch.randn(n, generator=gen) * 3
  g[: max(1, n // 50)] *= 40                     # no element class is negligible: a dropped vector or tail shows
  g[-1] = 25.0
  ref = g.double().pow(2).sum().sqrt().reshape(1)
  y32 = (g * g).sum().sqrt().reshape(1)
  L = _lib()
  part = torch.zeros(L.ms_reduce_partials_count(n), device=DEV)
  buf_a = torch.empty(n + 4, device=DEV)
  buf_u = torch.empty(n + 4, device=DEV)
  assert buf_a.data_ptr() % 16 == 0 and buf_u.data_ptr() % 16 == 0
  al, un = buf_a[:n], buf_u[1:n + 1]
  al.copy_(g); un.copy_(g)
  assert un.data_ptr() % 16 == 4
  o_a, o_u = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
  with _timed(labels):
    ops.grad_norm(al, o_a, part)
    ops.grad_norm(un, o_u, part)
  ck.derived('aligned', o_a, ref, y32)
  ck.derived('offset by one float', o_u, ref, y32)


# ------------------------------------------------------------------------------------------------ Adam
def _adam_segments(kind, n, gen):
  """-> (seg_of_chunk int32 (n / 64), seg_first int32 (n_seg))"""
  nchunk = n // 64
  firsts = [1, 2, 3, -1, 9]
  if kind == 'one':
    return torch.zeros(max(1, nchunk), dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
  if kind == 'chunks':
    return torch.arange(nchunk, dtype=torch.int32), torch.tensor([firsts[i % 5] for i in range(nchunk)], dtype=torch.int32)
  cuts = torch.sort(torch.randperm(nchunk - 1, generator=gen)[:36] + 1).values.tolist()
  seg = torch.zeros(nchunk, dtype=torch.int32)
  for c in cuts:
    seg[c:] += 1
  return seg, torch.tensor([firsts[i % 5] for i in range(37)], dtype=torch.int32)


def _adam_reference(dtype, p0, m0, v0, grads, norms32, max_norms, first, hp):
  """torch.optim.Adam (no amsgrad, no weight decay) with clip_grad_norm_ folded in and one step count per element:
  t = step - first + 1; elements whose first step is -1 or in the future are skipped; a non-finite norm skips the step."""
  lr, b1, b2, eps = hp
  p, m, v = p0.to(dtype).clone(), m0.to(dtype).clone(), v0.to(dtype).clone()
  for s, (g, nrm, mx) in enumerate(zip(grads, norms32, max_norms), start=1):
    if nrm is None:
      coef = torch.ones((), dtype=dtype)
    else:
      if not math.isfinite(nrm):
        continue
      coef = torch.clamp(torch.tensor(mx, dtype=dtype) / (torch.tensor(nrm, dtype=dtype) + torch.tensor(f32(1e-6), dtype=dtype)), max=1.0)
    act = (first >= 1) & (first <= s)
    t = (s - first + 1).clamp(min=1).double()
    step_size = (lr / (1.0 - b1 ** t)).to(dtype)                   # (python-double arithmetic cast once, as torch.optim.Adam does)
    bc2s = (1.0 - b2 ** t).sqrt().to(dtype)
    gi = g.to(dtype) * coef
    mn = m + (1.0 - b1) * (gi - m)
    vn = b2 * v + (1.0 - b2) * gi * gi
    pn = p - step_size * (mn / (vn.sqrt() / bc2s + eps))
    p, m, v = torch.where(act, pn, p), torch.where(act, mn, m), torch.where(act, vn, v)
  return p, m, v


def run_adam(e, ck, labels):
  from mix_stage_amd import ops
  pp = e['p']
  n, segmented = pp['n'], pp['segmented']
  gen = _gen(e)
  hp = (f32(1e-3), f32(0.9), f32(0.999), f32(1e-8))
  lr, b1, b2, eps = hp
  p0 = torch.randn(n, generator=gen) * 0.1
  p0[::7] *= 1e-4                                                  # near-zero weights
  m0 = torch.randn(n, generator=gen) * 0.01
  v0 = torch.rand(n, generator=gen) * 1e-4
  if segmented:
    seg, sfirst = _adam_segments(pp['seg'], n, gen)
    first = sfirst.long()[seg.long()].repeat_interleave(64)
  else:
    first = torch.ones(n, dtype=torch.long)
  grads, norms32, max_norms = [], [], []
  for kind in pp['norms']:
    g = torch.randn(n, generator=gen) * 0.02 * torch.exp(torch.randn(n, generator=gen))
    true = f32(g.double().norm().item())
    grads.append(g)
    norms32.append({'in': true, 'clip': true, 'inf': float('inf'), 'nan': float('nan'), 'none': None}[kind])
    max_norms.append(f32(true * (0.25 if kind == 'clip' else 1.5)))

  def device_run(offset):
    def buf(src):
      if offset:
        t = torch.empty(n + 4, device=DEV)[1:n + 1]
        assert t.data_ptr() % 16 == 4
      else:
        t = torch.empty(n, device=DEV)
        assert t.data_ptr() % 16 == 0
      t.copy_(src)
      return t
    p, m, v = buf(p0), buf(m0), buf(v0)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    if segmented:
      seg_d, first_d = seg.to(DEV), sfirst.to(DEV)
      scratch = torch.zeros(2 * sfirst.numel(), device=DEV)
    events, bad = [], 0
    for s, (g, nrm, mx) in enumerate(zip(grads, norms32, max_norms), start=1):
      gd = buf(g)
      nd = None if nrm is None else torch.tensor([nrm], device=DEV)
      before = (p.clone(), m.clone(), v.clone())
      if segmented:
        ops.adam_step_segmented(p, gd, m, v, nd, mx, lr, b1, b2, eps, state, seg_d, first_d, scratch)
      else:
        ops.adam_step(p, gd, m, v, nd, mx, lr, b1, b2, eps, state)
      st = state.cpu()
      events.append(int(st[0]) == s)
      if segmented and nrm is not None:
        isbad = not math.isfinite(nrm)
        bad += isbad
        events.append(int(st[2]) == (1 if isbad else 0) and int(st[3]) == bad)
        if isbad:
          events.append(all(torch.equal(x, y) for x, y in zip(before, (p, m, v))))
    return p, m, v, all(events)

  with _timed(labels):
    p, m, v, ok = device_run(False)
    if pp['offset']:
      po, mo, vo, ok_o = device_run(True)
  ck.true('step clock, skip flag, skip counter, refused steps bit-unchanged', ok)
  ref = _adam_reference(torch.float64, p0, m0, v0, grads, norms32, max_norms, first, hp)
  y32 = _adam_reference(torch.float32, p0, m0, v0, grads, norms32, max_norms, first, hp)
  steps = len(grads)
  never = ~((first >= 1) & (first <= steps))
  if segmented and bool(never.any()):
    for nm, got, init in (('p', p, p0), ('m', m, m0), ('v', v, v0)):
      ck.exact(nm + ' of segments never updated', got.cpu()[never], init[never])
  for nm, got, r, y in zip('pmv', (p, m, v), ref, y32):
    ck.derived(nm, got, r, y)
  if pp['offset']:
    ck.true('offset run: clock and flags', ok_o)
    for nm, a, b, r, y in zip('pmv', (po, mo, vo), (p, m, v), ref, y32):
      ck.exact(nm + ' offset-by-one-float views vs aligned', a.contiguous(), b)
      ck.derived(nm + ' offset', a, r, y)


# ------------------------------------------------------------------------------------------------ time resize
def run_lerp(e, ck, labels):
  from mix_stage_amd import ops
  B, C, Tin, F_, Tout = (e['p'][k] for k in ('B', 'C', 'Tin', 'F', 'Tout'))
  gen = _gen(e)
  x = torch.randn(B, C, Tin, F_, generator=gen) + torch.arange(F_).float() * 0.5      # columns differ: a wrong column shows
  gy = torch.randn(B, C, Tout, generator=gen)
  xh = x.to(DEV).requires_grad_()
  with _timed(labels):
    y = ops.lerp_time(xh, Tout)
    y.backward(gy.to(DEV))
  dev = DEV if x.numel() > BIG else 'cpu'
  x64 = x.double().to(dev).requires_grad_()
  y_ref = F.interpolate(x64, size=(Tout, 1), mode='bilinear').squeeze(-1)
  y_ref.backward(gy.double().to(dev))
  ck.fixed('y', y, y_ref, 1e-6)
  ck.fixed('dx', xh.grad, x64.grad, 1e-6)


# ------------------------------------------------------------------------------------------------ concat
def run_concat(e, ck, labels):
  from mix_stage_amd import ops
  B, C, D, T, S = (e['p'][k] for k in 'BCDTS')
  gen = _gen(e)
  unused = 7
  x = torch.randn(B, C, T, generator=gen)
  E = torch.randn(S, D, generator=gen) + torch.arange(S).float().reshape(S, 1)
  ids = torch.randint(0, S - 1, (B, 1) if e['p']['per_clip'] else (B, T), generator=gen)
  ids[ids >= unused] += 1
  gy = torch.randn(B, C + D, T, generator=gen)
  xh, Eh = x.to(DEV).requires_grad_(), E.to(DEV).requires_grad_()
  idh = ids.to(DEV).expand(B, T)
  with _timed(labels):
    out = ops.concat_style(xh, Eh, idh)
    out.backward(gy.to(DEV))
  x64, E64 = x.double().requires_grad_(), E.double().requires_grad_()
  ref = torch.cat([x64, F.embedding(ids.expand(B, T), E64).transpose(2, 1)], dim=1)
  ref.backward(gy.double())
  ck.exact('out', out, ref.detach().float())
  ck.exact('dx', xh.grad, x64.grad.float())
  ck.fixed('demb', Eh.grad, E64.grad, 1e-6)
  ck.true('unused embedding row has gradient exactly 0', not bool(Eh.grad[unused].any()) and not bool((ids == unused).any()))


# ------------------------------------------------------------------------------------------------ velocity / transposes
def run_velocity(e, ck, labels):
  from mix_stage_amd import ops
  B, T, P = (e['p'][k] for k in 'BTP')
  gen = _gen(e)
  x = torch.randn(B, T, P, generator=gen)
  gy = torch.randn(B, P, T, generator=gen)
  xh = x.to(DEV).requires_grad_()
  with _timed(labels):
    v = ops.velocity_cm(xh)
    v.backward(gy.to(DEV))
    cm = ops.to_channel_major(x.to(DEV))
    tm = ops.to_time_major(cm)
  # one IEEE fp32 subtraction per element: torch's float32 CPU result is the correctly rounded float64 one
  xr = x.clone().requires_grad_()
  v_ref = torch.cat([torch.zeros_like(xr[:, 0:1]), xr[:, 1:] - xr[:, :-1]], dim=1).transpose(1, 2)
  v_ref.backward(gy)
  ck.exact('velocity', v, v_ref.detach().contiguous())
  ck.exact('velocity dx', xh.grad, xr.grad)
  ck.exact('to_channel_major', cm, x.transpose(1, 2).contiguous())
  ck.exact('to_time_major', tm, x)


# ------------------------------------------------------------------------------------------------ stand-alone BatchNorm
def run_bn_trio(e, ck, labels):
  L = _lib()
  C, B, HW, world = (e['p'][k] for k in ('C', 'B', 'HW', 'world'))
  gen = _gen(e)
  eps, mom, slope = f32(1e-5), f32(0.1), f32(0.2)
  cs, cm = torch.rand(1, C, 1, generator=gen) + 0.5, torch.randn(1, C, 1, generator=gen)
  shards = [(torch.randn(B, C, HW, generator=gen) * cs + cm) * (1.0 + 0.6 * r) + 0.3 * r for r in range(world)]
  dys = [torch.randn(B, C, HW, generator=gen) for _ in range(world)]
  gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
  rm0, rv0 = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5
  n_local, N = B * HW, world * B * HW
  xs, ds = [s.to(DEV) for s in shards], [d.to(DEV) for d in dys]
  g_d, b_d = gamma.to(DEV), beta.to(DEV)
  allstats = torch.empty(world, C, 2, device=DEV)
  ys, saves, rms, rvs, sums, dyrs = [], [], [], [], [], []
  ws = torch.empty(L.ms_bn_bwd_workspace(B, C), dtype=torch.uint8, device=DEV)
  with _timed(labels):
    for r in range(world):
      assert L.ms_bn_stats(_p(xs[r]), _p(allstats[r]), B, C, HW, _stream()) == 0
    for r in range(world):
      y, save = torch.empty_like(xs[r]), torch.empty(4 * C, device=DEV)
      rm, rv = rm0.to(DEV), rv0.to(DEV)
      assert L.ms_bn_train_apply(_p(allstats), world, n_local, _p(g_d), _p(b_d), _p(rm), _p(rv), _p(xs[r]), _p(y), _p(save), B, C, HW,
                                 eps, mom, slope, _stream()) == 0
      ys.append(y); saves.append(save); rms.append(rm); rvs.append(rv)
    for r in range(world):
      s = torch.empty(C, 2, device=DEV)
      assert L.ms_bn_bwd_sums(_p(ds[r]), _p(xs[r]), _p(saves[r]), _p(s), B, C, HW, slope, _p(ws), ws.numel(), _stream()) == 0
      sums.append(s)
    gsum = sums[0].clone()
    for r in range(1, world):
      gsum += sums[r]
    for r in range(world):
      dyr = torch.empty_like(xs[r])
      assert L.ms_bn_bwd_apply(_p(ds[r]), _p(xs[r]), _p(saves[r]), _p(g_d), _p(gsum), float(N), _p(dyr), B, C, HW, slope, _stream()) == 0
      dyrs.append(dyr)
  pos = torch.cat(ys) > 0

  def ref(dtype, dev):
    X = torch.cat(shards).to(dev, dtype).requires_grad_()
    g_, b_ = gamma.to(dev, dtype).reshape(1, C, 1), beta.to(dev, dtype).reshape(1, C, 1)
    loc_sum = torch.stack([X.detach()[r * B:(r + 1) * B].sum((0, 2)) for r in range(world)])
    loc_m2 = torch.stack([(X.detach()[r * B:(r + 1) * B] - (loc_sum[r] / n_local).reshape(1, C, 1)).pow(2).sum((0, 2)) for r in range(world)])
    mean = X.mean((0, 2), keepdim=True)
    var = (X - mean).pow(2).mean((0, 2), keepdim=True)
    invstd = 1.0 / (var + eps).sqrt()
    xhat = (X - mean) * invstd
    z = xhat * g_ + b_
    pz = pos.to(dev)
    y = torch.where(pz, z, slope * z)
    dy = torch.cat(dys).to(dev, dtype)
    y.backward(dy)
    dz = dy * torch.where(pz, torch.ones((), dtype=dtype, device=dev), torch.tensor(slope, dtype=dtype, device=dev))
    s1 = torch.stack([dz[r * B:(r + 1) * B].sum((0, 2)) for r in range(world)])
    s2 = torch.stack([(dz * xhat.detach())[r * B:(r + 1) * B].sum((0, 2)) for r in range(world)])
    unb = var.detach().reshape(C) * (N / (N - 1.0)) if N > 1 else var.detach().reshape(C)
    rm = rm0.to(dev, dtype) + mom * (mean.detach().reshape(C) - rm0.to(dev, dtype))
    rv = rv0.to(dev, dtype) + mom * (unb - rv0.to(dev, dtype))
    return dict(stat_sum=loc_sum, stat_m2=loc_m2, mean=mean.detach().reshape(C), invstd=invstd.detach().reshape(C), y=y.detach(), z=z.detach(),
                running_mean=rm, running_var=rv, sum_dz=s1, sum_dz_xhat=s2, dyr=X.grad)

  R = ref(torch.float64, DEV if N * C > BIG else 'cpu')
  Y = ref(torch.float32, 'cpu')
  flip = pos.to(R['z'].device) != (R['z'] > 0)
  ck.atmost('LeakyReLU kinks (count)', int(flip.sum()), KINK_MAX)
  ck.atmost('|z| at a kink / max|z|', (R['z'][flip].abs().max() / R['z'].abs().max()).item() if bool(flip.any()) else 0.0, 2e-5)
  ck.derived('stats sum', allstats[:, :, 0], R['stat_sum'], Y['stat_sum'])
  ck.derived('stats M2', allstats[:, :, 1], R['stat_m2'], Y['stat_m2'])
  ck.derived('save mean', saves[0][:C], R['mean'], Y['mean'])
  ck.derived('save invstd', saves[0][C:2 * C], R['invstd'], Y['invstd'])
  ck.derived('y', torch.cat(ys), R['y'], Y['y'])
  ck.derived('running_mean', rms[0], R['running_mean'], Y['running_mean'])
  ck.derived('running_var', rvs[0], R['running_var'], Y['running_var'])
  ck.derived('sums dz (dbeta share)', torch.stack([s[:, 0] for s in sums]), R['sum_dz'], Y['sum_dz'])
  ck.derived('sums dz*xhat (dgamma share)', torch.stack([s[:, 1] for s in sums]), R['sum_dz_xhat'], Y['sum_dz_xhat'])
  ck.derived('dyr', torch.cat(dyrs), R['dyr'], Y['dyr'])
  for r in range(1, world):
    ck.exact('rank %d holds the same statistics' % r, saves[r], saves[0])


# ------------------------------------------------------------------------------------------------ cb8
def _cb8_expect(x_cm, tdt):
  """fp32 channel-major (B, C, *sp) -> the cb8 tensor (B, C8, *sp, 8) of torch's own cast, pad channels zero."""
  B, C = x_cm.shape[:2]
  sp = tuple(x_cm.shape[2:])
  C8 = (C + 7) // 8
  pad = torch.zeros((B, C8 * 8) + sp)
  pad[:, :C] = x_cm
  return pad.reshape((B, C8, 8) + sp).movedim(2, -1).contiguous().to(tdt)


def _cb8_unpack(y, C):
  """cb8 (B, C8, *sp, 8) -> fp32 channel-major (B, C, *sp)."""
  B, C8 = y.shape[:2]
  sp = tuple(y.shape[2:-1])
  return y.float().movedim(-1, 2).reshape((B, C8 * 8) + sp)[:, :C].contiguous()


def _wide(shape, gen):
  return torch.randn(shape, generator=gen) * 10 ** (torch.rand(shape, generator=gen) * 5 - 3)     # 1e-3 .. 1e2: fp16 subnormals included


def run_cb8(e, ck, labels):
  from mix_stage_amd import ops16
  from mix_stage_amd._lib import MS_BF16, MS_F16
  C, B = e['p']['C'], e['p']['B']
  tdt, dt = (torch.bfloat16, MS_BF16) if e['p']['dt'] == 'bf16' else (torch.float16, MS_F16)
  gen = _gen(e)
  C8 = (C + 7) // 8
  with _timed(labels):
    for sp in [(t,) for t in e['p']['Ts']] + [(5, 7)]:
      tag = 'x'.join(map(str, sp))
      x = _wide((B, C) + sp, gen)
      dy16 = _wide((B, C8) + sp + (8,), gen).to(tdt)                 # pad channels of a gradient hold anything: they must be dropped
      xh = x.to(DEV).requires_grad_()
      y = ops16.to_cb8(xh, dt)
      y.backward(dy16.to(DEV))
      ck.exact('to_cb8 %s' % tag, y, _cb8_expect(x, tdt))
      ck.exact('to_cb8 backward %s' % tag, xh.grad, _cb8_unpack(dy16, C))
      y16 = dy16.to(DEV).requires_grad_()
      back = ops16.from_cb8(y16, C)
      dyp = _wide((B, C) + sp, gen)
      back.backward(dyp.to(DEV))
      ck.exact('from_cb8 %s' % tag, back, _cb8_unpack(dy16, C))
      ck.exact('from_cb8 backward %s' % tag, y16.grad, _cb8_expect(dyp, tdt))
      rep = x.to(tdt).float()
      ck.exact('round trip of representable values %s' % tag, ops16.from_cb8(ops16.to_cb8(rep.to(DEV), dt), C), rep)
    for T in e['p']['Ts']:
      xb = _wide((B, T, C), gen)
      dv16 = _wide((B, C8, T, 8), gen).to(tdt)
      for vel in (False, True):
        xh = xb.to(DEV).requires_grad_()
        y = ops16.btc_to_cb8(xh, dt, velocity=vel)
        y.backward(dv16.to(DEV))
        val = torch.cat([torch.zeros_like(xb[:, :1]), xb[:, 1:] - xb[:, :-1]], dim=1) if vel else xb      # fp32 difference, rounded once below
        ck.exact('btc_to_cb8 T%d velocity%d' % (T, vel), y, _cb8_expect(val.transpose(1, 2).contiguous(), tdt))
        dv = _cb8_unpack(dv16, C).transpose(1, 2).contiguous()                                           # (B, T, C) fp32 of 16-bit values
        if vel:
          cur = dv.clone(); cur[:, 0] = 0
          nxt = torch.cat([dv[:, 1:], torch.zeros_like(dv[:, :1])], dim=1)
          dx = cur - nxt
        else:
          dx = dv
        ck.exact('btc_to_cb8 backward T%d velocity%d' % (T, vel), xh.grad, dx)
        ck.true('shapes T%d velocity%d' % (T, vel), y.shape == (B, C8, T, 8) and y.dtype == tdt and xh.grad.shape == (B, T, C))


# ------------------------------------------------------------------------------------------------ pre-step, metrics
FEAT_NAMES = ('pose', 'velocity', 'speed')


def _prestep_inputs(B, T, M, feats, seed):
  rng = np.random.default_rng(seed)
  P, F_ = 104, 128
  pose = (rng.standard_normal((B, 1, P)) * 40 + 100 + np.cumsum(rng.standard_normal((B, T, P)), axis=1)).astype(np.float32)
  audio = rng.standard_normal((B, T, F_)).astype(np.float32) * 3 - 20
  mask = [0, 7, 8, 9]
  PK = P - 2 * len(mask)
  blocks = {'pose': rng.standard_normal((M, PK)) * 40 + 100, 'velocity': rng.standard_normal((M, PK)), 'speed': np.abs(rng.standard_normal((M, PK // 2))) * 1.3}
  centers = np.concatenate([blocks[f] for f in feats], axis=1)
  pm, pv = rng.standard_normal(P) * 10 + 100, rng.random(P) * 50 + 1
  pv[5], pv[11] = 0.0, -1e-9
  am, av = rng.standard_normal(F_), rng.random(F_) * 4 + 0.1
  return pose, audio, centers, pm, pv, am, av, mask


def run_prestep(e, ck, labels):
  from mix_stage_amd.prestep import DevicePreStep
  B, T, M, bits = (e['p'][k] for k in ('B', 'T', 'M', 'feats'))
  feats = tuple(f for i, f in enumerate(FEAT_NAMES) if bits >> i & 1)
  pose, audio, centers, pm, pv, am, av, mask = _prestep_inputs(B, T, M, feats, zlib.crc32(e['id'].encode()) % 100000)
  pre = DevicePreStep(centers, pm, pv, am, av, mask=mask, feats=feats)
  with _timed(labels):
    a, lab, y = pre(torch.from_numpy(pose).cuda(), torch.from_numpy(audio).cuda())
  kept = PO.remove_joints(pose, mask)
  l_ref = np.concatenate([PO.kmeans_predict(kept[i:i + 64], centers, feats) for i in range(0, B, 64)])
  y_ref = PO.remove_joints(PO.znorm(pose, pm, pv), mask).astype(np.float32)
  a_ref = PO.znorm(audio, am, av).astype(np.float32)
  ck.exact('labels', lab, torch.from_numpy(l_ref))
  ck.true('every centre is some frame\'s label or M = 25', M == 25 or len(np.unique(l_ref)) > 1)
  for nm, got, r in (('pose znorm', y, y_ref), ('audio znorm', a, a_ref)):
    got = got.cpu().numpy()
    ck.atmost(nm + ' max rel (one rounding of the fp64 value, bar of test_prestep)', np.max(np.abs(got - r) / np.abs(r)), 2e-7)


def run_prestep_refused(e, ck, labels):
  L = _lib()
  B, T, P = 2, 8, 10
  pose = torch.randn(B, T, P, device=DEV)
  lab = torch.full((B, T), -5, dtype=torch.int64, device=DEV)
  with _timed(labels):
    for nm, PK, feats in (('odd PK with speed', 3, 5), ('feats = 0', 4, 0), ('feats = 8', 4, 8)):
      keep = torch.arange(PK, dtype=torch.int32, device=DEV)
      cen = torch.zeros(2, 3 * PK, dtype=torch.float64, device=DEV)
      ck.true(nm + ' refused', L.ms_kmeans_labels(_p(pose), _p(keep), _p(cen), _p(lab), B, T, P, PK, 2, feats, _stream()) != 0)
  ck.true('labels untouched', bool((lab == -5).all()))


def _metrics_inputs(B, T, seed):
  rng = np.random.default_rng(seed)
  P, mask = 104, [0, 7, 8, 9]
  gt = rng.standard_normal((B, T, P)).astype(np.float32)
  ycap = (gt.reshape(B, T, 2, 52)[..., [j for j in range(52) if j not in mask]].reshape(B, T, 96) + 0.15 * rng.standard_normal((B, T, 96))).astype(np.float32)
  mean, var = rng.standard_normal(P) * 20 + 100, rng.random(P) * 400 + 50
  return ycap, gt, mean, var, mask


def run_metrics(e, ck, labels):
  from mix_stage_amd.metrics import DeviceEvalAccumulators, DeviceStepMetrics
  B, T = e['p']['B'], e['p']['T']
  ycap, gt, mean, var, mask = _metrics_inputs(B, T, zlib.crc32(e['id'].encode()) % 100000)
  m = DeviceStepMetrics(mean, var, mask=mask)
  acc = DeviceEvalAccumulators(mean, var, mask=tuple(mask))
  with _timed(labels):
    got = m.update(torch.from_numpy(ycap).cuda(), torch.from_numpy(gt).cuda())
    for k in range(2):                                                                         # accumulation over two batches
      acc.update(torch.from_numpy(ycap * (1 + k)).cuda(), torch.from_numpy(gt * (1 + k)).cuda())
  ref = MO.step_metrics(ycap, gt, mean, var, mask)
  ck.atmost('L1 (bar of test_metrics)', abs(got['L1'] - ref['L1']), 1e-9)
  ck.atmost('VelL1 (bar of test_metrics)', abs(got['VelL1'] - ref['VelL1']), 1e-9)
  for a in (0.1, 0.2):
    ck.atmost('pck %s per joint' % a, np.abs(got['pck'][a][0].numpy() - ref['pck'][a][0]).max(), 1e-12)
    ck.atmost('pck %s mean' % a, abs(got['pck'][a][1] - ref['pck'][a][1]), 1e-12)
  o = MO.EvalAccumulators(mean, var, mask)
  for k in range(2):
    o.update(ycap * (1 + k), gt * (1 + k))
  h = acc.w1_hist.cpu().numpy()
  ck.true('W1 histograms exact', all(np.array_equal(h[i, j], o.hist[k]) for i, j, k in ((0, 0, 'y_vel'), (0, 1, 'y_acc'), (1, 0, 'gt_vel'), (1, 1, 'gt_acc'))))
  ck.true('rows', acc.rows == 2 * B * T == o.n)
  # fp64 sums of N = 2 * B * T terms in two different orders (the device adds the rows one after the other, numpy in blocks): each side
  # is within (N - 1) * 2^-53 * sum|terms| of the exact sum, whatever its order (Higham, Accuracy and Stability of Numerical
  # Algorithms, 4.2), so the two differ by at most twice that.  A dropped row or a wrong column is ~1 / N of sum|terms|, 10^9 times more
  kept = [j for j in range(52) if j not in mask]
  rows = {'y': np.concatenate([ycap.astype(np.float64) * (1 + k) for k in range(2)]).reshape(-1, 96),
          'gt': np.concatenate([gt.astype(np.float64) * (1 + k) for k in range(2)]).reshape(-1, 2, 52)[..., kept].reshape(-1, 96)}
  sums, gram = acc.fid_sums.cpu().numpy(), acc.fid_gram.cpu().numpy()
  tol = 2 * (2 * B * T - 1) * 2.0 ** -53
  for i, k in enumerate(('y', 'gt')):
    a = np.abs(rows[k])
    ck.atmost('FID sums %s / tolerance' % k, np.max(np.abs(sums[i] - o.sum[k].reshape(-1)) / (tol * a.sum(0))), 1.0)
    ck.atmost('FID Gram %s / tolerance' % k, np.max(np.abs(gram[i] - o.sq[k]) / (tol * (a.T @ a))), 1.0)


def run_metrics_refused(e, ck, labels):
  L = _lib()
  B, T = 2, 4
  with _timed(labels):
    P = 130                                                                                   # 65 joints
    out = torch.full((B, 2 + 65), -3.0, dtype=torch.float64, device=DEV)
    y, gt = torch.randn(B, T, P, device=DEV), torch.randn(B, T, P, device=DEV)
    keep = torch.arange(P, dtype=torch.int32, device=DEV)
    md = torch.ones(P, dtype=torch.float64, device=DEV)
    al = torch.tensor([0.1], device=DEV)
    ck.true('step_metrics: 65 joints refused', L.ms_step_metrics(_p(y), _p(gt), _p(keep), _p(keep), _p(md), _p(md), _p(al), 1, _p(out), B, T, P, P, _stream()) != 0)
    ck.true('step_metrics output untouched', bool((out == -3.0).all()))
    P = 8
    y, gt = torch.randn(B, T, P, device=DEV), torch.randn(B, T, P, device=DEV)
    keep = torch.arange(16, dtype=torch.int32, device=DEV) % P
    md = torch.ones(P, dtype=torch.float64, device=DEV)
    fs = torch.zeros(2, 16, dtype=torch.float64, device=DEV)
    fg = torch.zeros(2, 16, 16, dtype=torch.float64, device=DEV)
    hist = torch.zeros(2, 2, 10, dtype=torch.int64, device=DEV)
    for nm, PK in (('PK > P', 10), ('odd PK', 5), ('PK < 2', 0)):
      rc = L.ms_eval_accumulate(_p(y), _p(gt), _p(keep), _p(md), _p(md), _p(fs), _p(fg), _p(hist), B, T, P, PK, 0.1, 10, _stream())
      ck.true('eval_accumulate: %s refused' % nm, rc != 0)
  ck.true('accumulators untouched', not bool(fs.any()) and not bool(fg.any()) and not bool(hist.any()))


# ------------------------------------------------------------------------------------------------ batched copies
def run_copy_multi(e, ck, labels):
  from mix_stage_amd import ops
  gen = _gen(e)

  def make(i, n):
    if i % 3 == 2:
      src = torch.randint(-9, 9, (n,), generator=gen, dtype=torch.int64).to(DEV)
    elif i % 3 == 1:
      src = torch.randn(n + 1, generator=gen).to(DEV)[1:]                 # 4-byte aligned only
    else:
      src = torch.randn(n, generator=gen).to(DEV)
    whole = torch.full((n + 6,), 77, dtype=src.dtype, device=DEV)          # guard elements on both sides of the destination
    return whole, whole[3:3 + n], src

  if e['p']['kind'] == 'old':
    sizes = [1, 3, 17, 255, 256, 4097, 65536 + 5, 104 * 64 * 32, 2, 7, 1 << 20]
  else:
    sizes = [5, 4096, 3, 64 * 256 + 1, 0, 17, 1 << 16, 9, 300]            # 9 entries, a zero-byte one in the middle
  trip = [make(i, n) for i, n in enumerate(sizes)]
  with _timed(labels):
    if e['via'] == 'lib':
      n = len(trip)
      srcs = (ctypes.c_void_p * n)(*[(s.data_ptr() if s.numel() else None) for _, _, s in trip])
      dsts = (ctypes.c_void_p * n)(*[(d.data_ptr() if d.numel() else None) for _, d, _ in trip])
      nbytes = (ctypes.c_size_t * n)(*[d.numel() * d.element_size() for _, d, _ in trip])
      assert _lib().ms_copy_multi(n, srcs, dsts, nbytes, _stream()) == 0
    else:
      ops.copy_multi([(d, s) for _, d, s in trip])
  for i, (whole, d, s) in enumerate(trip):
    ck.exact('copy %d (%d elements)' % (i, s.numel()), d, s)
    ck.true('guards of copy %d' % i, bool((whole[:3] == 77).all()) and bool((whole[3 + s.numel():] == 77).all()))
  ck.true('launches', sum(l.startswith('ew|ew_copy_multi') for l in labels) == 1)


RUNNERS = {'softmax_mix': run_softmax_mix, 'cross_entropy': run_cross_entropy, 'lp_mean': run_lp_mean, 'lp_pair': run_lp_pair,
           'lp_pair_refused': run_lp_pair_refused, 'sqnorm': run_sqnorm, 'adam': run_adam, 'lerp': run_lerp, 'concat': run_concat,
           'velocity': run_velocity, 'bn_trio': run_bn_trio, 'cb8': run_cb8, 'prestep': run_prestep, 'prestep_refused': run_prestep_refused,
           'metrics': run_metrics, 'metrics_refused': run_metrics_refused, 'copy_multi': run_copy_multi}


@pytest.mark.parametrize('e', TABLE, ids=[e['id'] for e in TABLE])
def test_ew_entry_point_matches_fp64(e):
  labels = []
  ck = Checks(e)
  RUNNERS[e['op']](e, ck, labels)
  missing = [l for l in e['labels'] if not any(g.startswith(l) for g in labels)]
  present = [(l, g) for l in e['forbid'] for g in labels if g.startswith(l)]
  assert not missing and not present, ('%s did not reach its kernels: missing %s, forbidden %s; launches: %s'
                                       % (e['id'], missing, present, sorted(set(labels))))
  ck.finish()
