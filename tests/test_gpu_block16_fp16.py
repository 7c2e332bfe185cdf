"""GPU: fp16 TRAINING blocks (BN_TRAIN forward in both BatchNorm forms, bn_bwd16, the data gradient with parity classes,
upsample-add / broadcast / grouped inputs, fp32 score outputs, wgrad16 and wgrad16_c1, the y / y_raw choice) against fp64 on the
same fp16-rounded operands, with bars sized for fp16 -- test_gpu_kernels16._case(bars='dtype'): the smaller of the bf16 bar
x 2^-3 and 3 x the error the reference itself shows when it is rounded once at every place where the kernels store a 16-bit
tensor (tests/helpers/round16_model.py; the cases and their seeds: tests/helpers/fp16_block_table.py, held to their conditions
by tests/test_round16_model_cpu.py).  A bf16-grade result -- a bf16 pack left in an epilogue, an intermediate in the wrong type,
flushed subnormals -- sits at about 8 x the model and fails; under the bars of test_gpu_kernels16 it passed.

Every case runs under the launch timing and must name f16, never bf16, in every launch label that names an operand type.

test_tiny_gradients_*: dy elements of 1e-7, far inside fp16's subnormal range, carried at loss scales 2^16 and 2^10 to the bars
of unit-size gradients; the same blocks at S = 1 are measured and printed beside the model's prediction, not asserted.
test_overflow_*: one element of S * dy above 65504, or one input element that rounds to inf: what the fp64 reference makes
non-finite is non-finite on the device, everything outside the geometric reach of that element is finite and within the bars,
and ms_sqnorm of the device dw -- what the trainer's skip rule reads -- is non-finite.

`pytest -s` prints one row per case and check: model, measured, bar.

Shown to fail: this file was run once against the library built with two numerics-only changes in elementwise16.hip, and once with
the device tensors in bf16 under fp16's reference and bars (test_gpu_kernels16.py passed in full against the changed library):
  bn_bwd16_fused_kernel rounds dy_raw through bf16 before its fp16 pack      all 19 BN_TRAIN table cases and the 6 scaled BN_TRAIN runs:
                                                                             dw l2 1.6e-3 .. 2.0e-3 against bars of 0.7e-3 .. 1.0e-3 (the
                                                                             bf16-sized bar, 2e-2, passes it)
  act_bwd16_kernel clamps to +-65504 before its pack (a saturating store)    the three backward overflow cases: ms_sqnorm of dw finite
                                                                             (1.2e6, 9.4e5) for the LeakyReLU and fp32-output blocks, a finite
                                                                             bias gradient for the cb8 block
  device in bf16, reference and bars fp16, k3_bn_in_launch (exact mask)      fwd 3.06e-3 against 7.3e-4 (the bf16-sized bar: 1.2e-2, passes);
                                                                             dw l2 3.3e-2, dx l2 3.3e-2, dgamma l2 5.1e-3 against 0.9e-3 .. 1.1e-3;
                                                                             with the device mask: 2 mask flips beyond one fp16 rounding

Measured on one MI355X (`python -m pytest tests/test_gpu_block16_fp16.py -m gpu -s`; the kernels reduce in a fixed order, a rerun
prints the same figures).  model: the reference's own emulated error (for the gradients: against the reference with an unrounded
dy, so the device, which shares the dy rounding with _case's reference, sits a little below it); '-': no model figure.
The `dy1e-7 S...` rows show the model at that dy and S; their bar is the unit-size block's (3 x the model of the plain row).

  MEASURED_TABLE_BEGIN
  case                               check                              model  measured       bar
  k3_bn_in_launch                    mask flips (fraction)                  -  0.00e+00  2.00e-03
  k3_bn_in_launch                    mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k3_bn_in_launch                    fwd                             2.45e-04  2.45e-04  7.34e-04
  k3_bn_in_launch                    dw                              3.27e-04  2.01e-04  9.81e-04
  k3_bn_in_launch                    dw l2                           3.10e-04  2.21e-04  9.29e-04
  k3_bn_in_launch                    dgamma                          2.39e-04  1.92e-04  7.16e-04
  k3_bn_in_launch                    dgamma l2                       3.06e-04  2.11e-04  9.18e-04
  k3_bn_in_launch                    dbeta                           2.66e-04  8.89e-08  7.99e-04
  k3_bn_in_launch                    dbeta l2                        2.51e-04  6.83e-08  7.53e-04
  k3_bn_in_launch                    dx                              4.54e-04  3.98e-04  1.36e-03
  k3_bn_in_launch                    dx l2                           3.77e-04  2.97e-04  1.13e-03
  k3_bn_two_launch                   mask flips (fraction)                  -  0.00e+00  2.00e-03
  k3_bn_two_launch                   mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k3_bn_two_launch                   fwd                             4.85e-04  4.85e-04  1.45e-03
  k3_bn_two_launch                   dw                              3.31e-04  2.11e-04  9.93e-04
  k3_bn_two_launch                   dw l2                           3.12e-04  2.23e-04  9.36e-04
  k3_bn_two_launch                   dgamma                          3.60e-04  2.25e-04  1.08e-03
  k3_bn_two_launch                   dgamma l2                       3.98e-04  3.29e-04  1.19e-03
  k3_bn_two_launch                   dbeta                           2.66e-04  8.89e-08  7.99e-04
  k3_bn_two_launch                   dbeta l2                        2.51e-04  6.83e-08  7.53e-04
  k3_bn_two_launch                   dx                              4.54e-04  4.13e-04  1.36e-03
  k3_bn_two_launch                   dx l2                           3.76e-04  3.03e-04  1.13e-03
  k3_c256                            mask flips (fraction)                  -  0.00e+00  2.00e-03
  k3_c256                            mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k3_c256                            fwd                             3.91e-04  3.91e-04  1.17e-03
  k3_c256                            dw                              3.18e-04  2.17e-04  9.53e-04
  k3_c256                            dw l2                           2.97e-04  2.09e-04  8.91e-04
  k3_c256                            dgamma                          3.19e-04  2.67e-04  9.57e-04
  k3_c256                            dgamma l2                       3.01e-04  2.13e-04  9.02e-04
  k3_c256                            dbeta                           2.18e-04  6.88e-08  6.53e-04
  k3_c256                            dbeta l2                        2.12e-04  6.91e-08  6.35e-04
  k3_c256                            dx                              4.27e-04  4.12e-04  1.28e-03
  k3_c256                            dx l2                           3.64e-04  2.95e-04  1.09e-03
  k4s2_w16                           mask flips (fraction)                  -  0.00e+00  2.00e-03
  k4s2_w16                           mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k4s2_w16                           fwd                             2.74e-04  2.74e-04  8.22e-04
  k4s2_w16                           dw                              3.11e-04  2.63e-04  9.33e-04
  k4s2_w16                           dw l2                           3.01e-04  2.19e-04  9.03e-04
  k4s2_w16                           dgamma                          3.06e-04  2.08e-04  9.17e-04
  k4s2_w16                           dgamma l2                       2.83e-04  2.09e-04  8.48e-04
  k4s2_w16                           dbeta                           1.64e-04  6.26e-08  4.91e-04
  k4s2_w16                           dbeta l2                        1.57e-04  4.77e-08  4.70e-04
  k4s2_w16                           dx                              4.54e-04  3.66e-04  1.36e-03
  k4s2_w16                           dx l2                           3.67e-04  3.00e-04  1.10e-03
  k4s2_w4                            mask flips (fraction)                  -  0.00e+00  2.00e-03
  k4s2_w4                            mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k4s2_w4                            fwd                             3.25e-04  3.25e-04  9.75e-04
  k4s2_w4                            dw                              4.65e-04  3.32e-04  1.40e-03
  k4s2_w4                            dw l2                           3.20e-04  2.55e-04  9.61e-04
  k4s2_w4                            dgamma                          4.32e-04  2.20e-04  1.30e-03
  k4s2_w4                            dgamma l2                       3.23e-04  2.06e-04  9.70e-04
  k4s2_w4                            dbeta                           2.01e-04  8.15e-08  6.02e-04
  k4s2_w4                            dbeta l2                        1.83e-04  3.83e-08  5.48e-04
  k4s2_w4                            dx                              4.24e-04  3.63e-04  1.27e-03
  k4s2_w4                            dx l2                           3.70e-04  3.23e-04  1.11e-03
  k4s2_16to24_w37                    mask flips (fraction)                  -  0.00e+00  2.00e-03
  k4s2_16to24_w37                    mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k4s2_16to24_w37                    fwd                             3.00e-04  3.00e-04  8.99e-04
  k4s2_16to24_w37                    dw                              3.05e-04  2.11e-04  9.16e-04
  k4s2_16to24_w37                    dw l2                           2.89e-04  2.03e-04  8.67e-04
  k4s2_16to24_w37                    dgamma                          1.79e-04  1.44e-04  5.38e-04
  k4s2_16to24_w37                    dgamma l2                       2.42e-04  1.51e-04  7.26e-04
  k4s2_16to24_w37                    dbeta                           2.00e-04  6.69e-08  6.00e-04
  k4s2_16to24_w37                    dbeta l2                        1.95e-04  6.26e-08  5.84e-04
  k4s2_16to24_w37                    dx                              4.32e-04  3.74e-04  1.30e-03
  k4s2_16to24_w37                    dx l2                           3.58e-04  2.99e-04  1.08e-03
  up2_w16                            mask flips (fraction)                  -  0.00e+00  2.00e-03
  up2_w16                            mask flips beyond one rounding         -  0.00e+00  0.00e+00
  up2_w16                            fwd                             2.30e-04  2.30e-04  6.90e-04
  up2_w16                            dw                              3.53e-04  2.57e-04  1.06e-03
  up2_w16                            dw l2                           3.01e-04  2.15e-04  9.02e-04
  up2_w16                            dgamma                          3.32e-04  2.47e-04  9.95e-04
  up2_w16                            dgamma l2                       3.17e-04  2.34e-04  9.50e-04
  up2_w16                            dbeta                           1.97e-04  1.10e-07  5.92e-04
  up2_w16                            dbeta l2                        1.77e-04  6.35e-08  5.32e-04
  up2_w16                            dx2                             4.59e-04  3.43e-04  1.38e-03
  up2_w16                            dx2 l2                          3.57e-04  2.96e-04  1.07e-03
  up2_w16                            dx                              4.77e-04  3.48e-04  1.43e-03
  up2_w16                            dx l2                           3.56e-04  2.95e-04  1.07e-03
  up2_w2                             mask flips (fraction)                  -  0.00e+00  2.00e-03
  up2_w2                             mask flips beyond one rounding         -  0.00e+00  0.00e+00
  up2_w2                             fwd                             3.59e-04  3.59e-04  1.08e-03
  up2_w2                             dw                              3.55e-04  3.09e-04  1.07e-03
  up2_w2                             dw l2                           2.98e-04  2.35e-04  8.93e-04
  up2_w2                             dgamma                          4.49e-04  3.05e-04  1.35e-03
  up2_w2                             dgamma l2                       3.68e-04  2.52e-04  1.10e-03
  up2_w2                             dbeta                           1.94e-04  3.72e-08  5.82e-04
  up2_w2                             dbeta l2                        1.89e-04  3.63e-08  5.68e-04
  up2_w2                             dx2                             4.61e-04  3.83e-04  1.38e-03
  up2_w2                             dx2 l2                          3.76e-04  3.14e-04  1.13e-03
  up2_w2                             dx                              4.72e-04  4.45e-04  1.42e-03
  up2_w2                             dx l2                           3.66e-04  3.09e-04  1.10e-03
  bcast_g3                           mask flips (fraction)                  -  0.00e+00  2.00e-03
  bcast_g3                           mask flips beyond one rounding         -  0.00e+00  0.00e+00
  bcast_g3                           fwd                             2.27e-04  2.27e-04  6.80e-04
  bcast_g3                           dw                              4.91e-04  2.47e-04  1.47e-03
  bcast_g3                           dw l2                           3.05e-04  2.27e-04  9.14e-04
  bcast_g3                           dgamma                          3.40e-04  1.77e-04  1.02e-03
  bcast_g3                           dgamma l2                       3.02e-04  1.81e-04  9.05e-04
  bcast_g3                           dbeta                           2.62e-04  9.80e-08  7.87e-04
  bcast_g3                           dbeta l2                        2.34e-04  6.76e-08  7.01e-04
  bcast_g3                           dx                              3.68e-04  4.12e-04  1.10e-03
  bcast_g3                           dx l2                           3.64e-04  3.08e-04  1.09e-03
  grouped_g3                         mask flips (fraction)                  -  0.00e+00  2.00e-03
  grouped_g3                         mask flips beyond one rounding         -  0.00e+00  0.00e+00
  grouped_g3                         fwd                             3.81e-04  3.81e-04  1.14e-03
  grouped_g3                         dw                              3.14e-04  2.04e-04  9.43e-04
  grouped_g3                         dw l2                           3.00e-04  2.08e-04  9.01e-04
  grouped_g3                         dgamma                          2.49e-04  1.84e-04  7.48e-04
  grouped_g3                         dgamma l2                       2.79e-04  2.00e-04  8.36e-04
  grouped_g3                         dbeta                           2.44e-04  5.81e-08  7.32e-04
  grouped_g3                         dbeta l2                        2.53e-04  5.16e-08  7.58e-04
  grouped_g3                         dx                              4.09e-04  3.75e-04  1.23e-03
  grouped_g3                         dx l2                           3.64e-04  2.98e-04  1.09e-03
  grouped_bare_k1                    fwd                             0.00e+00  8.05e-08  2.00e-05
  grouped_bare_k1                    dw                              2.55e-04  2.55e-04  7.64e-04
  grouped_bare_k1                    dw l2                           2.05e-04  2.05e-04  6.16e-04
  grouped_bare_k1                    dbias                           0.00e+00  1.13e-07  1.00e-04
  grouped_bare_k1                    dbias l2                        0.00e+00  6.25e-08  1.00e-04
  grouped_bare_k1                    dx                              2.80e-04  2.80e-04  8.39e-04
  grouped_bare_k1                    dx l2                           2.81e-04  2.81e-04  8.42e-04
  cin74                              mask flips (fraction)                  -  0.00e+00  2.00e-03
  cin74                              mask flips beyond one rounding         -  0.00e+00  0.00e+00
  cin74                              fwd                             2.46e-04  2.46e-04  7.38e-04
  cin74                              dw                              3.44e-04  2.25e-04  1.03e-03
  cin74                              dw l2                           2.93e-04  2.15e-04  8.79e-04
  cin74                              dgamma                          3.72e-04  1.73e-04  1.12e-03
  cin74                              dgamma l2                       2.50e-04  1.69e-04  7.51e-04
  cin74                              dbeta                           2.15e-04  6.12e-08  6.44e-04
  cin74                              dbeta l2                        2.02e-04  6.23e-08  6.05e-04
  cin74                              dx                              3.71e-04  3.40e-04  1.11e-03
  cin74                              dx l2                           3.60e-04  3.01e-04  1.08e-03
  cin104                             mask flips (fraction)                  -  0.00e+00  2.00e-03
  cin104                             mask flips beyond one rounding         -  0.00e+00  0.00e+00
  cin104                             fwd                             2.12e-04  2.12e-04  6.37e-04
  cin104                             dw                              3.01e-04  1.90e-04  9.03e-04
  cin104                             dw l2                           3.00e-04  2.11e-04  9.01e-04
  cin104                             dgamma                          4.55e-04  2.02e-04  1.36e-03
  cin104                             dgamma l2                       2.86e-04  1.87e-04  8.58e-04
  cin104                             dbeta                           2.78e-04  6.98e-08  8.34e-04
  cin104                             dbeta l2                        2.34e-04  5.33e-08  7.03e-04
  cin104                             dx                              4.67e-04  3.42e-04  1.40e-03
  cin104                             dx l2                           3.57e-04  2.90e-04  1.07e-03
  cout5_f32                          mask flips (fraction)                  -  0.00e+00  2.00e-03
  cout5_f32                          mask flips beyond one rounding         -  0.00e+00  0.00e+00
  cout5_f32                          fwd                             4.48e-04  4.48e-04  1.34e-03
  cout5_f32                          dw                              2.65e-04  2.65e-04  7.96e-04
  cout5_f32                          dw l2                           2.26e-04  2.26e-04  6.79e-04
  cout5_f32                          dgamma                          1.61e-04  1.61e-04  4.83e-04
  cout5_f32                          dgamma l2                       1.23e-04  1.23e-04  3.68e-04
  cout5_f32                          dbeta                           0.00e+00  6.11e-08  1.01e-04
  cout5_f32                          dbeta l2                        0.00e+00  4.65e-08  1.00e-04
  cout5_f32                          dx                              5.72e-04  5.72e-04  1.71e-03
  cout5_f32                          dx l2                           2.97e-04  2.97e-04  8.91e-04
  bare_cout1                         fwd                             0.00e+00  2.06e-07  2.00e-05
  bare_cout1                         dw                              1.83e-04  1.83e-04  5.50e-04
  bare_cout1                         dw l2                           1.94e-04  1.94e-04  5.82e-04
  bare_cout1                         dbias                           0.00e+00  1.28e-07  1.00e-04
  bare_cout1                         dbias l2                        0.00e+00  1.28e-07  1.00e-04
  bare_cout1                         dx                              3.38e-04  3.38e-04  1.01e-03
  bare_cout1                         dx l2                           2.88e-04  2.88e-04  8.63e-04
  lrelu_k4s2_cin104                  mask flips (fraction)                  -  0.00e+00  2.00e-03
  lrelu_k4s2_cin104                  mask flips beyond one rounding         -  0.00e+00  0.00e+00
  lrelu_k4s2_cin104                  fwd                             2.89e-04  2.89e-04  8.67e-04
  lrelu_k4s2_cin104                  dw                              2.42e-04  4.86e-05  7.26e-04
  lrelu_k4s2_cin104                  dw l2                           2.08e-04  4.04e-05  6.23e-04
  lrelu_k4s2_cin104                  dbias                           2.61e-04  6.71e-08  7.83e-04
  lrelu_k4s2_cin104                  dbias l2                        1.93e-04  5.25e-08  5.78e-04
  lrelu_k4s2_cin104                  dx                              4.24e-04  3.21e-04  1.27e-03
  lrelu_k4s2_cin104                  dx l2                           2.95e-04  2.10e-04  8.84e-04
  2d_c1_3x3                          mask flips (fraction)                  -  0.00e+00  2.00e-03
  2d_c1_3x3                          mask flips beyond one rounding         -  0.00e+00  0.00e+00
  2d_c1_3x3                          fwd                             4.05e-04  4.05e-04  1.22e-03
  2d_c1_3x3                          dw                              3.81e-04  2.88e-04  1.14e-03
  2d_c1_3x3                          dw l2                           3.07e-04  2.42e-04  9.20e-04
  2d_c1_3x3                          dgamma                          4.31e-04  3.29e-04  1.29e-03
  2d_c1_3x3                          dgamma l2                       2.98e-04  2.09e-04  8.94e-04
  2d_c1_3x3                          dbeta                           2.27e-04  8.14e-08  6.81e-04
  2d_c1_3x3                          dbeta l2                        1.97e-04  7.88e-08  5.92e-04
  2d_c1_3x3                          dx                              2.45e-04  2.24e-04  7.35e-04
  2d_c1_3x3                          dx l2                           3.46e-04  2.92e-04  1.04e-03
  2d_k4s2                            mask flips (fraction)                  -  0.00e+00  2.00e-03
  2d_k4s2                            mask flips beyond one rounding         -  0.00e+00  0.00e+00
  2d_k4s2                            fwd                             2.48e-04  2.48e-04  7.43e-04
  2d_k4s2                            dw                              3.27e-04  3.27e-04  9.82e-04
  2d_k4s2                            dw l2                           2.96e-04  2.21e-04  8.87e-04
  2d_k4s2                            dgamma                          3.85e-04  2.48e-04  1.16e-03
  2d_k4s2                            dgamma l2                       2.90e-04  2.32e-04  8.69e-04
  2d_k4s2                            dbeta                           3.65e-04  1.00e-07  1.10e-03
  2d_k4s2                            dbeta l2                        2.55e-04  6.55e-08  7.65e-04
  2d_k4s2                            dx                              4.14e-04  2.88e-04  1.24e-03
  2d_k4s2                            dx l2                           3.70e-04  3.03e-04  1.11e-03
  2d_k3x8                            mask flips (fraction)                  -  0.00e+00  2.00e-03
  2d_k3x8                            mask flips beyond one rounding         -  0.00e+00  0.00e+00
  2d_k3x8                            fwd                             2.85e-04  2.85e-04  8.56e-04
  2d_k3x8                            dw                              2.31e-04  1.57e-04  6.94e-04
  2d_k3x8                            dw l2                           2.87e-04  2.02e-04  8.61e-04
  2d_k3x8                            dgamma                          2.57e-04  2.80e-04  7.72e-04
  2d_k3x8                            dgamma l2                       3.25e-04  3.25e-04  9.74e-04
  2d_k3x8                            dbeta                           2.91e-04  4.97e-08  8.73e-04
  2d_k3x8                            dbeta l2                        2.14e-04  6.06e-08  6.41e-04
  2d_k3x8                            dx                              4.54e-04  4.08e-04  1.36e-03
  2d_k3x8                            dx l2                           3.54e-04  2.91e-04  1.06e-03
  2d_k3_c128                         mask flips (fraction)                  -  0.00e+00  2.00e-03
  2d_k3_c128                         mask flips beyond one rounding         -  0.00e+00  0.00e+00
  2d_k3_c128                         fwd                             3.60e-04  3.60e-04  1.08e-03
  2d_k3_c128                         dw                              2.99e-04  1.98e-04  8.96e-04
  2d_k3_c128                         dw l2                           2.95e-04  2.10e-04  8.84e-04
  2d_k3_c128                         dgamma                          3.07e-04  2.44e-04  9.20e-04
  2d_k3_c128                         dgamma l2                       3.33e-04  2.35e-04  1.00e-03
  2d_k3_c128                         dbeta                           2.84e-04  8.43e-08  8.53e-04
  2d_k3_c128                         dbeta l2                        2.37e-04  7.75e-08  7.11e-04
  2d_k3_c128                         dx                              5.64e-04  3.66e-04  1.69e-03
  2d_k3_c128                         dx l2                           3.59e-04  2.93e-04  1.08e-03
  fragile                            fwd                             3.58e-04  3.58e-04  1.07e-03
  fragile                            dw                              2.57e-04  1.87e-04  7.72e-04
  fragile                            dw l2                           2.91e-04  2.09e-04  8.74e-04
  fragile                            dgamma                          2.86e-04  2.12e-04  8.59e-04
  fragile                            dgamma l2                       2.95e-04  2.20e-04  8.86e-04
  fragile                            dbeta                           2.00e-04  6.84e-08  6.01e-04
  fragile                            dbeta l2                        2.13e-04  5.68e-08  6.40e-04
  fragile                            dx                              5.08e-04  3.98e-04  1.52e-03
  fragile                            dx l2                           3.57e-04  2.96e-04  1.07e-03
  relu_slope0                        fwd                             2.45e-04  2.45e-04  7.34e-04
  relu_slope0                        dw                              2.88e-04  1.91e-04  8.63e-04
  relu_slope0                        dw l2                           3.12e-04  2.16e-04  9.35e-04
  relu_slope0                        dgamma                          2.73e-04  1.47e-04  8.18e-04
  relu_slope0                        dgamma l2                       2.90e-04  2.25e-04  8.69e-04
  relu_slope0                        dbeta                           2.78e-04  3.66e-08  8.35e-04
  relu_slope0                        dbeta l2                        2.44e-04  1.13e-08  7.32e-04
  relu_slope0                        dx                              4.47e-04  2.94e-04  1.34e-03
  relu_slope0                        dx l2                           3.71e-04  2.96e-04  1.11e-03
  k3_bn_in_launch dy1e-7 S65536      mask flips (fraction)                  -  0.00e+00  2.00e-03
  k3_bn_in_launch dy1e-7 S65536      mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k3_bn_in_launch dy1e-7 S65536      fwd                             2.45e-04  2.45e-04  7.34e-04
  k3_bn_in_launch dy1e-7 S65536      dw                              2.57e-04  1.63e-04  9.81e-04
  k3_bn_in_launch dy1e-7 S65536      dw l2                           2.85e-04  2.07e-04  9.29e-04
  k3_bn_in_launch dy1e-7 S65536      dgamma                          2.38e-04  1.92e-04  7.16e-04
  k3_bn_in_launch dy1e-7 S65536      dgamma l2                       2.76e-04  2.11e-04  9.18e-04
  k3_bn_in_launch dy1e-7 S65536      dbeta                           2.56e-04  6.18e-08  7.99e-04
  k3_bn_in_launch dy1e-7 S65536      dbeta l2                        2.15e-04  5.99e-08  7.53e-04
  k3_bn_in_launch dy1e-7 S65536      dx                              4.83e-04  3.35e-04  1.36e-03
  k3_bn_in_launch dy1e-7 S65536      dx l2                           3.43e-04  2.85e-04  1.13e-03
  k3_bn_in_launch dy1e-7 S1024       mask flips (fraction)                  -  0.00e+00  2.00e-03
  k3_bn_in_launch dy1e-7 S1024       mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k3_bn_in_launch dy1e-7 S1024       fwd                             2.45e-04  2.45e-04  7.34e-04
  k3_bn_in_launch dy1e-7 S1024       dw                              2.67e-04  1.88e-04  9.81e-04
  k3_bn_in_launch dy1e-7 S1024       dw l2                           3.50e-04  2.69e-04  9.29e-04
  k3_bn_in_launch dy1e-7 S1024       dgamma                          2.53e-04  1.92e-04  7.16e-04
  k3_bn_in_launch dy1e-7 S1024       dgamma l2                       3.22e-04  2.11e-04  9.18e-04
  k3_bn_in_launch dy1e-7 S1024       dbeta                           3.16e-04  8.83e-08  7.99e-04
  k3_bn_in_launch dy1e-7 S1024       dbeta l2                        2.62e-04  6.64e-08  7.53e-04
  k3_bn_in_launch dy1e-7 S1024       dx                              4.83e-04  3.99e-04  1.36e-03
  k3_bn_in_launch dy1e-7 S1024       dx l2                           4.32e-04  3.77e-04  1.13e-03
  k4s2_w16 dy1e-7 S65536             mask flips (fraction)                  -  0.00e+00  2.00e-03
  k4s2_w16 dy1e-7 S65536             mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k4s2_w16 dy1e-7 S65536             fwd                             2.74e-04  2.74e-04  8.22e-04
  k4s2_w16 dy1e-7 S65536             dw                              4.00e-04  2.29e-04  9.33e-04
  k4s2_w16 dy1e-7 S65536             dw l2                           3.11e-04  2.16e-04  9.03e-04
  k4s2_w16 dy1e-7 S65536             dgamma                          3.91e-04  2.08e-04  9.17e-04
  k4s2_w16 dy1e-7 S65536             dgamma l2                       3.36e-04  2.09e-04  8.48e-04
  k4s2_w16 dy1e-7 S65536             dbeta                           1.83e-04  5.59e-08  4.91e-04
  k4s2_w16 dy1e-7 S65536             dbeta l2                        1.88e-04  5.63e-08  4.70e-04
  k4s2_w16 dy1e-7 S65536             dx                              5.06e-04  3.73e-04  1.36e-03
  k4s2_w16 dy1e-7 S65536             dx l2                           3.66e-04  2.93e-04  1.10e-03
  k4s2_w16 dy1e-7 S1024              mask flips (fraction)                  -  0.00e+00  2.00e-03
  k4s2_w16 dy1e-7 S1024              mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k4s2_w16 dy1e-7 S1024              fwd                             2.74e-04  2.74e-04  8.22e-04
  k4s2_w16 dy1e-7 S1024              dw                              4.00e-04  2.65e-04  9.33e-04
  k4s2_w16 dy1e-7 S1024              dw l2                           3.64e-04  2.72e-04  9.03e-04
  k4s2_w16 dy1e-7 S1024              dgamma                          4.42e-04  2.08e-04  9.17e-04
  k4s2_w16 dy1e-7 S1024              dgamma l2                       3.51e-04  2.09e-04  8.48e-04
  k4s2_w16 dy1e-7 S1024              dbeta                           2.42e-04  7.46e-08  4.91e-04
  k4s2_w16 dy1e-7 S1024              dbeta l2                        2.24e-04  4.66e-08  4.70e-04
  k4s2_w16 dy1e-7 S1024              dx                              5.06e-04  3.99e-04  1.36e-03
  k4s2_w16 dy1e-7 S1024              dx l2                           4.81e-04  4.16e-04  1.10e-03
  up2_w16 dy1e-7 S65536              mask flips (fraction)                  -  0.00e+00  2.00e-03
  up2_w16 dy1e-7 S65536              mask flips beyond one rounding         -  0.00e+00  0.00e+00
  up2_w16 dy1e-7 S65536              fwd                             2.30e-04  2.30e-04  6.90e-04
  up2_w16 dy1e-7 S65536              dw                              3.76e-04  2.68e-04  1.06e-03
  up2_w16 dy1e-7 S65536              dw l2                           3.05e-04  2.17e-04  9.02e-04
  up2_w16 dy1e-7 S65536              dgamma                          4.38e-04  2.47e-04  9.95e-04
  up2_w16 dy1e-7 S65536              dgamma l2                       3.37e-04  2.34e-04  9.50e-04
  up2_w16 dy1e-7 S65536              dbeta                           2.09e-04  9.80e-08  5.92e-04
  up2_w16 dy1e-7 S65536              dbeta l2                        1.98e-04  7.16e-08  5.32e-04
  up2_w16 dy1e-7 S65536              dx2                             4.24e-04  3.61e-04  1.38e-03
  up2_w16 dy1e-7 S65536              dx2 l2                          3.63e-04  2.96e-04  1.07e-03
  up2_w16 dy1e-7 S65536              dx                              3.40e-04  3.13e-04  1.43e-03
  up2_w16 dy1e-7 S65536              dx l2                           3.63e-04  2.94e-04  1.07e-03
  up2_w16 dy1e-7 S1024               mask flips (fraction)                  -  0.00e+00  2.00e-03
  up2_w16 dy1e-7 S1024               mask flips beyond one rounding         -  0.00e+00  0.00e+00
  up2_w16 dy1e-7 S1024               fwd                             2.30e-04  2.30e-04  6.90e-04
  up2_w16 dy1e-7 S1024               dw                              4.00e-04  2.98e-04  1.06e-03
  up2_w16 dy1e-7 S1024               dw l2                           4.19e-04  3.41e-04  9.02e-04
  up2_w16 dy1e-7 S1024               dgamma                          4.57e-04  2.47e-04  9.95e-04
  up2_w16 dy1e-7 S1024               dgamma l2                       3.82e-04  2.34e-04  9.50e-04
  up2_w16 dy1e-7 S1024               dbeta                           2.56e-04  6.53e-08  5.92e-04
  up2_w16 dy1e-7 S1024               dbeta l2                        2.46e-04  5.89e-08  5.32e-04
  up2_w16 dy1e-7 S1024               dx2                             7.19e-04  5.43e-04  1.38e-03
  up2_w16 dy1e-7 S1024               dx2 l2                          5.14e-04  4.52e-04  1.07e-03
  up2_w16 dy1e-7 S1024               dx                              4.03e-04  3.98e-04  1.43e-03
  up2_w16 dy1e-7 S1024               dx l2                           4.91e-04  4.28e-04  1.07e-03
  lrelu_k4s2_cin104 dy1e-7 S65536    mask flips (fraction)                  -  0.00e+00  2.00e-03
  lrelu_k4s2_cin104 dy1e-7 S65536    mask flips beyond one rounding         -  0.00e+00  0.00e+00
  lrelu_k4s2_cin104 dy1e-7 S65536    fwd                             2.89e-04  2.89e-04  8.67e-04
  lrelu_k4s2_cin104 dy1e-7 S65536    dw                              2.71e-04  4.38e-05  7.26e-04
  lrelu_k4s2_cin104 dy1e-7 S65536    dw l2                           2.14e-04  4.05e-05  6.23e-04
  lrelu_k4s2_cin104 dy1e-7 S65536    dbias                           3.02e-04  9.99e-08  7.83e-04
  lrelu_k4s2_cin104 dy1e-7 S65536    dbias l2                        2.26e-04  6.43e-08  5.78e-04
  lrelu_k4s2_cin104 dy1e-7 S65536    dx                              3.41e-04  3.18e-04  1.27e-03
  lrelu_k4s2_cin104 dy1e-7 S65536    dx l2                           2.99e-04  2.10e-04  8.84e-04
  lrelu_k4s2_cin104 dy1e-7 S1024     mask flips (fraction)                  -  0.00e+00  2.00e-03
  lrelu_k4s2_cin104 dy1e-7 S1024     mask flips beyond one rounding         -  0.00e+00  0.00e+00
  lrelu_k4s2_cin104 dy1e-7 S1024     fwd                             2.89e-04  2.89e-04  8.67e-04
  lrelu_k4s2_cin104 dy1e-7 S1024     dw                              2.99e-04  1.35e-04  7.26e-04
  lrelu_k4s2_cin104 dy1e-7 S1024     dw l2                           2.86e-04  1.64e-04  6.23e-04
  lrelu_k4s2_cin104 dy1e-7 S1024     dbias                           2.93e-04  1.07e-07  7.83e-04
  lrelu_k4s2_cin104 dy1e-7 S1024     dbias l2                        2.46e-04  6.13e-08  5.78e-04
  lrelu_k4s2_cin104 dy1e-7 S1024     dx                              4.86e-04  3.18e-04  1.27e-03
  lrelu_k4s2_cin104 dy1e-7 S1024     dx l2                           5.23e-04  4.64e-04  8.84e-04
  k3_bn_in_launch dy1e-7 S1          mask flips (fraction)                  -  0.00e+00  2.00e-03
  k3_bn_in_launch dy1e-7 S1          mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k3_bn_in_launch dy1e-7 S1          fwd                             2.45e-04  2.45e-04  7.34e-04
  k3_bn_in_launch dy1e-7 S1          dw                              1.75e-01  1.36e-01  5.00e-03
  k3_bn_in_launch dy1e-7 S1          dw l2                           2.65e-01  1.99e-01  2.50e-03
  k3_bn_in_launch dy1e-7 S1          dgamma                          1.55e-01  2.20e-04  5.00e-03
  k3_bn_in_launch dy1e-7 S1          dgamma l2                       1.77e-01  2.21e-04  2.50e-03
  k3_bn_in_launch dy1e-7 S1          dbeta                           1.95e-01  8.82e-08  5.00e-03
  k3_bn_in_launch dy1e-7 S1          dbeta l2                        1.96e-01  7.01e-08  2.50e-03
  k3_bn_in_launch dy1e-7 S1          dx                              2.68e-01  2.11e-01  5.00e-03
  k3_bn_in_launch dy1e-7 S1          dx l2                           3.43e-01  2.98e-01  2.50e-03
  k4s2_w16 dy1e-7 S1                 mask flips (fraction)                  -  0.00e+00  2.00e-03
  k4s2_w16 dy1e-7 S1                 mask flips beyond one rounding         -  0.00e+00  0.00e+00
  k4s2_w16 dy1e-7 S1                 fwd                             2.74e-04  2.74e-04  8.22e-04
  k4s2_w16 dy1e-7 S1                 dw                              2.19e-01  1.76e-01  5.00e-03
  k4s2_w16 dy1e-7 S1                 dw l2                           2.71e-01  2.07e-01  2.50e-03
  k4s2_w16 dy1e-7 S1                 dgamma                          1.65e-01  1.86e-04  5.00e-03
  k4s2_w16 dy1e-7 S1                 dgamma l2                       1.80e-01  2.09e-04  2.50e-03
  k4s2_w16 dy1e-7 S1                 dbeta                           1.23e-01  3.40e-08  5.00e-03
  k4s2_w16 dy1e-7 S1                 dbeta l2                        1.56e-01  4.06e-08  2.50e-03
  k4s2_w16 dy1e-7 S1                 dx                              3.20e-01  2.91e-01  5.00e-03
  k4s2_w16 dy1e-7 S1                 dx l2                           4.08e-01  3.62e-01  2.50e-03
  up2_w16 dy1e-7 S1                  mask flips (fraction)                  -  0.00e+00  2.00e-03
  up2_w16 dy1e-7 S1                  mask flips beyond one rounding         -  0.00e+00  0.00e+00
  up2_w16 dy1e-7 S1                  fwd                             2.30e-04  2.30e-04  6.90e-04
  up2_w16 dy1e-7 S1                  dw                              3.19e-01  2.60e-01  5.00e-03
  up2_w16 dy1e-7 S1                  dw l2                           3.23e-01  2.76e-01  2.50e-03
  up2_w16 dy1e-7 S1                  dgamma                          2.28e-01  2.45e-04  5.00e-03
  up2_w16 dy1e-7 S1                  dgamma l2                       1.90e-01  2.31e-04  2.50e-03
  up2_w16 dy1e-7 S1                  dbeta                           1.97e-01  7.56e-08  5.00e-03
  up2_w16 dy1e-7 S1                  dbeta l2                        1.63e-01  5.57e-08  2.50e-03
  up2_w16 dy1e-7 S1                  dx2                             4.27e-01  3.42e-01  5.00e-03
  up2_w16 dy1e-7 S1                  dx2 l2                          4.35e-01  4.07e-01  2.50e-03
  up2_w16 dy1e-7 S1                  dx                              3.52e-01  3.03e-01  5.00e-03
  up2_w16 dy1e-7 S1                  dx l2                           3.86e-01  3.48e-01  2.50e-03
  lrelu_k4s2_cin104 dy1e-7 S1        mask flips (fraction)                  -  0.00e+00  2.00e-03
  lrelu_k4s2_cin104 dy1e-7 S1        mask flips beyond one rounding         -  0.00e+00  0.00e+00
  lrelu_k4s2_cin104 dy1e-7 S1        fwd                             2.89e-04  2.89e-04  8.67e-04
  lrelu_k4s2_cin104 dy1e-7 S1        dw                              2.27e-01  1.48e-01  5.00e-03
  lrelu_k4s2_cin104 dy1e-7 S1        dw l2                           2.32e-01  1.56e-01  2.50e-03
  lrelu_k4s2_cin104 dy1e-7 S1        dbias                           1.75e-01  5.37e-08  5.00e-03
  lrelu_k4s2_cin104 dy1e-7 S1        dbias l2                        1.45e-01  5.24e-08  2.50e-03
  lrelu_k4s2_cin104 dy1e-7 S1        dx                              3.82e-01  3.29e-01  5.00e-03
  lrelu_k4s2_cin104 dy1e-7 S1        dx l2                           5.02e-01  4.61e-01  2.50e-03
  ovf_bare_cb8 bwd (outside the reach) fwd                             2.55e-04  2.55e-04  7.65e-04
  ovf_bare_cb8 bwd (outside the reach) dx                              3.78e-04  2.85e-04  1.13e-03
  ovf_bare_cb8 bwd (outside the reach) dx l2                           2.92e-04  2.07e-04  8.76e-04
  ovf_bare_cb8 bwd (outside the reach) dw                              2.46e-04  1.10e-07  7.38e-04
  ovf_bare_cb8 bwd (outside the reach) dw l2                           2.06e-04  5.75e-08  6.19e-04
  ovf_bare_cb8 bwd (outside the reach) dbias                           1.27e-04  0.00e+00  3.80e-04
  ovf_bare_cb8 bwd (outside the reach) dbias l2                        1.68e-04  0.00e+00  5.04e-04
  ovf_bare_cb8 fwd (outside the reach) fwd                             2.55e-04  2.55e-04  7.65e-04
  ovf_bare_cb8 fwd (outside the reach) dx                              3.78e-04  2.52e-04  1.13e-03
  ovf_bare_cb8 fwd (outside the reach) dx l2                           2.92e-04  2.08e-04  8.76e-04
  ovf_bare_cb8 fwd (outside the reach) dw                              2.46e-04  1.10e-07  7.38e-04
  ovf_bare_cb8 fwd (outside the reach) dw l2                           2.06e-04  5.74e-08  6.19e-04
  ovf_bare_cb8 fwd (outside the reach) dbias                           1.27e-04  0.00e+00  3.80e-04
  ovf_bare_cb8 fwd (outside the reach) dbias l2                        1.68e-04  0.00e+00  5.04e-04
  ovf_lrelu bwd (outside the reach)  fwd                             2.94e-04  2.94e-04  8.83e-04
  ovf_lrelu bwd (outside the reach)  dx                              3.38e-04  2.49e-04  1.01e-03
  ovf_lrelu bwd (outside the reach)  dx l2                           2.90e-04  2.08e-04  8.70e-04
  ovf_lrelu bwd (outside the reach)  dw                              2.36e-04  4.09e-05  7.09e-04
  ovf_lrelu bwd (outside the reach)  dw l2                           2.05e-04  3.85e-05  6.15e-04
  ovf_lrelu bwd (outside the reach)  dbias                           1.26e-04  4.12e-08  3.79e-04
  ovf_lrelu bwd (outside the reach)  dbias l2                        1.26e-04  4.84e-08  3.77e-04
  ovf_lrelu fwd (outside the reach)  fwd                             2.94e-04  2.96e-04  8.83e-04
  ovf_lrelu fwd (outside the reach)  dx                              3.38e-04  2.49e-04  1.01e-03
  ovf_lrelu fwd (outside the reach)  dx l2                           2.90e-04  2.12e-04  8.70e-04
  ovf_lrelu fwd (outside the reach)  dw                              2.36e-04  4.20e-05  7.09e-04
  ovf_lrelu fwd (outside the reach)  dw l2                           2.05e-04  3.84e-05  6.15e-04
  ovf_lrelu fwd (outside the reach)  dbias                           1.26e-04  4.94e-08  3.79e-04
  ovf_lrelu fwd (outside the reach)  dbias l2                        1.26e-04  4.55e-08  3.77e-04
  ovf_bare_f32 bwd (outside the reach) fwd                             0.00e+00  1.74e-07  2.00e-05
  ovf_bare_f32 bwd (outside the reach) dx                              3.84e-04  3.35e-04  1.15e-03
  ovf_bare_f32 bwd (outside the reach) dx l2                           2.89e-04  2.05e-04  8.68e-04
  ovf_bare_f32 bwd (outside the reach) dw                              2.07e-04  1.05e-07  6.21e-04
  ovf_bare_f32 bwd (outside the reach) dw l2                           2.10e-04  5.62e-08  6.29e-04
  ovf_bare_f32 bwd (outside the reach) dbias                           0.00e+00  3.42e-08  1.00e-04
  ovf_bare_f32 bwd (outside the reach) dbias l2                        0.00e+00  3.51e-08  1.00e-04
  ovf_bare_f32 fwd (outside the reach) fwd                             0.00e+00  1.74e-07  2.00e-05
  ovf_bare_f32 fwd (outside the reach) dx                              3.84e-04  2.52e-04  1.15e-03
  ovf_bare_f32 fwd (outside the reach) dx l2                           2.89e-04  2.06e-04  8.68e-04
  ovf_bare_f32 fwd (outside the reach) dw                              2.07e-04  1.05e-07  6.21e-04
  ovf_bare_f32 fwd (outside the reach) dw l2                           2.10e-04  5.56e-08  6.29e-04
  ovf_bare_f32 fwd (outside the reach) dbias                           0.00e+00  5.62e-08  1.00e-04
  ovf_bare_f32 fwd (outside the reach) dbias l2                        0.00e+00  4.46e-08  1.00e-04
  MEASURED_TABLE_END
"""
import contextlib
import re

import pytest
import torch
import torch.nn.functional as F

from helpers import round16_model as M
from helpers.fp16_block_table import TABLE, BY_ID, SCALED, TINY_DY, LOSS_SCALES, OVERFLOW

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = torch.float16
NAMES_F16 = re.compile(r'(?<![a-z0-9])f16(?![0-9])')
NAMES_BF16 = re.compile(r'bf16')


@contextlib.contextmanager
def _bn_fused(v):
  from mix_stage_amd import _lib
  L = _lib.lib()
  prev = L.ms_debug_set_bn_fused(v) if v is not None else None
  try:
    yield
  finally:
    if v is not None:
      L.ms_debug_set_bn_fused(prev)


def _check_labels(c, labels):
  typed = [l for l in labels if NAMES_F16.search(l) or NAMES_BF16.search(l)]
  assert typed and not [l for l in typed if NAMES_BF16.search(l)], (c['id'], sorted(set(labels)))
  missing = [rx for rx in c['expect'] if not any(re.search(rx, l) for l in labels)]
  present = [(rx, l) for rx in c['forbid'] for l in labels if re.search(rx, l)]
  assert not missing and not present, (c['id'], missing, present, sorted(set(labels)))
  bn_own = [l for l in labels if re.search(r'bn_(finalize_)?apply16', l)]
  if c['bn_fused'] == 1:
    assert not bn_own, ('in-launch BatchNorm expected', sorted(set(labels)))
  if c['bn_fused'] == 0:
    assert bn_own, ('two-launch BatchNorm expected', sorted(set(labels)))


def _run(c, dy_scale=1.0, loss_scale=1.0, check=True, bar_model=None):
  from test_gpu_kernels16 import _case
  from test_gpu_dispatch_parity import _timed
  nd = c['nd']
  H, W = c['sp'] if nd == 2 else (1, c['sp'][0])
  labels = []
  with _bn_fused(c['bn_fused']), _timed(labels):
    measured = _case(nd, c['B'], c['cin'], c['cout'], c['groups'], c['k'], c['s'], c['p'], H, W, M.MODES[c['mode']],
                     M.IN_MODES[c['in_mode']], c['out_f32'], dt=DT, seed=c['seed'], fragile=c['fragile'], slope=c['slope'],
                     grad_tol=c['grad_tol'], mask=c['mask'], bars='dtype', dy_scale=dy_scale, loss_scale=loss_scale,
                     two_launch=c['bn_fused'] == 0, check=check, bar_model=bar_model)
  _check_labels(c, labels)
  return measured


def _report(tag, measured, model):
  for k, (v, bar) in measured.items():
    print('  %-34s %-30s %9s %9.2e %9.2e' % (tag, k, '%9.2e' % model[k] if k in model else '-', v, bar))


@pytest.mark.parametrize('c', TABLE, ids=[c['id'] for c in TABLE])
def test_fp16_training_block_matches_fp64(c):
  measured = _run(c)
  _report(c['id'], measured, M.case_model(c, DT))


@pytest.mark.parametrize('S', LOSS_SCALES, ids=['S2^16', 'S2^10'])
@pytest.mark.parametrize('cid', SCALED)
def test_tiny_gradients_carried_by_the_loss_scale(cid, S):
  c = BY_ID[cid]
  measured = _run(c, dy_scale=TINY_DY, loss_scale=S, bar_model=M.case_model(c, DT))      # the bars of the unit-size gradient
  _report('%s dy1e-7 S%g' % (cid, S), measured, M.case_model(c, DT, S=S, dy_scale=TINY_DY))


@pytest.mark.parametrize('cid', SCALED)
def test_tiny_gradients_unscaled_are_measured(cid):
  """S = 1: measured and printed beside the model's prediction (the gradients are lost in both), not asserted; the forward pass does
  not see the gradient and keeps its bar."""
  c = BY_ID[cid]
  measured = _run(c, dy_scale=TINY_DY, loss_scale=1.0, check=False)
  _report('%s dy1e-7 S1' % cid, measured, M.case_model(c, DT, S=1.0, dy_scale=TINY_DY))
  assert measured['fwd'][0] <= measured['fwd'][1]


# ------------------------------------------------------------------------------------------------ overflow must stay visible
B0, C0, T0 = 1, 3, 5            # the overflowed element: batch item, channel (output channel of dy / input channel of x), column
OVF_S = 2.0 ** 10


def _overflow(c, kind):
  """kind 'bwd': S * dy[B0, C0, T0] = 1e5 > 65504; kind 'fwd': x[B0, C0, T0] = 7e4, which rounds to inf.  -> rows for the report."""
  from mix_stage_amd import ops, ops16, _lib
  from mix_stage_amd._lib import MS_F16
  from test_gpu_kernels16 import dtype_bar
  mode, out_f32, k, s, p = M.MODES[c['mode']], c['out_f32'], c['k'], c['s'], c['p']
  W = c['sp'][0]
  o, dy = M.case_tensors(c)
  S = OVF_S
  model = M.block_model(o, dy, 1, 1, s, p, mode, M.PLAIN, 0.2, out_f32, DT, S, mask='device' if mode == M.LRELU else 'exact')
  OW = dy.shape[2]
  reach = {kk: None for kk in ('y', 'dx', 'dw', 'dbias')}
  if kind == 'bwd':
    dy[B0, C0, T0] = 1e5 / S
    cols = [T0 * s - p + j for j in range(k) if 0 <= T0 * s - p + j < W]
    reach['dx'] = torch.zeros(o['x'].shape, dtype=torch.bool); reach['dx'][B0, :, cols] = True
    reach['dw'] = torch.zeros(o['w'].shape, dtype=torch.bool); reach['dw'][C0] = True
    if not out_f32:      # (an fp32 dy is summed as it arrives: S * dy = 1e5 is finite there, only its cb8 conversion overflows)
      reach['dbias'] = torch.zeros(o['bias'].shape, dtype=torch.bool); reach['dbias'][C0] = True
  else:
    o['x'][B0, C0, T0] = 7e4
    cols = [q for q in range(OW) if 0 <= T0 - (q * s - p) < k]
    reach['y'] = torch.zeros(dy.shape, dtype=torch.bool); reach['y'][B0, :, cols] = True
    reach['dw'] = torch.zeros(o['w'].shape, dtype=torch.bool); reach['dw'][:, C0] = True

  # ---- device
  x = o['x'].to(DEV).requires_grad_()
  wp, bp = o['w'].to(DEV).requires_grad_(), o['bias'].to(DEV).requires_grad_()
  y = ops16.conv_block16(ops16.to_cb8(x, MS_F16), wp, bp, ops.ConvGeom(1, 1, k, s, p, slope=0.2), mode, out_f32=out_f32)
  y32 = y if out_f32 else ops16.from_cb8(y, c['cout'])
  # (the seed of the backward pass: y32's gradient is S * dy; the non-finite y of the forward case must not reach the sum)
  y32.backward(dy.to(DEV) * S)
  dev = dict(y=y32.detach(), dx=x.grad / S, dw=wp.grad / S, dbias=bp.grad / S)
  norm = torch.zeros(1, device=DEV)
  part = torch.zeros(_lib.lib().ms_reduce_partials_count(wp.grad.numel()), device=DEV)
  ops.grad_norm(wp.grad.reshape(-1), norm, part)
  torch.cuda.synchronize()
  assert not torch.isfinite(norm).item(), ('ms_sqnorm of dw', norm.item())

  # ---- fp64 on the same rounded operands, inf included (torch's cast, as in _case)
  r16 = lambda t: t.to(DT).double()
  w64, b64 = r16(o['w']).requires_grad_(), o['bias'].double().requires_grad_()
  xin = r16(o['x']).requires_grad_()
  raw = F.conv1d(xin, w64, b64, stride=s, padding=p)
  ref_y = torch.where(dev['y'].cpu() > 0, raw, 0.2 * raw) if mode == M.LRELU else raw      # (slopes follow the device's signs)
  ref_y.backward(r16(dy * S) / S)                  # out_f32 too: the dyr conversion is where its overflow happens
  ref = dict(y=ref_y.detach(), dx=xin.grad, dw=w64.grad, dbias=dy.double().sum((0, 2)) if out_f32 else b64.grad)

  gt = 2e-2 if (mode == M.LRELU or not out_f32) else 1e-2
  rows = []
  for kk in ('y', 'dx', 'dw', 'dbias'):
    a, b = dev[kk].detach().cpu().double(), ref[kk]
    inside = reach[kk] if reach[kk] is not None else torch.zeros(b.shape, dtype=torch.bool)
    bad_ref = ~torch.isfinite(b)
    assert not (bad_ref & ~inside).any(), (kk, 'the reference is non-finite outside the geometric reach')
    assert (bad_ref.any().item()) == (reach[kk] is not None), (kk, 'reach without a non-finite reference element, or the reverse')
    assert torch.isfinite(a[bad_ref]).sum().item() == 0, (kk, 'finite on the device where the reference is not',
                                                        int(torch.isfinite(a[bad_ref]).sum()), int(bad_ref.sum()))
    ao, bo = a[~inside], b[~inside]
    assert torch.isfinite(ao).all(), (kk, 'non-finite outside the reach', int((~torch.isfinite(ao)).sum()))
    sc = bo.abs().max().item() + (1e-6 if kk == 'y' else 1e-9)
    e, l2 = (ao - bo).abs().max().item() / sc, (ao - bo).norm().item() / (bo.norm().item() + 1e-12)
    if kk == 'y':
      bar = 2e-5 if out_f32 else dtype_bar(1.2e-2, model['fwd'])
      rows.append(('fwd', model['fwd'], e, bar))
      assert e <= bar, (kk, e, bar)
    else:
      bmax, bl2 = dtype_bar(2 * gt, model[kk]) + 1e-6 / sc, dtype_bar(gt, model[kk + ' l2'])      # (_case's rule)
      rows += [(kk, model[kk], e, bmax), (kk + ' l2', model[kk + ' l2'], l2, bl2)]
      assert e <= bmax and l2 <= bl2, (kk, e, bmax, l2, bl2)
  return rows


@pytest.mark.parametrize('kind', ['bwd', 'fwd'])
@pytest.mark.parametrize('c', OVERFLOW, ids=[c['id'] for c in OVERFLOW])
def test_overflow_stays_visible(c, kind):
  for what, mod, v, bar in _overflow(c, kind):
    print('  %-34s %-30s %9.2e %9.2e %9.2e' % ('%s %s (outside the reach)' % (c['id'], kind), what, mod, v, bar))
