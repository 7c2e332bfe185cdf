"""The fp16 training blocks of tests/test_gpu_block16_fp16.py: plain data (no torch, no GPU), shared with
tests/test_round16_model_cpu.py, which holds every case and seed to the two conditions a case must meet to separate fp16 from
bf16 (emulated bf16 / fp16 error in [5, 12]; at most flip_frac / 2 of the pre-activations inside the kink band).

Sizes are the smallest that still cross the edge a case exists for: a tile, a parity class, a group, a pad channel."""

BARE, LRELU, BN_TRAIN = 'BARE', 'LRELU', 'BN_TRAIN'


# expect / forbid: regular expressions over the launch labels of the case (the launches it exists for took place)
def C(id, nd, B, cin, cout, k, s, p, sp, mode=BN_TRAIN, groups=1, in_mode='plain', out_f32=False, seed=0, bn_fused=None,
      fragile=False, slope=0.2, grad_tol=None, mask=None, expect=(), forbid=(), why=''):
  return dict(id=id, nd=nd, B=B, cin=cin, cout=cout, k=k, s=s, p=p, sp=sp, mode=mode, groups=groups, in_mode=in_mode,
              out_f32=out_f32, seed=seed, bn_fused=bn_fused, fragile=fragile, slope=slope, grad_tol=grad_tol,
              mask=mask or ('device' if mode in (BN_TRAIN, LRELU) else 'exact'), expect=expect, forbid=forbid, why=why)


TABLE = [
    # ---- in-launch and two-launch BatchNorm; the 128-row tile
    C('k3_bn_in_launch', 1, 4, 64, 64, 3, 1, 1, (16,), bn_fused=1, seed=1, why='BatchNorm inside the conv launch'),
    C('k3_bn_two_launch', 1, 4, 64, 64, 3, 1, 1, (16,), bn_fused=0, seed=1, why='BatchNorm as its own launch, from the stored y_raw'),
    C('k3_c256', 1, 2, 256, 256, 3, 1, 1, (64,), seed=2, why='the 128-row tile'),
    # ---- parity classes of unequal extent
    C('k4s2_w16', 1, 4, 64, 64, 4, 2, 1, (16,), seed=1, why='two parity classes'),
    C('k4s2_w4', 1, 4, 64, 64, 4, 2, 1, (4,), why='parity classes at two output columns'),
    C('k4s2_16to24_w37', 1, 3, 16, 24, 4, 2, 1, (37,), why='odd width: parity classes of unequal extent'),
    # ---- upsample-add input
    C('up2_w16', 1, 4, 64, 64, 3, 1, 1, (16,), in_mode='up2', seed=3, why='upsample-add input, both data gradients'),
    C('up2_w2', 1, 4, 64, 64, 3, 1, 1, (2,), in_mode='up2', seed=1, why='upsample-add at one coarse column'),
    # ---- broadcast and grouped inputs
    C('bcast_g3', 1, 3, 10, 16, 3, 1, 1, (19,), groups=3, in_mode='bcast', seed=1, why='one input read by 3 groups; cin 10 pads to 16'),
    C('grouped_g3', 1, 3, 16, 24, 3, 1, 1, (19,), groups=3, seed=1, why='3 groups of 16 -> 24'),
    C('grouped_bare_k1', 1, 3, 16, 104, 1, 1, 0, (19,), mode=BARE, groups=2, out_f32=True, why='grouped fp32 scores'),
    # ---- pad channels and score outputs
    C('cin74', 1, 3, 74, 64, 3, 1, 1, (16,), seed=2, why='cin not a multiple of 8'),
    C('cin104', 1, 3, 104, 64, 3, 1, 1, (16,), why='cin not a multiple of 16'),
    C('cout5_f32', 1, 4, 64, 5, 4, 2, 1, (2,), out_f32=True, why='5 fp32 output channels, one output column'),
    C('bare_cout1', 1, 4, 256, 1, 4, 1, 0, (15,), mode=BARE, out_f32=True, seed=1, why='one fp32 score channel'),
    C('lrelu_k4s2_cin104', 1, 4, 104, 64, 4, 2, 1, (16,), mode=LRELU, why='LeakyReLU block (discriminator conv1)'),
    # ---- 2-D
    C('2d_c1_3x3', 2, 2, 1, 64, 3, 1, 1, (10, 12), seed=2, expect=(r'^wgrad16_c1_kernel<f16>', r'^conv16_kernel<f16,'),
      forbid=(r'^conv16_c1_3x3_kernel',), why='wgrad16_c1; the matrix-pipe forward at cin = 1 in train mode'),
    C('2d_k4s2', 2, 2, 16, 32, 4, 2, 1, (10, 14), seed=3, why='2-D parity classes'),
    C('2d_k3x8', 2, 2, 16, 32, (3, 8), 1, (1, 3), (8, 16), seed=5, why='non-square kernel, unequal padding'),
    C('2d_k3_c128', 2, 2, 64, 128, 3, 1, 1, (8, 16), why='2-D 128-row tile'),
    # ---- the y / y_raw choice (test_block16_bn_backward_reads_y_or_y_raw_per_channel_block): the y_raw path takes the activation
    # mask from the ROUNDED conv output, which the model follows (round16_model.py: xhat_mask); that test's l2 rail of 3e-2 takes
    # the place of the bf16 bar, so fp16 gets the smaller of it x 2^-3 and 3 x the model, like every other case.  Both run with
    # the exact mask: the seeds are ones at which no fp16 mask differs from exact math (test_round16_model_cpu.py holds them to it)
    C('fragile', 1, 4, 64, 64, 3, 1, 1, (16,), fragile=True, grad_tol=3e-2, mask='exact', seed=2, why='channels that do not invert from y'),
    C('relu_slope0', 1, 4, 64, 64, 3, 1, 1, (16,), slope=0.0, grad_tol=3e-2, mask='exact', seed=1, why='nothing inverts: y_raw everywhere'),
]

BY_ID = {c['id']: c for c in TABLE}

# ---- part 4: gradients that need the loss scale (dy elements of size 1e-7, far inside fp16's subnormal range)
SCALED = ['k3_bn_in_launch', 'k4s2_w16', 'up2_w16', 'lrelu_k4s2_cin104']
TINY_DY = 1e-7
LOSS_SCALES = [2.0 ** 16, 2.0 ** 10]

# ---- part 5: overflow must stay visible (no BatchNorm, which would spread it)
OVERFLOW = [
    C('ovf_bare_cb8', 1, 4, 64, 64, 3, 1, 1, (16,), mode=BARE),
    C('ovf_lrelu', 1, 4, 64, 64, 4, 2, 1, (16,), mode=LRELU),
    C('ovf_bare_f32', 1, 4, 64, 8, 3, 1, 1, (16,), mode=BARE, out_f32=True),
]
