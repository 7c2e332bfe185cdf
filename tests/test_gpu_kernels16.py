"""GPU: the 16-bit arithmetic mode (bf16 / fp16 operands on v_mfma_f32_32x32x16, fp32 accumulate; cb8 tensors) block by
block through the C-ABI, against an fp64 reference evaluated on the SAME 16-bit-rounded operands -- what is left is the
accumulation order, so the fp32 outputs (scores, weight gradients, statistics) are checked tightly and the 16-bit outputs to
one rounding of the output type."""
import pytest
import torch
import torch.nn.functional as F

from helpers import round16_model as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32_GRAD_BAR = 1e-4
MODEL_K = 3          # bars='dtype': fp16 bars are MODEL_K x the reference's own emulated rounding error (bf16-grade lands at ~8 x)

BARE, LRELU, BN_TRAIN, BN_EVAL = 0, 1, 2, 3
PLAIN, BCAST, UP2 = 0, 1, 2


def dtype_bar(legacy, model_value):
  """The fp16 bar of bars='dtype' for one 16-bit-limited check: `legacy` is the bf16-sized bar without its absolute floor,
  `model_value` the reference's own emulated error for the check (helpers/round16_model.py)."""
  if model_value == 0.0:
    # no 16-bit tensor enters this result (bias / beta gradient of an fp32 dy): fp32-limited, it differs from fp64 by the order
    # of an fp32 sum -- held to the bar the fp32 blocks have for their gradients (test_gpu_kernels._conv_block_case)
    return min(legacy, F32_GRAD_BAR)
  return min(legacy / 8, MODEL_K * model_value)


def _round(t, dt):
  return t.to(dt).to(torch.float64)


def _case(nd, B, cin, cout, groups, k, s, p, H, W, mode, in_mode=PLAIN, out_f32=False, dt=torch.bfloat16, seed=0, fragile=False,
          slope=0.2, grad_tol=None, mask='exact', ref_dev='cpu', bn_folded=False, flip_frac=2e-3, keep=None, bars='legacy',
          dy_scale=1.0, loss_scale=1.0, two_launch=False, check=True, bar_model=None):
  """One 16-bit block against fp64 on its rounded operands.  Returns {check: (measured, bar)}, values relative to the
  reference's max-abs.

  mask='device': the reference's LeakyReLU takes its slope from the sign of the device output.  Where the BatchNorm runs in a
  launch of its own it normalises the STORED 16-bit conv output, so a pre-activation within one 16-bit rounding of 0 may take
  the other slope than in exact math; such elements (at most `flip_frac` of the output, each within one rounding of the conv
  output -- carried through BatchNorm's affine map -- of 0) follow the device, and every bar stays as it is.
  ref_dev: where the float64 reference runs.  bn_folded: eval BatchNorm folded into the weights (the inference form).
  keep: a dict that receives the device tensors of the run (output, every gradient, running statistics, save).

  bars='legacy': the bars every type had so far (sized for bf16).  bars='dtype': bf16 keeps them; for fp16 every 16-bit-limited
  check (forward of cb8 outputs and of BN_TRAIN, every gradient's max and l2) gets the smaller of the legacy bar x 2^-3 and
  MODEL_K x the error that helpers/round16_model.py emulates for that check on this case's tensors, plus the legacy absolute
  floor; a caller's grad_tol takes the place of the legacy gradient bar in that rule (and, as the model knows the masks of the
  y_raw path, the max-abs check that the legacy form of such a call leaves out gets its bar too).  The
  fp32-limited checks (out_f32 forward outside BN_TRAIN, running statistics) keep their bars; a gradient that no 16-bit tensor
  enters (model figure 0: the bias / beta gradient of an fp32 dy) is fp32-limited too and gets F32_GRAD_BAR, the fp32 blocks' bar.
  dy_scale: size of the incoming gradient's elements.  loss_scale: S -- the device backward is seeded with S * dy, every device
  gradient is divided by S before it is compared, and the reference uses round16(S * dy) / S.  (The absolute floor of the
  max-abs gradient bars, 1e-6, is an fp32-accumulation allowance for gradients of order 1: it shrinks with dy_scale below 1.)
  two_launch: tells the model that BatchNorm normalises the stored 16-bit conv output (the caller switched the in-launch form
  off).  check=False: measure only -- nothing about the gradients or the forward error is asserted.
  bar_model: a {check: emulated error} to take the fp16 bars from instead of this run's own model -- the unit-scale model of the
  block, for runs with a dy_scale and a loss scale that are held to the bars of unit-size gradients."""
  from mix_stage_amd import ops, ops16
  from mix_stage_amd._lib import MS_BF16, MS_F16
  msdt = MS_BF16 if dt == torch.bfloat16 else MS_F16
  # (the tensors come from the helper the CPU model tests draw from: same generator, same order as ever)
  opnd = M.gen_operands(nd, B, cin, cout, groups, k, s, p, H, W, in_mode, seed, fragile)
  w, bias, gamma, beta, rm, rv = (opnd[n].to(DEV) for n in ('w', 'bias', 'gamma', 'beta', 'rm', 'rv'))
  if in_mode == UP2:
    a = opnd['a'].to(DEV).requires_grad_()
    r = opnd['r'].to(DEV).requires_grad_()
    xa, xr = ops16.to_cb8(a, msdt), ops16.to_cb8(r, msdt)
  else:
    x = opnd['x'].to(DEV).requires_grad_()
    xc = ops16.to_cb8(x, msdt)
  wp = w.clone().requires_grad_(); bp = bias.clone().requires_grad_()
  gp = gamma.clone().requires_grad_(); bep = beta.clone().requires_grad_()
  rm_h, rv_h = rm.clone(), rv.clone()
  geom = ops.ConvGeom(nd, groups, k, s, p, slope=slope)
  bn = mode in (BN_TRAIN, BN_EVAL)
  kw = dict(gamma=gp if bn else None, beta=bep if bn else None, running_mean=rm_h if bn else None,
            running_var=rv_h if bn else None, out_f32=out_f32)
  if in_mode == UP2:
    y = ops16.conv_block16(xa, wp, bp, geom, mode, x2=xr, in_mode=UP2, **kw)
  else:
    y = ops16.conv_block16(xc, wp, bp, geom, mode, in_mode=in_mode, bn_folded=bn_folded, **kw)
  ctot = cout * groups
  y32 = y if out_f32 else ops16.from_cb8(y, ctot)
  S = float(loss_scale)
  dy_cpu = M.gen_dy(opnd, y32.shape, dy_scale)
  dyv = dy_cpu.to(DEV)
  if keep is not None:
    fn = y.grad_fn
    keep.update(y=y.detach(), save=fn.saved_tensors[6] if (fn is not None and type(fn).__name__ == '_ConvBlock16FnBackward') else None)
  if mode != BN_EVAL:
    (y32 * (dyv if S == 1.0 else dyv * S)).sum().backward()
  if keep is not None:
    keep.update(dw=wp.grad, dbias=bp.grad, dgamma=gp.grad, dbeta=bep.grad, running_mean=rm_h, running_var=rv_h)
    keep.update(dx0=a.grad, dx1=r.grad) if in_mode == UP2 else keep.update(dx0=x.grad)

  # ---- fp64 reference on the rounded operands
  rdev = ref_dev
  w64 = _round(w.to(rdev), dt).requires_grad_()
  b64 = bias.to(rdev).double().requires_grad_()
  if in_mode == UP2:
    a64, r64 = _round(a.detach().to(rdev), dt), _round(r.detach().to(rdev), dt)
    xin = _round((a64.repeat_interleave(2, dim=-1) + r64).float(), dt).requires_grad_()
  else:
    xin = _round(x.detach().to(rdev), dt).requires_grad_()
  xcat = torch.cat([xin] * groups, 1) if in_mode == BCAST else xin
  conv = F.conv2d if nd == 2 else F.conv1d
  raw = conv(xcat, w64, b64, stride=s, padding=p, groups=groups)
  g64 = gamma.to(rdev).double().requires_grad_(); be64 = beta.to(rdev).double().requires_grad_()
  dims = (0, 2, 3) if nd == 2 else (0, 2)
  shape = (1, -1, 1, 1) if nd == 2 else (1, -1, 1)
  if mode == BN_TRAIN:
    # statistics AND (in-launch BatchNorm) the normalisation come from the fp32 accumulators; the backward pass takes x_hat and the
    # LeakyReLU mask from the 16-bit output y, whose sign is the true sign of z: plain fp64 math is the reference (a
    # straight-through rounding of `raw`, which the two-launch form of round 2 needed mirrored here, would be the wrong model)
    mean, var = raw.mean(dims), raw.var(dims, unbiased=False)
    raw_r = raw
    z = (raw_r - mean.view(shape)) / torch.sqrt(var.view(shape) + 1e-5) * g64.view(shape) + be64.view(shape)
    zscale = g64.detach().abs() / torch.sqrt(var.detach() + 1e-5)
    ref = F.leaky_relu(z, slope)
  elif mode == BN_EVAL:
    z = (raw - rm.to(rdev).double().view(shape)) / torch.sqrt(rv.to(rdev).double().view(shape) + 1e-5) * g64.view(shape) + be64.view(shape)
    zscale = g64.detach().abs() / torch.sqrt(rv.to(rdev).double() + 1e-5)
    ref = F.leaky_relu(z, 0.2)
  elif mode == LRELU:
    z, zscale = raw, torch.ones(ctot, dtype=torch.float64, device=raw.device)
    ref = F.leaky_relu(raw, 0.2)
  else:
    ref = raw
  measured = {}      # (returned: check -> (measured, bar), relative to the reference's max-abs)
  if mask == 'device' and mode != BARE:
    pos = y32.detach().to(rdev) > 0
    flip = pos != (z.detach() > 0)
    u16 = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    zmax = z.detach().abs().max().item()
    band = u16 * raw.detach().abs() * zscale.view(shape) + 1e-5 * zmax      # one rounding of the conv output, in units of z
    outside = (flip & (z.detach().abs() > band)).sum().item()
    frac = flip.sum().item() / flip.numel()
    measured['mask flips (fraction)'] = (frac, flip_frac)
    measured['mask flips beyond one rounding'] = (outside, 0)
    assert outside == 0 and frac <= flip_frac, ('mask', flip.sum().item(), flip.numel(), outside)
    sl = slope if mode == BN_TRAIN else 0.2
    ref = torch.where(pos, z, sl * z)
  if mode != BN_EVAL:
    # cb8 outputs receive a 16-bit gradient: S * dy rounded once
    dy_used = dyv.to(rdev).double() if out_f32 else _round(dyv.to(rdev) * S, dt) / S
    (ref * dy_used).sum().backward()

  model = None
  assert bars in ('legacy', 'dtype'), bars
  if bars == 'dtype' and dt == torch.float16:
    model = bar_model if bar_model is not None else M.block_model(
        opnd, None if mode == BN_EVAL else dy_cpu, nd, groups, s, p, mode, in_mode, slope, out_f32, dt, S, rdev, two_launch, mask,
        bn_folded)
  def bar16(legacy, what):
    # (`legacy` without its absolute floor)
    return dtype_bar(legacy, model[what]) if model is not None else legacy

  fp32_fwd = out_f32 and mode != BN_TRAIN
  out_tol = 2e-5 if fp32_fwd else bar16(1.2e-2, 'fwd')      # fp32 from the accumulators vs one 16-bit rounding
  scale = ref.abs().max().item() + 1e-6
  err = (y32.detach().to(rdev).double() - ref.detach()).abs().max().item()
  measured['fwd'] = (err / scale, out_tol)
  assert not check or err <= out_tol * scale, ('forward', err, scale, out_tol)
  if mode == BN_TRAIN:
    n = raw.numel() // ctot
    new_rm = 0.9 * rm.to(rdev).double() + 0.1 * mean.detach()
    new_rv = 0.9 * rv.to(rdev).double() + 0.1 * raw.detach().var(dims, unbiased=True) if n > 1 else None
    assert (rm_h.to(rdev).double() - new_rm).abs().max().item() <= 1e-4
    if new_rv is not None:
      assert (rv_h.to(rdev).double() - new_rv).abs().max().item() <= 2e-3 * (1 + new_rv.abs().max().item())
  # gradients: dy went through a 16-bit rounding (cb8 outputs) and BN backward rounds dy_raw again
  gt = grad_tol or (2e-2 if mode in (BN_TRAIN, LRELU) or not out_f32 else 1e-2)
  floor = 1e-6 * min(1.0, dy_scale)
  def close(a, b, what, tol=gt):
    sc = b.abs().max().item() + 1e-9
    a = a.detach().to(rdev).double() / S
    e = (a - b).abs().max().item()
    l2 = (a - b).norm().item() / (b.norm().item() + 1e-12)
    if grad_tol and model is None:
      bmax, bl2 = float('inf'), tol
    else:
      bmax, bl2 = bar16(2 * tol, what) + floor / sc, bar16(tol, what + ' l2')
    measured[what] = (e / sc, bmax)
    measured[what + ' l2'] = (l2, bl2)
    # (a wrongly masked element -- y_raw path, |z| below one rounding -- is off by the LeakyReLU factor: bounded in l2, not in max)
    assert not check or (e / sc <= bmax and l2 <= bl2), (what, e, sc, l2, bmax, bl2)
  if mode != BN_EVAL:
    close(wp.grad, w64.grad, 'dw')
    if mode != BN_TRAIN:
      close(bp.grad, b64.grad, 'dbias')
    else:
      close(gp.grad, g64.grad, 'dgamma'); close(bep.grad, be64.grad, 'dbeta')
    if in_mode == UP2:
      dxin = xin.grad
      close(r.grad, dxin, 'dx2')
      close(a.grad, dxin.reshape(dxin.shape[0], dxin.shape[1], -1, 2).sum(-1), 'dx')
    else:
      close(x.grad, xin.grad, 'dx')
  return measured


CASES_1D = [
    # name, B, cin, cout, groups, k, s, p, W, mode, in_mode, out_f32
    ('dec1', 8, 128, 128, 4, 3, 1, 1, 64, BN_TRAIN, PLAIN, False),
    ('dec0_bcast', 8, 74, 128, 4, 3, 1, 1, 64, BN_TRAIN, BCAST, False),
    ('unet_pre', 4, 256, 256, 1, 3, 1, 1, 64, BN_TRAIN, PLAIN, False),
    ('unet_down', 4, 64, 64, 1, 4, 2, 1, 64, BN_TRAIN, PLAIN, False),
    ('unet_deep', 6, 64, 64, 1, 4, 2, 1, 4, BN_TRAIN, PLAIN, False),
    ('unet_up2', 4, 64, 64, 1, 3, 1, 1, 16, BN_TRAIN, UP2, False),
    ('unet_up2_t2', 4, 64, 64, 1, 3, 1, 1, 2, BN_TRAIN, UP2, False),
    ('pse0', 4, 104, 64, 1, 3, 1, 1, 64, BN_TRAIN, PLAIN, False),
    ('pse_last', 6, 64, 5, 1, 4, 2, 1, 2, BN_TRAIN, PLAIN, True),
    ('cls0', 4, 266, 256, 1, 3, 1, 1, 64, BN_TRAIN, PLAIN, False),
    ('cls_logits', 4, 256, 8, 1, 1, 1, 0, 64, BARE, PLAIN, True),
    ('logits_g', 4, 64, 104, 4, 1, 1, 0, 64, BARE, PLAIN, True),
    ('d_conv1', 4, 104, 64, 1, 4, 2, 1, 64, LRELU, PLAIN, False),
    ('d_conv3', 4, 128, 256, 1, 4, 1, 1, 16, BN_TRAIN, PLAIN, False),
    ('d_logits', 4, 256, 1, 1, 4, 1, 0, 15, BARE, PLAIN, True),
    ('eval_k3', 4, 64, 64, 1, 3, 1, 1, 64, BN_EVAL, PLAIN, False),
    ('bare_cb8', 4, 64, 64, 1, 3, 1, 1, 32, BARE, PLAIN, False),
    ('t256', 2, 64, 128, 2, 3, 1, 1, 256, BN_TRAIN, PLAIN, False),
]


@pytest.mark.parametrize('case', CASES_1D, ids=[c[0] for c in CASES_1D])
def test_block16_1d(case):
  _, B, cin, cout, groups, k, s, p, W, mode, in_mode, out_f32 = case
  _case(1, B, cin, cout, groups, k, s, p, 1, W, mode, in_mode, out_f32)


CASES_2D = [
    # name, B, cin, cout, k, s, p, H, W
    ('ae0', 2, 1, 64, 3, 1, 1, 16, 32),
    ('ae1', 2, 64, 64, 4, 2, 1, 16, 32),
    ('ae2', 2, 64, 128, 3, 1, 1, 8, 16),
    ('ae7', 3, 64, 128, (3, 8), 1, (1, 3), 8, 16),
    ('odd', 2, 16, 32, 4, 2, 1, 10, 14),
]


@pytest.mark.parametrize('case', CASES_2D, ids=[c[0] for c in CASES_2D])
def test_block16_2d(case):
  _, B, cin, cout, k, s, p, H, W = case
  _case(2, B, cin, cout, 1, k, s, p, H, W, BN_TRAIN)


@pytest.mark.parametrize('name,args', [
    ('dec1', (1, 8, 128, 128, 4, 3, 1, 1, 1, 64)), ('unet_pre', (1, 4, 256, 256, 1, 3, 1, 1, 1, 64)),
    ('unet_up2', (1, 4, 64, 64, 1, 3, 1, 1, 1, 16)), ('ae2', (2, 2, 64, 128, 1, 3, 1, 1, 8, 16)), ('big2d', (2, 16, 16, 64, 1, 3, 1, 1, 64, 64))])
def test_block16_bn_backward_reads_y_or_y_raw_per_channel_block(name, args):
  """BN_TRAIN backward takes x_hat and the activation mask from the block's output where BatchNorm + LeakyReLU invert safely and
  from the kept y_raw elsewhere: channels with tiny gamma / dominant beta, and a ReLU block (nothing inverts), in-launch and
  two-launch BatchNorm forms ('big2d': 512 pixel tiles)."""
  nd, B, cin, cout, groups, k, s, p, H, W = args
  in_mode = UP2 if name == 'unet_up2' else PLAIN
  # (the y_raw path takes the activation mask from the ROUNDED conv output: against exact math its gradients carry ~1 % l2 --
  # what every block had before the backward pass read y; hence the wider rail here)
  _case(nd, B, cin, cout, groups, k, s, p, H, W, BN_TRAIN, in_mode, fragile=True, grad_tol=3e-2)
  _case(nd, B, cin, cout, groups, k, s, p, H, W, BN_TRAIN, in_mode, slope=0.0, grad_tol=3e-2)


def test_block16_first_audio_layer_eval_and_lrelu():
  """1 -> 64 channels, 3x3 (AudioEncoder conv.0): eval-mode BatchNorm and plain LeakyReLU run on the vector-unit kernel
  (conv16_c1.hip), train mode on the matrix-pipe kernel; both against exact math on the same 16-bit inputs."""
  _case(2, 2, 1, 64, 1, 3, 1, 1, 16, 32, BN_EVAL)
  _case(2, 3, 1, 64, 1, 3, 1, 1, 10, 12, LRELU)
  _case(2, 2, 1, 64, 1, 3, 1, 1, 16, 32, BN_EVAL, dt=torch.float16, bars='dtype')


def test_block16_fp16_eval():
  _case(1, 4, 64, 64, 1, 3, 1, 1, 1, 64, BN_EVAL, dt=torch.float16, bars='dtype')
  _case(1, 4, 128, 128, 2, 3, 1, 1, 1, 64, LRELU, dt=torch.float16, bars='dtype')


def test_converters_roundtrip():
  from mix_stage_amd import ops16
  from mix_stage_amd._lib import MS_BF16
  x = torch.randn(3, 13, 7, device=DEV)
  c = ops16.to_cb8(x, MS_BF16)
  assert c.shape == (3, 2, 7, 8) and c.dtype == torch.bfloat16
  back = ops16.from_cb8(c, 13)
  assert torch.equal(back, x.bfloat16().float())
  assert float(c[:, 1, :, 5:].abs().max()) == 0.0                   # pad channels are zero
  p = torch.randn(2, 9, 20, device=DEV)                              # (B, T, C)
  v = ops16.btc_to_cb8(p, MS_BF16, velocity=True)
  ref = torch.zeros_like(p); ref[:, 1:] = p[:, 1:] - p[:, :-1]
  got = ops16.from_cb8(v, 20).transpose(1, 2)
  assert torch.equal(got, ref.bfloat16().float())
  p2 = p.clone().requires_grad_()
  w = torch.randn(2, 9, 20, device=DEV)
  (ops16.from_cb8(ops16.btc_to_cb8(p2, MS_BF16, velocity=True), 20).transpose(1, 2) * w).sum().backward()
  wr = w.bfloat16().float()
  exp = torch.zeros_like(p); exp[:, 1:] += wr[:, 1:]; exp[:, :-1] -= wr[:, 1:]
  assert (p2.grad - exp).abs().max().item() <= 1e-6
