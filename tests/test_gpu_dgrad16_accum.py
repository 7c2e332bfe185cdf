"""GPU: ms_bwd_options.dx_accum in the 16-bit modes -- the data-gradient launch of a plain-input block adds a cb8 tensor of dx's
type and shape to its fp32 accumulators before the one rounding to 16 bits (conv16_kernel.h: EP_DGRAD_ACC).  Every case goes
through ms_conv_block_bwd_ex three times on the same saved tensors: without dx_accum, with an all-zero one and with a random O(1)
one.  The operands and the fp64 reference (the block in float64 on the 16-bit-rounded operands) are built as in
tests/test_gpu_kernels16.py."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels16 import BARE, BCAST, BN_TRAIN, DEV, LRELU, PLAIN, UP2, _round

pytestmark = pytest.mark.gpu

# name: (nd, B, cin, cout, groups, k, s, p, H, W, mode) -- shapes tests/test_gpu_kernels16.py runs, so a kernel exists for each
CASES = {
    'unet_down': (1, 4, 64, 64, 1, 4, 2, 1, 1, 64, BN_TRAIN),
    'unet_deep': (1, 6, 64, 64, 1, 4, 2, 1, 1, 4, BN_TRAIN),          # fewer frames than a tile
    'unet_pre': (1, 4, 256, 256, 1, 3, 1, 1, 1, 64, BN_TRAIN),
    'cls0': (1, 4, 266, 256, 1, 3, 1, 1, 1, 64, BN_TRAIN),            # dx has 6 pad channels in its last block
    'dec1': (1, 8, 128, 128, 4, 3, 1, 1, 1, 64, BN_TRAIN),            # grouped
    'd_conv3': (1, 4, 128, 256, 1, 4, 1, 1, 1, 16, BN_TRAIN),
    'd_conv1': (1, 4, 104, 64, 1, 4, 2, 1, 1, 64, LRELU),
    'ae1': (2, 2, 64, 64, 1, 4, 2, 1, 16, 32, BN_TRAIN),
    'ae2': (2, 2, 64, 128, 1, 3, 1, 1, 8, 16, BN_TRAIN),
    'odd': (2, 2, 16, 32, 1, 4, 2, 1, 10, 14, BN_TRAIN),              # ragged in both axes, odd class sizes
}
RUNS = [(n, torch.bfloat16) for n in CASES] + [(n, torch.float16) for n in ('unet_down', 'cls0', 'odd')]
PATTERN = 1.75       # exactly representable in both 16-bit types and in fp32


class _Block:
  """One 16-bit block after its forward pass: the tensors its backward reads, and the fp64 data gradient."""

  def __init__(self, nd, B, cin, cout, groups, k, s, p, H, W, mode, in_mode=PLAIN, dt=torch.bfloat16, seed=0, reference=True):
    from mix_stage_amd import ops, ops16
    from mix_stage_amd._lib import MS_BF16, MS_F16
    msdt = MS_BF16 if dt == torch.bfloat16 else MS_F16
    g = torch.Generator().manual_seed(seed)
    sp = (H, W) if nd == 2 else (W,)
    self.cin_tot = cin_tot = cin if in_mode == BCAST else cin * groups
    kt = (k, k) if nd == 2 else (k,)
    fan = cin
    for v in kt:
      fan *= v
    ctot = cout * groups
    w = (torch.randn((ctot, cin) + kt, generator=g) * fan ** -0.5).to(DEV)
    bias = (torch.randn(ctot, generator=g) * 0.1).to(DEV)
    gamma = (0.5 + torch.rand(ctot, generator=g)).to(DEV)
    beta = (torch.randn(ctot, generator=g) * 0.1).to(DEV)
    rm = (torch.randn(ctot, generator=g) * 0.1).to(DEV)
    rv = (0.5 + torch.rand(ctot, generator=g)).to(DEV)
    x2 = None
    if in_mode == UP2:
      xa = torch.randn((B, cin_tot, W // 2), generator=g).to(DEV)
      xr = torch.randn((B, cin_tot, W), generator=g).to(DEV)
      x, x2 = ops16.to_cb8(xa, msdt), ops16.to_cb8(xr, msdt)
    else:
      xp = torch.randn((B, cin_tot) + sp, generator=g).to(DEV)
      x = ops16.to_cb8(xp, msdt)
    wp = w.clone().requires_grad_()
    bn = mode == BN_TRAIN
    geom = ops.ConvGeom(nd, groups, k, s, p, slope=0.2)
    y = ops16.conv_block16(x, wp, bias, geom, mode, gamma=gamma if bn else None, beta=beta if bn else None,
                           running_mean=rm if bn else None, running_var=rv if bn else None, x2=x2, in_mode=in_mode)
    fn = y.grad_fn
    assert type(fn).__name__ == '_ConvBlock16FnBackward'
    self.desc, self.mode, self.in_mode, self.dt = fn.geom_desc, mode, in_mode, dt
    self.x, self.x2, self.w, self.bias, self.gamma = x, x2, w, bias, (gamma if bn else None)
    _, _, _, _, self.y_raw, self.y, self.save = fn.saved_tensors
    osp = tuple(y.shape[2:-1])
    dyp = torch.randn((B, ctot) + osp, generator=g).to(DEV)
    self.dy = ops16.to_cb8(dyp, msdt)
    self.acc = ops16.to_cb8(torch.randn((B, cin_tot) + sp, generator=g).to(DEV), msdt)      # O(1), pad channels zero
    self.dx64 = None
    if reference:
      # fp64 on the rounded operands the device sees (x, w and dy in 16 bits; bias and the BatchNorm parameters in fp32)
      x64 = _round(xp.cpu(), dt).requires_grad_()
      conv = F.conv2d if nd == 2 else F.conv1d
      raw = conv(x64, _round(w.cpu(), dt), bias.cpu().double(), stride=s, padding=p, groups=groups)
      if mode == BN_TRAIN:
        dims, shape = ((0, 2, 3), (1, -1, 1, 1)) if nd == 2 else ((0, 2), (1, -1, 1))
        mean, var = raw.mean(dims), raw.var(dims, unbiased=False)
        z = (raw - mean.view(shape)) / torch.sqrt(var.view(shape) + 1e-5) * gamma.cpu().double().view(shape) + beta.cpu().double().view(shape)
        ref = F.leaky_relu(z, 0.2)
      elif mode == LRELU:
        ref = F.leaky_relu(raw, 0.2)
      else:
        ref = raw
      (ref * _round(dyp.cpu(), dt)).sum().backward()
      self.dx64 = x64.grad

  def takes_accum(self):
    from mix_stage_amd._lib import lib
    return lib().ms_dgrad_takes_accum(ctypes.byref(self.desc))

  def backward(self, acc=None, want_dx=True):
    """ms_conv_block_bwd_ex on the saved tensors -> (rc, everything the call may write, pre-filled with PATTERN)."""
    from mix_stage_amd import ops
    from mix_stage_amd._lib import BwdOptions, lib
    from mix_stage_amd.ops import _ptr, _stream
    d = self.desc
    new = lambda t: torch.full_like(t, PATTERN)
    out = dict(dx=new(self.x) if want_dx else None, dx2=new(self.x2) if (want_dx and self.x2 is not None) else None,
               dyr=new(self.dy) if self.mode != BARE else None, dw=new(self.w),
               dbias=new(self.bias),
               dgamma=new(self.gamma) if self.gamma is not None else None, dbeta=new(self.gamma) if self.gamma is not None else None)
    ws = ops.workspace(d._bwd_ws, self.x.device)
    opt = BwdOptions()
    if acc is not None:
      opt.dx_accum = acc.data_ptr()
    rc = lib().ms_conv_block_bwd_ex(ctypes.byref(d), _ptr(self.x), _ptr(self.x2), _ptr(self.w), _ptr(self.gamma), None, None,
                                    _ptr(self.y_raw), _ptr(self.y), _ptr(self.save), _ptr(self.dy), _ptr(out['dyr']), _ptr(out['dx']),
                                    _ptr(out['dx2']), _ptr(out['dw']), _ptr(out['dbias']), _ptr(out['dgamma']), _ptr(out['dbeta']),
                                    _ptr(ws), ws.numel(), _stream(), ctypes.byref(opt))
    torch.cuda.synchronize()
    return rc, out


def _same_bits(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize('name,dt', RUNS, ids=['%s-%s' % (n, 'bf16' if t == torch.bfloat16 else 'fp16') for n, t in RUNS])
def test_dgrad16_adds_dx_accum_before_the_one_rounding(name, dt):
  """(a) a zero dx_accum changes no bit of dx; dw, dyr and the BatchNorm gradients never change.  (b) element-wise, the fused
  F = round(A + acc) is within the three half-ulps 1.01 u (|plain| + |F| + |P|) + tiny of the two-step P = round(round(A) + acc),
  A the launch's fp32 accumulator: both round the same A, F once, P twice (u = 2^-8 bf16, 2^-11 fp16; tiny: fp16 subnormals).  acc is
  O(1), so a misaddressed pixel, channel block or parity class breaks it.  (c) against fp64 (the block's data gradient from the
  rounded operands, plus acc), F's l2 error is at most 1.02 x P's.  (d) pad channels of dx stay zero, acc is not written."""
  blk = _Block(*CASES[name], dt=dt)
  assert blk.takes_accum() == 1
  acc = blk.acc
  acc_before = acc.clone()
  rc0, plain = blk.backward()
  rcz, zero = blk.backward(torch.zeros_like(acc))
  rcf, fused = blk.backward(acc)
  assert rc0 == 0 and rcz == 0 and rcf == 0
  # (a)
  assert _same_bits(zero['dx'], plain['dx'])
  for k in ('dw', 'dyr', 'dbias', 'dgamma', 'dbeta'):
    if plain[k] is not None:
      assert _same_bits(zero[k], plain[k]) and _same_bits(fused[k], plain[k]), k
  # (b)
  u, tiny = (2.0 ** -8, 2.0 ** -133) if dt == torch.bfloat16 else (2.0 ** -11, 2.0 ** -24)
  Pt = plain['dx'] + acc                                   # torch's 16-bit add: the two-step form
  pl, Fv, Pv = plain['dx'].double(), fused['dx'].double(), Pt.double()
  excess = ((Fv - Pv).abs() - (1.01 * u * (pl.abs() + Fv.abs() + Pv.abs()) + tiny)).max().item()
  differ = (Fv != Pv).float().mean().item()
  # (c)
  def plain_layout(t):                                     # cb8 (B, C8, ..., 8) -> (B, C, ...)
    t = t.movedim(-1, 2)
    return t.reshape((t.shape[0], -1) + tuple(t.shape[3:]))[:, :blk.cin_tot].cpu()
  ref = blk.dx64 + plain_layout(acc.double())
  eF = (plain_layout(Fv) - ref).norm().item() / ref.norm().item()
  eP = (plain_layout(Pv) - ref).norm().item() / ref.norm().item()
  print('%s %s: (b) worst excess over the bound %.3e, F != P in %.1f %% of the elements; (c) l2 error fused %.4e two-step %.4e ratio %.4f'
        % (name, dt, excess, 100 * differ, eF, eP, eF / eP))
  assert excess <= 0.0, excess
  assert eF <= 1.02 * eP, (eF, eP)
  # (d)
  valid = blk.cin_tot % 8
  if valid:
    assert float(fused['dx'][:, -1, ..., valid:].abs().max()) == 0.0
  else:
    assert name != 'cls0'
  assert _same_bits(acc, acc_before)


@pytest.mark.parametrize('what', ['up2', 'bcast', 'dx_null'])
def test_dx_accum_is_refused_where_the_launch_cannot_take_it(what):
  """dx_accum on an upsample-add block, on a broadcast-input block, or without dx: an error, and nothing is launched or written."""
  if what == 'up2':
    blk = _Block(1, 4, 64, 64, 1, 3, 1, 1, 1, 16, BN_TRAIN, in_mode=UP2, reference=False)
  elif what == 'bcast':
    blk = _Block(1, 8, 74, 128, 4, 3, 1, 1, 1, 64, BN_TRAIN, in_mode=BCAST, reference=False)
  else:
    blk = _Block(*CASES['unet_down'], reference=False)
  assert blk.takes_accum() == (1 if what == 'dx_null' else 0)
  acc = torch.zeros_like(blk.x2 if what == 'up2' else blk.x)
  rc, out = blk.backward(acc, want_dx=what != 'dx_null')
  assert rc != 0
  for k, t in out.items():
    if t is not None:
      assert bool((t == PATTERN).all()), k
  # ... and the same call without dx_accum runs
  rc, out = blk.backward(None, want_dx=what != 'dx_null')
  assert rc == 0 and not bool((out['dw'] == PATTERN).all())
