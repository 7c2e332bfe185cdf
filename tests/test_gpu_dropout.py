"""GPU: dropout inside the ConvNormRelu block (p > 0 in training mode): conv (+bias) -> dropout(p) -> BatchNorm -> (Leaky)ReLU with
the mask regenerated inside the BatchNorm passes (csrc/dropout.hip, include/mixstage.h: ms_dropout_bn_fwd ...).

  * ms_dropout_mask against the Python mirror (tests/helpers/philox_ref.py), bit for bit;
  * the block, forward and backward, against float64: F.conv* -> * mask / (1 - p) -> F.batch_norm(training=True) -> leaky_relu
    under autograd on the CPU, the mask from the mirror -- and, frozen (layers.freeze_batchnorm), against batch_norm(training=False).
    Bars: those of the batch-statistics block (test_gpu_frozen_bn.py, test_gpu_kernels._conv_block_case): forward 2e-5, gradients
    1e-4, of the tensor's max-abs, element-wise.  The shapes sit at the edges of the one-launch kernels (DROPOUT_FUSED_MAX = 4096
    values per channel; the NE = 4 / 8 / 16 instances change at 1024 and 2048);
  * the 16-bit modes to the bars test_gpu_frozen_bn.py holds its 16-bit cases to; a few cases under bf16x6;
  * eval mode and p = 0 launch what they always launched; the trainer draws fresh masks every step, eager and captured alike.

Every test but the p = 0 label list and the eval twin fails without the feature: the block raised NotImplementedError."""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import philox_ref as R
from oracle import mixstage_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FWD_BAR, GRAD_BAR = 2e-5, 1e-4
SEED = 0x5678_0000_1234          # the default state's seed in these tests: words (0x1234, 0x5678)
MOD_ID = 5                       # the module id the stand-alone blocks are given


def _state(seed=SEED, step=0):
  from mix_stage_amd import ops
  return ops.dropout_state_words(seed, step).to(DEV)


def _ref_mask(shape, p, site, step=0, seed=SEED, channelwise=False):
  return torch.from_numpy(R.mask_like(shape, p, R.seed_words(seed), site, step, channelwise))


# ---- the mask --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,channelwise,p', [((2, 5, 7), False, 0.25), ((3, 64, 64), False, 0.1), ((2, 5, 3, 7), True, 0.5),
                                                 ((2, 4, 64, 33), True, 0.25)], ids=['2x5x7', '3x64x64', 'cw_2x5x3x7', 'cw_2x4x64x33'])
def test_mask_equals_the_python_reference_bit_for_bit(shape, channelwise, p):
  from mix_stage_amd import ops
  for site, step, seed in ((7, 0, SEED), (R.site_of(52, 3), 9, 0xffffffff_deadbeef)):
    got = ops.dropout_mask(shape, p, site, _state(seed, step), channelwise=channelwise).cpu()
    exp = _ref_mask(shape, p, site, step, seed, channelwise)
    assert got.dtype == torch.float32 and torch.equal(got, exp), (shape, site, step)
    assert 0 < int((got != 0).sum()) < got.numel()


# ---- one block against float64 ----------------------------------------------------------------------------------------------------------
def errs_of(a, b):
  a, b = a.detach().double().cpu(), b.detach().double().cpu()
  assert a.shape == b.shape, (a.shape, b.shape)
  return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


# (name, nd, cin, cout, kernel, stride, groups, input spatial, B, in_mode, leaky, p) -- cin / cout per group.
# Output (B, C, HW) and the form it takes, from ms_dropout_bn_fwd / _bwd: n = B * HW <= 1024: <4>, <= 2048: <8>, <= 4096: <16>, else two passes
CASES = [
    ('hw1', 1, 4, 3, 4, 2, 1, (2,), 2, 'plain', True, 0.25),                  # (2, 3, 1): k4 s2, one value per clip and channel
    ('b2c5t7', 1, 3, 5, 3, 1, 1, (7,), 2, 'plain', True, 0.25),               # (2, 5, 7): rows that are no multiple of 4
    ('n1024', 1, 8, 8, 3, 1, 1, (256,), 4, 'plain', True, 0.1),               # (4, 8, 256): the last size of <4>
    ('n1028_k4s2', 1, 8, 8, 4, 2, 1, (514,), 4, 'plain', True, 0.1),          # (4, 8, 257): the first of <8>
    ('n4096_g2', 1, 4, 4, 3, 1, 2, (128,), 32, 'plain', True, 0.5),           # (32, 8, 128): grouped; the last size of <16>
    ('n4098', 1, 8, 8, 3, 1, 1, (2049,), 2, 'plain', True, 0.1),              # (2, 8, 2049): two passes
    ('odd_relu', 1, 5, 7, 3, 1, 1, (683,), 3, 'plain', False, 0.25),          # (3, 7, 683): n = 2049, <16>; ReLU (slope 0)
    ('up2add', 1, 8, 8, 3, 1, 1, (8,), 2, 'up2', True, 0.25),
    ('bcast_g2', 1, 10, 33, 3, 1, 2, (19,), 3, 'bcast', True, 0.1),
    ('2d_3x3', 2, 4, 5, 3, 1, 1, (6, 7), 6, 'plain', True, 0.25),             # channel dropout: (6, 5, 6, 7)
    ('2d_4x4s2', 2, 8, 8, 4, 2, 1, (64, 66), 4, 'plain', True, 0.25),         # channel dropout, (4, 8, 32, 33): n = 4224, two passes
]
IDS = [c[0] for c in CASES]
EXPECT = {'hw1': '<4>', 'b2c5t7': '<4>', 'n1024': '<4>', 'n1028_k4s2': '<8>', 'n4096_g2': '<16>', 'n4098': None, 'odd_relu': '<16>',
          'up2add': '<4>', 'bcast_g2': '<4>', '2d_3x3': '<4>', '2d_4x4s2': None}


def _mk(case, seed, p=None):
  import mix_stage_amd as A
  name, nd, cin, cout, k, s, g, sp, B, in_mode, leaky, p_case = case
  blk = A.ConvNormRelu(cin, cout, type='%dd' % nd, leaky=leaky, kernel_size=k, stride=s, groups=g, p=p_case if p is None else p)
  sd = O.deterministic_state({'dr%d.' % seed + kk: v for kk, v in blk.state_dict().items()})
  blk.load_state_dict({kk.split('.', 1)[1]: v for kk, v in sd.items()})
  gen = torch.Generator().manual_seed(1000 + seed)
  C = cout * g
  with torch.no_grad():
    blk.norm.running_mean.copy_(0.3 * torch.randn(C, generator=gen))
    blk.norm.running_var.copy_(0.25 + torch.rand(C, generator=gen))
    blk.norm.weight.copy_(0.5 + torch.rand(C, generator=gen))
    blk.norm.bias.copy_(0.2 * torch.randn(C, generator=gen))
    blk.norm.num_batches_tracked.fill_(7)
  blk._drop_id = MOD_ID
  return blk.to(DEV).train()


def _inputs(case, gen, B):
  name, nd, cin, cout, k, s, g, sp, _, in_mode, leaky, p = case
  if in_mode == 'up2':
    return [torch.randn(B, cin * g, sp[0] // 2, generator=gen), torch.randn(B, cin * g, sp[0], generator=gen)]
  return [torch.randn(B, cin if in_mode == 'bcast' else cin * g, *sp, generator=gen)]


def _run_hip(blk, case, xs, cast=None):
  in_mode = case[9]
  leaves = [x.to(DEV).requires_grad_() for x in xs]
  ins = leaves if cast is None else [cast(t) for t in leaves]
  if in_mode == 'up2':
    y = blk.forward_upsample_add(*ins)
  else:
    y = blk.forward_broadcast(ins[0]) if in_mode == 'bcast' else blk(ins[0])
  return y, leaves


def _run_ref(blk, case, xs, site, frozen, step=0, round_to=None, stats=None):
  """float64: conv -> * mask / (1 - p) -> batch_norm -> leaky_relu.  round_to: the 16-bit dtype the operands are rounded to first."""
  name, nd, cin, cout, k, s, g, sp, _, in_mode, leaky, p = case
  rd = (lambda t: t.to(round_to).double()) if round_to is not None else (lambda t: t.double())
  leaves = [rd(x).requires_grad_() for x in xs]
  if in_mode == 'up2':
    xin = F.interpolate(leaves[0], scale_factor=2, mode='nearest') + leaves[1]
    if round_to is not None:
      xin = xin + (rd(xin.detach().float()) - xin.detach())          # (the kernel adds in fp32 and rounds the sum once)
  else:
    xin = torch.cat([leaves[0]] * g, dim=1) if in_mode == 'bcast' else leaves[0]
  ps = {'w': rd(blk.conv.weight.detach().cpu()).requires_grad_()}
  for n, t in (('bias', blk.conv.bias), ('gamma', blk.norm.weight), ('beta', blk.norm.bias)):
    ps[n] = t.detach().double().cpu().requires_grad_()
  conv = F.conv1d if nd == 1 else F.conv2d
  raw = conv(xin, ps['w'], ps['bias'], stride=blk.conv.stride, padding=blk.conv.padding, groups=g)
  mask = _ref_mask(tuple(raw.shape), blk._p, site, step, channelwise=nd == 2).double()
  rm, rv = stats if stats is not None else (blk.norm.running_mean, blk.norm.running_var)      # (as they are BEFORE the device pass)
  rm, rv = rm.detach().double().cpu().clone(), rv.detach().double().cpu().clone()
  z = F.batch_norm(raw * mask, rm, rv, ps['gamma'], ps['beta'], training=not frozen, momentum=blk.norm.momentum, eps=blk.norm.eps)
  return F.leaky_relu(z, 0.2 if leaky else 0.0), leaves, ps, (rm, rv), mask


def _labels_of(fn):
  from mix_stage_amd import ops
  ops.timing_enable(True)
  try:
    out = fn()
    torch.cuda.synchronize()
    return out, [r['label'].split('|')[-1] for r in ops.timing_report() for _ in range(r['count'])]
  finally:
    ops.timing_enable(False)


def _check_labels(labels, frozen, expect):
  fwd = [l for l in labels if l.startswith(('bn_finalize', 'bn_apply'))]
  bwd = [l for l in labels if l.startswith('bn_bwd')]
  assert len(fwd) == 1 and len(bwd) == 1 and fwd[0].endswith(' dropout') and bwd[0].endswith(' dropout'), labels
  assert (' frozen' in fwd[0]) == (' frozen' in bwd[0]) == frozen, labels
  assert fwd[0].startswith('bn_apply' if frozen else 'bn_finalize_apply'), labels
  if expect is None:
    assert bwd[0].startswith('bn_bwd(reduce+apply)') and ('chunks' in fwd[0]), labels
  else:
    assert bwd[0].startswith('bn_bwd_fused' + expect) and expect in fwd[0], labels
  # the conv ran as the block's BARE launch (no statistics in it), data and weight gradients as ever
  conv_l = [l for l in labels if 'conv_fwd' in l]
  assert conv_l and all('+bn' not in l and (' ep' not in l or l.endswith(' ep0')) for l in conv_l), labels
  assert not any('bnstats' in l or 'bnfused' in l for l in labels), labels
  assert any('dgrad' in l for l in labels) and any('wgrad' in l for l in labels), labels


def _case(case, seed, frozen, expect='unset', check_labels=True):
  """-> False where a pre-activation sits within fp32 rounding of the LeakyReLU kink (the caller draws again)."""
  import mix_stage_amd as A
  from mix_stage_amd import layers
  A.manual_dropout_seed(SEED)
  B = case[8]
  blk = _mk(case, seed)
  if frozen:
    assert layers.freeze_batchnorm(blk) == 1
  buf0 = [blk.norm.running_mean.clone(), blk.norm.running_var.clone()]
  gen = torch.Generator().manual_seed(seed)
  xs = _inputs(case, gen, B)
  y_ref, leaves_ref, ps, (rm_ref, rv_ref), mask = _run_ref(blk, case, xs, R.site_of(MOD_ID, 0), frozen)
  assert mask.numel() < 64 or 0 < int((mask != 0).sum()) < mask.numel()
  gy = torch.randn(y_ref.shape, generator=gen)

  def step():
    y, leaves = _run_hip(blk, case, xs)
    y.backward(gy.to(DEV))
    return y, leaves
  (y, leaves), labels = _labels_of(step)
  figs = {'fwd': (errs_of(y, y_ref), FWD_BAR)}
  if ((y.detach().cpu() > 0) != (y_ref.detach() > 0)).any():
    assert figs['fwd'][0] < FWD_BAR, figs
    return False
  y_ref.backward(gy.double())
  for i, (a, b) in enumerate(zip(leaves, leaves_ref)):
    figs['dx%d' % i] = (errs_of(a.grad, b.grad), GRAD_BAR)
  for n, t in (('w', blk.conv.weight), ('bias', blk.conv.bias), ('gamma', blk.norm.weight), ('beta', blk.norm.bias)):
    figs['d' + n] = (errs_of(t.grad, ps[n].grad), GRAD_BAR)
  print(case[0], 'frozen' if frozen else 'batch', {k: '%.2e' % v[0] for k, v in figs.items()})
  bad = {k: v for k, v in figs.items() if not v[0] < v[1]}
  assert not bad, 'errors (max-abs / max-abs of the reference, bar): %s | all: %s' % (bad, figs)
  sd = blk.state_dict()
  if frozen:
    # the statistics are read, never written: bit for bit; no tracked batch
    assert torch.equal(blk.norm.running_mean, buf0[0]) and torch.equal(blk.norm.running_var, buf0[1])
    assert int(sd['norm.num_batches_tracked']) == 7
  else:
    assert errs_of(blk.norm.running_mean, rm_ref) < FWD_BAR and errs_of(blk.norm.running_var, rv_ref) < FWD_BAR
    assert not torch.equal(blk.norm.running_mean, buf0[0]) and int(sd['norm.num_batches_tracked']) == 8
  if check_labels:
    _check_labels(labels, frozen, EXPECT[case[0]] if expect == 'unset' else expect)
  # the next pass of the same block draws another mask (visit 1) -- and equals the reference for THAT site
  with torch.no_grad():
    y2, _ = _run_hip(blk, case, xs)
  assert blk._drop_visit == 2
  if not frozen:
    return True              # (a batch-statistics block has moved its running statistics: its second pass is checked frozen)
  y2_ref = _run_ref(blk, case, xs, R.site_of(MOD_ID, 1), True)[0]
  assert not torch.equal(y2, y.detach())
  flips = (y2.cpu() > 0) != (y2_ref.detach() > 0)
  assert errs_of(torch.where(flips, torch.zeros_like(y2.cpu()), y2.cpu()), torch.where(flips, torch.zeros_like(y2_ref), y2_ref.detach())) < FWD_BAR
  return True


def _draws(case, frozen, **kw):
  for attempt in range(4):
    if _case(case, zlib.crc32(case[0].encode()) % 1000 + attempt, frozen, **kw):
      return
  raise AssertionError('no draw without a sign flip at a LeakyReLU kink')


@pytest.mark.parametrize('frozen', [False, True], ids=['batch', 'frozen'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_dropout_block_fwd_bwd_vs_fp64(case, frozen):
  _draws(case, frozen)


@pytest.mark.parametrize('frozen', [False, True], ids=['batch', 'frozen'])
@pytest.mark.parametrize('case', [c for c in CASES if c[0] in ('n1024', 'up2add', '2d_3x3')], ids=lambda c: c[0])
def test_dropout_block_bf16x6(case, frozen):
  from mix_stage_amd import _lib
  old = _lib.lib().ms_set_precision(1)
  try:
    _draws(case, frozen, check_labels=False)
  finally:
    _lib.lib().ms_set_precision(old)


def test_two_runs_same_bits_and_affine_off():
  """Fixed-order reductions: the same state, site and inputs give the same bits; gamma / beta without requires_grad get no gradient
  and leave every other result as it was."""
  import mix_stage_amd as A
  for case in (CASES[2], CASES[5], CASES[10]):
    xs = _inputs(case, torch.Generator().manual_seed(5), case[8])
    out = []
    for affine in (True, True, False):
      A.manual_dropout_seed(SEED)
      blk = _mk(case, 5)
      blk.norm.weight.requires_grad_(affine)
      blk.norm.bias.requires_grad_(affine)
      y, leaves = _run_hip(blk, case, xs)
      gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6))
      y.backward(gy.to(DEV))
      assert (blk.norm.weight.grad is None) == (not affine)
      out.append((y.detach(), leaves[0].grad, blk.conv.weight.grad, blk.conv.bias.grad, blk.norm.running_mean.clone(), blk.norm.running_var.clone()))
    for a, b, c in zip(*out):
      assert torch.equal(a, b) and torch.equal(a, c)


def test_double_model_passes_the_boundary_casts():
  import mix_stage_amd as A
  A.manual_dropout_seed(SEED)
  case = CASES[1]
  blk = _mk(case, 3).double()
  xs = _inputs(case, torch.Generator().manual_seed(3), case[8])
  y_ref, leaves_ref, ps, (rm_ref, rv_ref), _ = _run_ref(blk, case, xs, R.site_of(MOD_ID, 0), False)
  x = xs[0].double().to(DEV).requires_grad_()
  y = blk(x)
  assert y.dtype == torch.float64 and blk.norm.running_mean.dtype == torch.float64
  gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
  y.backward(gy.double().to(DEV))
  y_ref.backward(gy.double())
  assert errs_of(y, y_ref) < FWD_BAR and errs_of(x.grad, leaves_ref[0].grad) < GRAD_BAR and x.grad.dtype == torch.float64
  assert errs_of(blk.norm.weight.grad, ps['gamma'].grad) < GRAD_BAR and errs_of(blk.conv.weight.grad, ps['w'].grad) < GRAD_BAR
  assert errs_of(blk.norm.running_mean, rm_ref) < FWD_BAR and errs_of(blk.norm.running_var, rv_ref) < FWD_BAR


# ---- 16-bit modes -------------------------------------------------------------------------------------------------------------------------
# Bars: those test_gpu_frozen_bn.py holds its 16-bit cases to (test_gpu_kernels16._case with bars='dtype' on the BN_TRAIN block of the
# same geometry) -- bf16: forward 1.2e-2, gradients 2 x 2e-2 on the max (+ the 1e-6 floor) and 2e-2 in l2; fp16: the smaller of those / 8
# and MODEL_K x the error helpers/round16_model.py emulates for the BN_TRAIN block in its two-launch form on this case's tensors.  The
# reference is float64 on the 16-bit-rounded operands with the mirror's mask.
# (name, nd, B, cin, cout, groups, k, s, pad, H, W, in_mode, p)
CASES16 = [
    ('k3', 1, 4, 64, 64, 1, 3, 1, 1, 1, 64, 0, 0.1),
    ('k4s2', 1, 4, 64, 64, 1, 4, 2, 1, 1, 64, 0, 0.25),
    ('up2add', 1, 4, 64, 64, 1, 3, 1, 1, 1, 16, 2, 0.25),
    ('2d', 2, 4, 16, 32, 1, 3, 1, 1, 8, 16, 0, 0.25),               # channel dropout
    ('two_pass', 1, 5, 16, 16, 1, 3, 1, 1, 1, 1000, 0, 0.1),        # n = 5000 > 4096: the two-pass kernels
]


@pytest.mark.parametrize('frozen', [False, True], ids=['batch', 'frozen'])
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('case', CASES16, ids=[c[0] for c in CASES16])
def test_dropout_block16_fwd_bwd_vs_fp64(case, dt, frozen):
  import mix_stage_amd as A
  from helpers import round16_model as M16
  from mix_stage_amd import layers, ops16
  from mix_stage_amd._lib import MS_BF16, MS_BN_TRAIN, MS_F16
  from test_gpu_kernels16 import dtype_bar
  name, nd, B, cin, cout, groups, k, s, pad, H, W, in_mode, p = case
  msdt = MS_BF16 if dt == torch.bfloat16 else MS_F16
  slope = 0.2
  A.manual_dropout_seed(SEED)
  opnd = M16.gen_operands(nd, B, cin, cout, groups, k, s, pad, H, W, in_mode, 3, False)
  blk = A.ConvNormRelu(cin, cout, type='%dd' % nd, leaky=True, kernel_size=k, stride=s, padding=pad, groups=groups, p=p)
  with torch.no_grad():
    blk.conv.weight.copy_(opnd['w']); blk.conv.bias.copy_(opnd['bias'])
    blk.norm.weight.copy_(opnd['gamma']); blk.norm.bias.copy_(opnd['beta'])
    blk.norm.running_mean.copy_(opnd['rm']); blk.norm.running_var.copy_(opnd['rv'])
  blk = blk.to(DEV).train()
  blk._drop_id = MOD_ID
  layers.set_compute_dtype(blk, 'bf16' if dt == torch.bfloat16 else 'fp16')
  if frozen:
    layers.freeze_batchnorm(blk)
  rm0, rv0 = blk.norm.running_mean.clone(), blk.norm.running_var.clone()
  tcase = (name, nd, cin, cout, k, s, groups, (H, W) if nd == 2 else (W,), B, 'up2' if in_mode == 2 else 'plain', True, p)
  xs = [opnd['a'], opnd['r']] if in_mode == 2 else [opnd['x']]
  C = cout * groups

  def step():
    y_, leaves_ = _run_hip(blk, tcase, xs, cast=lambda t: ops16.to_cb8(t, msdt))
    y32_ = ops16.from_cb8(y_, C)
    dy_ = M16.gen_dy(opnd, y32_.shape, 1.0)
    (y32_ * dy_.to(DEV)).sum().backward()
    return y32_, dy_, leaves_
  (y32, dy_cpu, leaves), labels = _labels_of(step)
  fwd_l = [l for l in labels if l.startswith(('bn_finalize', 'bn_apply')) and not l.startswith('bn_apply16')]
  assert len(fwd_l) == 1 and fwd_l[0].endswith(' dropout') and sum(1 for l in labels if l.startswith('bn_bwd') and l.endswith(' dropout')) == 1, labels
  assert ('chunks' in fwd_l[0]) == (name == 'two_pass'), labels
  y_ref, leaves_ref, ps, (rm_ref, rv_ref), _ = _run_ref(blk, tcase, xs, R.site_of(MOD_ID, 0), frozen, round_to=dt, stats=(rm0, rv0))
  # a pre-activation within rounding of 0 follows the device's mask, as in every 16-bit block test
  pos = y32.detach().cpu() > 0
  flip = pos != (y_ref.detach() > 0)
  assert flip.sum().item() <= 2e-3 * flip.numel()
  z = torch.where(y_ref > 0, y_ref, y_ref / slope)
  ref = torch.where(pos, z, slope * z)
  (ref * dy_cpu.to(dt).double()).sum().backward()
  model = None
  if dt == torch.float16:
    model = M16.block_model(opnd, dy_cpu, nd, groups, s, pad, MS_BN_TRAIN, in_mode, slope, False, dt, 1.0, 'cpu', True, 'device', False)
  bar16 = lambda legacy, what: dtype_bar(legacy, model[what]) if model is not None else legacy
  figs = {}
  sc = ref.abs().max().item() + 1e-6
  figs['fwd'] = ((y32.detach().cpu().double() - ref.detach()).abs().max().item() / sc, bar16(1.2e-2, 'fwd'))

  def close(a_, b_, what, tol=2e-2):
    scb = b_.abs().max().item() + 1e-9
    a_ = a_.detach().cpu().double()
    figs[what] = ((a_ - b_).abs().max().item() / scb, bar16(2 * tol, what) + 1e-6 / scb)
    figs[what + ' l2'] = ((a_ - b_).norm().item() / (b_.norm().item() + 1e-12), bar16(tol, what + ' l2'))
  close(blk.conv.weight.grad, ps['w'].grad, 'dw')
  close(blk.norm.weight.grad, ps['gamma'].grad, 'dgamma')
  close(blk.norm.bias.grad, ps['beta'].grad, 'dbeta')
  if in_mode == 2:
    close(leaves[1].grad, leaves_ref[1].grad, 'dx2')
    close(leaves[0].grad, leaves_ref[0].grad, 'dx')
  else:
    close(leaves[0].grad, leaves_ref[0].grad, 'dx')
  scb = ps['bias'].grad.abs().max().item() + 1e-9
  figs['dbias'] = ((blk.conv.bias.grad.cpu().double() - ps['bias'].grad).abs().max().item() / scb, figs['dbeta'][1])
  print(name, dt, 'frozen' if frozen else 'batch', {k_: '%.2e (bar %.2e)' % v for k_, v in figs.items()})
  bad = {k_: v for k_, v in figs.items() if not v[0] <= v[1]}
  assert not bad, bad
  if frozen:
    assert torch.equal(blk.norm.running_mean, rm0) and torch.equal(blk.norm.running_var, rv0) and blk._pending_batches == 0
  else:
    assert errs_of(blk.norm.running_mean, rm_ref) < 1.2e-2 and errs_of(blk.norm.running_var, rv_ref) < 1.2e-2 and blk._pending_batches == 1


# ---- what does not change -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in CASES if c[0] in ('n1024', 'up2add', '2d_4x4s2')], ids=lambda c: c[0])
def test_eval_mode_is_bit_identical_to_the_p0_twin(case):
  xs = _inputs(case, torch.Generator().manual_seed(8), case[8])
  drop, twin = _mk(case, 8).eval(), _mk(case, 8, p=0).eval()
  with torch.no_grad():
    (y_d, _), lab_d = _labels_of(lambda: _run_hip(drop, case, xs))
    (y_t, _), lab_t = _labels_of(lambda: _run_hip(twin, case, xs))
  assert torch.equal(y_d, y_t) and lab_d == lab_t and not any('dropout' in l for l in lab_d), (lab_d, lab_t)
  assert drop._drop_visit == 0 and drop._pending_batches == 0


def _build_gan(p, M=8, S=8, T=64, P=104):
  import mix_stage_amd as A
  G = A.JointLateClusterSoftStyle4_G(time_steps=T, out_feats=P, num_clusters=M, style_dict={i: i for i in range(S)},
                                     style_dim=10, lambda_id=0.1, argmax=1, some_grad_flag=1, train_only=1, shape={}, p=p)
  D = A.Speech2Gesture_D(in_channels=P, p=p)
  model = A.GAN(G, D, criterion='L1Loss', input_modalities=['audio/log_mel_400'], update_D_prob_flag=0, no_grad=0)
  model.load_state_dict(O.deterministic_state(model.state_dict()))
  model.G.thresh.value, model.G.thresh.iters = 1, 10 ** 9
  return model.to(DEV)


B = 4


def _trainer_run(p, use_graphs, kinds, batches, dropout_seed=11, start=None, record_labels=False, **kw):
  from mix_stage_amd.train_step import MixStageTrainStep
  torch.manual_seed(99)
  model = _build_gan(p)
  ts = MixStageTrainStep(model, use_graphs=use_graphs, dropout_seed=dropout_seed, **kw)
  if start is not None:
    start(model, ts)
  losses, labels = [], []
  for (audio, pose, labels_in, style), k in zip(batches, kinds):
    fn = lambda: ts.step(audio.to(DEV), labels_in.to(DEV), pose.to(DEV), style.to(DEV), kind=k)
    if record_labels:
      labels.append(_labels_of(fn)[1])
    else:
      fn()
    losses.append([float(l) for l in ts.losses])
  return losses, {k: v.clone() for k, v in model.state_dict().items()}, model, ts, labels


def test_p0_model_launches_nothing_new():
  """The label list of a G-step and a D-step of a p = 0 model: no ` dropout` launch, no `advance`; the trainer holds no state."""
  batches = [O.synthetic_batch(B, M=8, S=8, seed=60 + i) for i in range(2)]
  losses, _, model, ts, labels = _trainer_run(0, False, ['G', 'D'], batches, record_labels=True)
  assert ts.dropout_state() is None and ts._dropout_state is None
  for step_labels in labels:
    assert len(step_labels) > 50
    for l in step_labels:
      assert 'dropout' not in l and 'advance' not in l, l
  with pytest.raises(RuntimeError):
    ts.set_dropout_state(dict(seed=1, step=0))


def test_generator_size_model_runs_and_draws_fresh_masks():
  """JointLateClusterSoftStyle4_G(p=0.1) + Speech2Gesture_D(p=0.1) at the golden size (B = 4, T = 64, M = S = 8): a G-step and a
  D-step run, every p > 0 block launches its dropout passes (D twice in the D-step, on two sites), the step leads with `advance`,
  and the fused forms stand aside."""
  from mix_stage_amd import layers
  batches = [O.synthetic_batch(B, M=8, S=8, seed=60 + i) for i in range(2)]
  losses, sd, model, ts, labels = _trainer_run(0.1, False, ['G', 'D'], batches, record_labels=True)
  assert all(np.isfinite(v) for row in losses for v in row)
  drop = layers.dropout_blocks(model)
  d_blocks = [b for b in drop if any(b is m for m in model.D.modules())]
  assert len(drop) > 40 and len(d_blocks) == 2
  for k, step_labels in zip('GD', labels):
    # (G-step: the chained decoder stands aside; D-step: G runs in eval mode -- its usual launches -- and D's paired pass stands aside)
    step_labels = [l for l in step_labels if k == 'G' or not l.startswith(('chain', 'decoder_chain'))]
    assert sum(1 for l in step_labels if l == 'bn_finalize advance dropout') == 1 == sum(1 for l in step_labels if 'advance' in l), step_labels[:3]
    assert not any(l.startswith(('chain', 'decoder_chain')) or ' pair' in l for l in step_labels), [l for l in step_labels if 'chain' in l or ' pair' in l]
  fwd = [l for l in labels[0] if l.startswith('bn_finalize_apply') and l.endswith(' dropout')]
  bwd = [l for l in labels[0] if l.startswith('bn_bwd') and l.endswith(' dropout')]
  assert len(fwd) >= len(bwd) > 30
  # D-step: D runs on the fake and on the real poses -- visits 0 and 1 of its two blocks
  assert all(b._drop_visit == 2 for b in d_blocks)
  assert ts.dropout_state() == dict(seed=11, step=2)
  assert [b._drop_id for b in model.modules() if isinstance(b, layers.ConvNormRelu)] == list(range(len([b for b in model.modules() if isinstance(b, layers.ConvNormRelu)])))


def test_trainer_eager_equals_captured_and_resumes():
  """4 steps eager == 4 steps captured, bit for bit (losses, parameters, buffers), over two rounds of capture and replay; the state
  counts the steps; set_dropout_state reproduces the run from step 2."""
  kinds = ['G', 'D', 'G', 'D']
  batches = [O.synthetic_batch(B, M=8, S=8, seed=60 + i) for i in range(4)]
  eager = _trainer_run(0.1, False, kinds, batches)
  graph = _trainer_run(0.1, True, kinds, batches)
  assert eager[0] == graph[0]
  for k, v in eager[1].items():
    assert torch.equal(v, graph[1][k]), k
  assert eager[3].dropout_state() == graph[3].dropout_state() == dict(seed=11, step=4)
  assert len(graph[3]._graphs) == 2                             # (steps 3 and 4 replayed what steps 1 and 2 captured)
  # another seed: other masks from the first step on
  other = _trainer_run(0.1, False, kinds[:1], batches[:1], dropout_seed=12)
  assert other[0][0] != eager[0][0]
  # resume: the state after step 2 of the eager run, written into a fresh trainer whose model holds that run's weights and moments
  half = _trainer_run(0.1, False, kinds[:2], batches[:2])
  st, opt_state, weights, sched = half[3].dropout_state(), half[3].optimizer_state(), half[1], half[2].lambda_scheduler.state()
  assert st == dict(seed=11, step=2)

  def start(model, ts):
    model.load_state_dict(weights)
    model.lambda_scheduler.set_state(sched)
    ts.set_optimizer_state(opt_state)
    ts.set_dropout_state(st)
  resumed = _trainer_run(0.1, False, kinds[2:], batches[2:], dropout_seed=777, start=start)
  assert resumed[0] == eager[0][2:]
  assert resumed[3].dropout_state() == dict(seed=11, step=4)


def test_replays_draw_the_reference_mask_of_their_step():
  """One captured D-step replayed three times: the discriminator's first block sees, at replay k, exactly the mask the mirror gives
  for (its module id, visit, step k) -- read back through ms_dropout_mask on the trainer's state between the replays."""
  from mix_stage_amd import layers, ops
  from mix_stage_amd.train_step import MixStageTrainStep
  model = _build_gan(0.1)
  ts = MixStageTrainStep(model, use_graphs=True, dropout_seed=0xabcdef)
  blk = [b for b in model.D.modules() if isinstance(b, layers.ConvNormRelu)][0]
  batch = O.synthetic_batch(B, M=8, S=8, seed=61)
  audio, pose, labels_in, style = [t.to(DEV) for t in batch]
  seen = []
  for k in range(3):
    ts.step(audio, labels_in, pose, style, kind='D')
    assert ts.dropout_state()['step'] == k + 1
    for visit in (0, 1):
      site = R.site_of(blk._drop_id, visit)
      got = ops.dropout_mask((B, 128, 16), 0.1, site, ts._dropout_state).cpu()
      exp = torch.from_numpy(R.mask_like((B, 128, 16), 0.1, R.seed_words(0xabcdef), site, k + 1))
      assert torch.equal(got, exp)
      seen.append(got)
  assert len(ts._graphs) == 1
  for i in range(len(seen)):
    for j in range(i):
      assert not torch.equal(seen[i], seen[j])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_python_refusals(monkeypatch):
  import mix_stage_amd as A
  from mix_stage_amd import ops, train_step
  from mix_stage_amd.train_step import MixStageTrainStep
  with pytest.raises(ValueError):
    A.ConvNormRelu(4, 4, p=1.0)
  state = _state()
  t = torch.randn(2, 4, 8, device=DEV)
  v = torch.ones(4, device=DEV)
  for bad_p in (1.0, -0.5, 2.0, float('nan'), 0.0):
    with pytest.raises(ValueError):
      ops.dropout_bn_act(t, v, v, v.clone(), v.clone(), 0.2, 1e-5, 0.1, bad_p, 0, state)
  for bad_state in (None, state.cpu(), state.float(), torch.zeros(3, dtype=torch.int32, device=DEV)):
    with pytest.raises(TypeError):
      ops.dropout_bn_act(t, v, v, v.clone(), v.clone(), 0.2, 1e-5, 0.1, 0.5, 0, bad_state)
  with pytest.raises(NotImplementedError, match="bn_sync='global'"):
    MixStageTrainStep(_build_gan(0.1), bn_sync='global')
  monkeypatch.setattr(train_step, '_dp_world', lambda pg=None: 2)
  with pytest.raises(NotImplementedError, match='single-rank'):
    MixStageTrainStep(_build_gan(0.1))
  # the block itself, should the global statistics be switched on behind the trainer's back
  monkeypatch.setattr(ops, 'bn_sync_active', lambda: True)
  blk = _mk(CASES[1], 1)
  with pytest.raises(NotImplementedError, match="bn_sync='global'"):
    blk(torch.randn(2, 3, 7, device=DEV))


def test_c_abi_refusals_return_before_any_launch():
  from mix_stage_amd import _lib
  L = _lib.lib()
  Bn, C, HW = 2, 8, 2049
  t = lambda *s: torch.randn(*s, device=DEV)
  y_raw, y, dy, dyr, save, g = t(Bn, C, HW), t(Bn, C, HW), t(Bn, C, HW), t(Bn, C, HW), t(4 * C), t(C)
  rm, rv = t(C), t(C).abs() + 0.5
  state = _state()
  need = L.ms_dropout_bn_workspace(Bn, C, HW)
  assert need == 2 * C * 2 * 4
  ws = torch.full((need,), 0x55, dtype=torch.uint8, device=DEV)
  P = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  before = [x.clone() for x in (y, dyr, save, rm, rv, ws, state)]

  def fwd(p=0.25, state_=state, ws_=ws, nbytes=need):
    return L.ms_dropout_bn_fwd(P(y_raw), P(g), P(g), P(rm), P(rv), P(y), P(save), Bn, C, HW, 0.2, 1e-5, 0.1, 0, 0, p, 7, P(state_), P(ws_), nbytes, s)

  def bwd(p=0.25, state_=state, ws_=ws, nbytes=need):
    return L.ms_dropout_bn_bwd(P(dy), P(y_raw), P(save), P(g), P(dyr), None, None, Bn, C, HW, 0.2, 1e-5, 0, 0, p, 7, P(state_), P(ws_), nbytes, s)
  for fn in (fwd, bwd):
    assert fn(state_=None) != 0 and 'state' in L.ms_last_error().decode()
    assert fn(nbytes=need - 1) != 0 and 'workspace' in L.ms_last_error().decode()
    assert fn(ws_=None) != 0 and 'workspace' in L.ms_last_error().decode()
    for bad_p in (1.0, -0.1, 1.5, float('nan')):
      assert fn(p=bad_p) != 0 and '[0, 1)' in L.ms_last_error().decode()
  assert L.ms_dropout_advance(None, s) != 0 and L.ms_dropout_mask(P(y), 16, 1, 0.5, 0, None, s) != 0
  assert L.ms_dropout_mask(P(y), 16, 1, 1.0, 0, P(state), s) != 0 and L.ms_dropout_mask(P(y), 16, 0, 0.5, 0, P(state), s) != 0
  torch.cuda.synchronize()
  for a, b in zip(before, (y, dyr, save, rm, rv, ws, state)):
    assert torch.equal(a, b)
  # ... and with everything in order both run, the step word moves by one
  assert fwd() == 0 and bwd() == 0 and L.ms_dropout_advance(P(state), s) == 0
  torch.cuda.synchronize()
  assert state.cpu().tolist()[2] == 1 and not torch.equal(y, before[0]) and not torch.equal(dyr, before[1])
