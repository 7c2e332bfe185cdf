"""CPU: frozen BatchNorm statistics (layers.freeze_batchnorm, MixStageTrainStep(freeze_bn=)) -- the flags and what carries them,
the validation of freeze_bn=, the C-ABI declarations the differentiable BN_EVAL form uses (no signature moved), and the float64
reference the GPU tests compare with (tests/test_gpu_frozen_bn.py imports frozen_reference from here), checked against the closed
form of DESIGN 4m."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frozen_reference(x, w, bias, gamma, beta, rm, rv, stride, padding, groups, slope, eps):
  """conv -> batch_norm(training=False) -> leaky_relu in the dtype of its arguments (the tests hand it float64 leaves), under
  autograd.  x (B, C, T) or (B, C, H, W)."""
  conv = F.conv1d if x.dim() == 3 else F.conv2d
  y_raw = conv(x, w, bias, stride=stride, padding=padding, groups=groups)
  z = F.batch_norm(y_raw, rm, rv, gamma, beta, training=False, eps=eps)
  return F.leaky_relu(z, slope)


def closed_form(x, w, bias, gamma, beta, rm, rv, stride, padding, groups, slope, eps, dy):
  """The formulas of the frozen block written out (include/mixstage.h, ms_conv_block_bwd): -> y, dy_raw, dgamma, dbeta, dbias."""
  conv = F.conv1d if x.dim() == 3 else F.conv2d
  y_raw = conv(x, w, bias, stride=stride, padding=padding, groups=groups)
  shape = [1, -1] + [1] * (x.dim() - 2)
  invstd = 1.0 / torch.sqrt(rv + eps)
  s = gamma * invstd
  xhat = (y_raw - rm.view(shape)) * invstd.view(shape)
  z = gamma.view(shape) * xhat + beta.view(shape)
  y = torch.where(z > 0, z, slope * z)
  dz = dy * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
  dy_raw = dz * s.view(shape)
  red = [0] + list(range(2, x.dim()))
  return y, dy_raw, (dz * xhat).sum(red), dz.sum(red), dy_raw.sum(red)


@pytest.mark.parametrize('nd,slope', [(1, 0.2), (2, 0.2), (1, 0.0)])
def test_reference_equals_the_closed_form(nd, slope):
  g = torch.Generator().manual_seed(3 + nd)
  B, cin, cout, groups = 3, 4, 6, 2
  sp = (9,) if nd == 1 else (5, 7)
  k = (3,) * nd
  x = torch.randn(B, cin * groups, *sp, generator=g, dtype=torch.float64).requires_grad_()
  w = torch.randn(cout * groups, cin, *k, generator=g, dtype=torch.float64).requires_grad_()
  bias, gamma, beta = [torch.randn(cout * groups, generator=g, dtype=torch.float64).requires_grad_() for _ in range(3)]
  rm = torch.randn(cout * groups, generator=g, dtype=torch.float64)
  rv = torch.rand(cout * groups, generator=g, dtype=torch.float64) + 0.1
  args = (x, w, bias, gamma, beta, rm, rv, 1, 1, groups, slope, 1e-5)
  rm0, rv0 = rm.clone(), rv.clone()
  y = frozen_reference(*args)
  dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
  y.backward(dy)
  assert torch.equal(rm, rm0) and torch.equal(rv, rv0)            # the statistics are read, never written
  with torch.no_grad():
    y2, dy_raw, dgamma, dbeta, dbias = closed_form(*args, dy)
    conv_t = F.conv_transpose1d if nd == 1 else F.conv_transpose2d
    dx = conv_t(dy_raw, w, None, stride=1, padding=1, groups=groups)
  for name, got, exp in (('y', y2, y), ('dgamma', dgamma, gamma.grad), ('dbeta', dbeta, beta.grad), ('dbias', dbias, bias.grad), ('dx', dx, x.grad)):
    assert (got - exp.detach()).abs().max().item() <= 1e-12 * max(1.0, exp.abs().max().item()), name


def _model():
  import mix_stage_amd as A
  G = A.JointLateClusterSoftStyle4_G(num_clusters=8, style_dict={i: i for i in range(8)}, shape={})
  D = A.Speech2Gesture_D()
  return A.GAN(G, D, criterion='L1Loss', input_modalities=['audio/log_mel_400'])


def test_helpers_flag_exactly_the_conv_norm_relu_blocks():
  from mix_stage_amd import layers
  m = _model()
  before = {k: v.clone() for k, v in m.state_dict().items()}
  blocks = [b for b in m.modules() if isinstance(b, layers.ConvNormRelu)]
  assert layers.frozen_batchnorm_blocks(m) == []
  n = layers.freeze_batchnorm(m.G.unet)
  assert n == len([b for b in m.G.unet.modules() if isinstance(b, layers.ConvNormRelu)]) == 12
  assert layers.frozen_batchnorm_blocks(m) == [b for b in blocks if any(b is u for u in m.G.unet.modules())]
  assert not any(hasattr(o, '_bn_frozen') for o in m.modules() if not isinstance(o, layers.ConvNormRelu))
  assert layers.freeze_batchnorm(m) == len(blocks) and layers.frozen_batchnorm_blocks(m) == blocks
  # a plain attribute: the state_dict (409 keys) neither names it nor moved, `training` is untouched, deepcopy carries it
  after = m.state_dict()
  assert list(after.keys()) == list(before.keys()) and len(after) == 409
  assert all(torch.equal(after[k], before[k]) for k in before)
  assert all(b.training for b in blocks)
  assert len(layers.frozen_batchnorm_blocks(copy.deepcopy(m))) == len(blocks)
  assert layers.freeze_batchnorm(m.D, False) == 2 and len(layers.frozen_batchnorm_blocks(m)) == len(blocks) - 2
  assert layers.freeze_batchnorm(torch.nn.Linear(2, 2)) == 0


def test_a_frozen_block_tracks_no_batches_and_plans_no_corun():
  from mix_stage_amd import layers
  blk = layers.ConvNormRelu(4, 4, leaky=True)
  x = torch.zeros(2, 4, 8, requires_grad=True)
  from mix_stage_amd._lib import MS_BN_EVAL, MS_BN_TRAIN
  assert blk._next_desc(x).mode == MS_BN_TRAIN
  layers.freeze_batchnorm(blk)
  assert blk.training and blk._next_desc(x) is None            # (gradients enabled: two launches, no hold)
  with torch.no_grad():
    assert blk._next_desc(x).mode == MS_BN_EVAL                # (no gradient: today's one-launch eval form)
  assert blk._pending_batches == 0


def test_freeze_bn_argument_is_validated():
  from mix_stage_amd import layers
  from mix_stage_amd.train_step import MixStageTrainStep
  m = _model()
  roots = layers.freeze_bn_roots
  assert roots(m, None) == [] and roots(m, True) == [m] and roots(m, 'G') == [m.G] and roots(m, 'D') == [m.D]
  assert roots(m, ['G.unet', m.D.conv3]) == [m.G.unet, m.D.conv3]
  for bad in ('X', 'G.unet', 3, 2.5, m.G, ['G.nope'], [7], [torch.nn.Linear(1, 1)]):
    with pytest.raises(ValueError):
      roots(m, bad)
    with pytest.raises(ValueError):
      MixStageTrainStep(m, freeze_bn=bad)                      # (checked before anything touches a device)
  assert layers.frozen_batchnorm_blocks(m) == []


def _decl(name):
  hdr = open(os.path.join(ROOT, 'include', 'mixstage.h')).read()
  hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
  m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, hdr, flags=re.S)
  assert m, '%s is not declared in include/mixstage.h' % name
  return [a.strip() for a in m.group(1).split(',')]


def test_header_and_signatures_agree_and_the_abi_did_not_move():
  from mix_stage_amd import _lib
  for name, n in (('ms_conv_block_fwd', 15), ('ms_conv_block_fwd_ex', 16), ('ms_conv_block_bwd', 21), ('ms_conv_block_bwd_ex', 22)):
    args = _decl(name)
    restype, argtypes = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and len(args) == len(argtypes) == n, name
  assert [a.split()[-1] for a in _decl('ms_conv_block_fwd')[9:12]] == ['y_raw', 'y', 'save']
  L = _lib.lib()
  assert L.ms_abi_version() == 4
  # the workspace sizes name the bytes of the frozen forms: the conv runs as the block's MS_BARE launch, the backward is mode-blind
  for geo in ((2, 256, 1, 64, 256, 1, 1, 3, 1, 1, 0, 1, 1, 64), (2, 64, 16, 16, 64, 1, 3, 3, 1, 1, 1, 1, 16, 16)):
    by_mode = {}
    for mode in (_lib.MS_BARE, _lib.MS_BN_EVAL):
      d = _lib.ConvDesc(*geo, mode, _lib.MS_IN_PLAIN, 0.2, 1e-5, 0.1, _lib.MS_DT_BN_FROZEN if mode == _lib.MS_BN_EVAL else 0)
      by_mode[mode] = (L.ms_conv_block_fwd_workspace(ctypes.byref(d)), L.ms_conv_block_bwd_workspace(ctypes.byref(d)))
    assert by_mode[_lib.MS_BARE] == by_mode[_lib.MS_BN_EVAL] and min(by_mode[_lib.MS_BN_EVAL]) >= 256
  hdr = open(os.path.join(ROOT, 'include', 'mixstage.h')).read()
  assert 'y_raw    BN_TRAIN only' not in hdr and 'save     BN_TRAIN only' not in hdr
  assert re.search(r'#define\s+MS_DT_BN_FROZEN\s+0x%x\b' % _lib.MS_DT_BN_FROZEN, hdr)
