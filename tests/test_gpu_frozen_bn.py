"""GPU: conv blocks with FROZEN BatchNorm statistics (layers.freeze_batchnorm; C-ABI: MS_BN_EVAL with MS_DT_BN_FROZEN, and its backward),
fp32, bf16x6, bf16 and fp16, against float64: F.conv* -> F.batch_norm(training=False) -> leaky_relu under autograd (test_frozen_bn_cpu.py
checks that reference against the closed form).  One case per launch form of the BatchNorm backward, the branch constants quoted
from launch_bn_bwd (csrc/elementwise.hip) and kernels.h next to each.

Bars: those of test_gpu_kernels._conv_block_case for the BN_TRAIN block of the same geometry -- forward 2e-5, gradients 1e-4,
relative to the tensor's max-abs (an element-wise bound) -- and the same figures on the Frobenius norm.  The bias gradient is a
real gradient here (sum of dy_raw), not the rounding noise it is in front of batch statistics: it takes the gradient bar.

Every backward case fails without the feature: _ConvBlockFn._backward raised 'backward through an eval-mode (running-stats)
ConvNormRelu is not on the path' for every MS_BN_EVAL block."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import mixstage_oracle as O
from test_frozen_bn_cpu import frozen_reference

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FWD_BAR, GRAD_BAR = 2e-5, 1e-4


def errs_of(a, b):
  """(max-abs error / max-abs of the reference, Frobenius error / Frobenius norm of the reference)."""
  a, b = a.detach().double().cpu(), b.detach().double().cpu()
  assert a.shape == b.shape, (a.shape, b.shape)
  return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item(), ((a - b).norm() / (b.norm() + 1e-30)).item()


# (name, nd, cin, cout, kernel, stride, groups, input spatial, B, in_mode, leaky) -- cin / cout per group
CASES = [
    # vec4 (HW % 4 == 0) && n = B*HW <= 1024: bn_bwd_fused4<1>.  The clip-resident conv (1-D k3 s1 256 -> 256, T = 64)
    ('f4_1_clip', 1, 256, 256, 3, 1, 1, (64,), 2, 'plain', True),
    # n <= 2048: bn_bwd_fused4<2>
    ('f4_2_clip_b32', 1, 256, 256, 3, 1, 1, (64,), 32, 'plain', True),
    # n <= BN_BWD32_FUSED_MAX = 256 * 16 = 4096: bn_bwd_fused4<4>
    ('f4_4_2d', 2, 64, 64, 3, 1, 1, (16, 16), 16, 'plain', True),
    # HW % 4 != 0, n <= 256 * 4: bn_bwd_fused<4> (D.conv3's shape: k4 s1, T = 16 -> 15)
    ('f_4_dconv3', 1, 256, 256, 4, 1, 1, (16,), 2, 'plain', True),
    # ... n <= 256 * 8: bn_bwd_fused<8>;  n <= 256 * 16: bn_bwd_fused<16>  (HW = 15, n = 1500 / 3000)
    ('f_8', 1, 8, 8, 4, 1, 1, (16,), 100, 'plain', True),
    ('f_16', 1, 8, 8, 4, 1, 1, (16,), 200, 'plain', True),
    # HW = 1 (the style encoder's tail: k4 s2, T = 2 -> 1): bn_bwd_fused<4>
    ('f_4_hw1', 1, 256, 8, 4, 2, 1, (2,), 2, 'plain', True),
    # 2-D 4x4 s2 64 -> 64 on 64 x 64 (HW = 1024).  B = 2: n = 2048, bn_bwd_fused4<2>;  B = 5: n = 5120 > BN_BWD32_FUSED_MAX, the
    # two-pass bn_bwd(reduce4+apply4)
    ('f4_2_2d_s2', 2, 64, 64, 4, 2, 1, (64, 64), 2, 'plain', True),
    ('r4a4_2d_s2', 2, 64, 64, 4, 2, 1, (64, 64), 5, 'plain', True),
    # its HW % 4 != 0 twin (62 x 62 -> 31 x 31 = 961, n = 4805): bn_bwd(reduce+apply) + colsum_finalize
    ('ra_2d_s2', 2, 64, 64, 4, 2, 1, (62, 62), 5, 'plain', True),
    # the scalar two passes again, HW % 4 != 0: (B, C, HW) = (3, 600, 1367), bwd_chunks wants 2 chunks -> 2 + 1 batch items, 4101 values
    # per channel;  (5, 3, 821): five chunks of one item
    ('ra_c600_b3', 1, 8, 600, 3, 1, 1, (1367,), 3, 'plain', True),
    ('ra_c3_b5', 1, 3, 3, 3, 1, 1, (821,), 5, 'plain', True),
    # input modes: MS_IN_UP2ADD (T = 8 from 4), MS_IN_BCAST with 2 groups
    ('up2add', 1, 256, 256, 3, 1, 1, (8,), 2, 'up2', True),
    ('bcast_g2', 1, 10, 33, 3, 1, 2, (19,), 3, 'bcast', True),
    # the first conv, 1 -> 64 3x3 (conv_c1 and its weight-gradient stream)
    ('conv_c1', 2, 1, 64, 3, 1, 1, (8, 20), 2, 'plain', True),
    # ReLU: slope 0
    ('relu', 1, 256, 256, 3, 1, 1, (64,), 2, 'plain', False),
]
IDS = [c[0] for c in CASES]


def _mk(case, seed, adverse=False):
  import mix_stage_amd as A
  name, nd, cin, cout, k, s, g, sp, B, in_mode, leaky = case
  blk = A.ConvNormRelu(cin, cout, type='%dd' % nd, leaky=leaky, kernel_size=k, stride=s, groups=g)
  sd = O.deterministic_state({'fz%d.' % seed + kk: v for kk, v in blk.state_dict().items()})
  blk.load_state_dict({kk.split('.', 1)[1]: v for kk, v in sd.items()})
  gen = torch.Generator().manual_seed(1000 + seed)
  C = cout * g
  with torch.no_grad():
    # running statistics and an affine map that are nobody's defaults
    blk.norm.running_mean.copy_(0.3 * torch.randn(C, generator=gen))
    blk.norm.running_var.copy_(0.25 + torch.rand(C, generator=gen))
    blk.norm.weight.copy_(0.5 + torch.rand(C, generator=gen))
    blk.norm.bias.copy_(0.2 * torch.randn(C, generator=gen))
    blk.norm.num_batches_tracked.fill_(7)
    if adverse:
      blk.norm.weight[0::8] = 0.0                       # gamma == 0: y is constant, dgamma is not
      blk.norm.weight[1::8] *= -1.0                     # gamma < 0
      blk.norm.running_var[2::8] = 1e-12                # invstd = 1/sqrt(eps)
      blk.norm.bias[3::8] = 50.0                        # beta >> gamma: every z on one side of the kink
      blk.norm.bias[4::8] = -50.0
  return blk.to(DEV).train()


def _inputs(case, gen, B):
  name, nd, cin, cout, k, s, g, sp, _, in_mode, leaky = case
  if in_mode == 'up2':
    return [torch.randn(B, cin * g, sp[0] // 2, generator=gen), torch.randn(B, cin * g, sp[0], generator=gen)]
  return [torch.randn(B, cin if in_mode == 'bcast' else cin * g, *sp, generator=gen)]


def _run_hip(blk, case, xs):
  in_mode = case[9]
  leaves = [x.to(DEV).requires_grad_() for x in xs]
  if in_mode == 'up2':
    y = blk.forward_upsample_add(*leaves)
  else:
    y = blk.forward_broadcast(leaves[0]) if in_mode == 'bcast' else blk(leaves[0])
  return y, leaves


def _run_ref(blk, case, xs):
  name, nd, cin, cout, k, s, g, sp, _, in_mode, leaky = case
  leaves = [x.double().requires_grad_() for x in xs]
  if in_mode == 'up2':
    xin = F.interpolate(leaves[0], scale_factor=2, mode='nearest') + leaves[1]
  else:
    xin = torch.cat([leaves[0]] * g, dim=1) if in_mode == 'bcast' else leaves[0]
  ps = {n: t.detach().double().cpu().requires_grad_() for n, t in
        (('w', blk.conv.weight), ('bias', blk.conv.bias), ('gamma', blk.norm.weight), ('beta', blk.norm.bias))}
  rm, rv = blk.norm.running_mean.detach().double().cpu(), blk.norm.running_var.detach().double().cpu()
  y = frozen_reference(xin, ps['w'], ps['bias'], ps['gamma'], ps['beta'], rm, rv, blk.conv.stride, blk.conv.padding, g,
                       0.2 if leaky else 0.0, blk.norm.eps)
  return y, leaves, ps


def _labels_of(fn):
  from mix_stage_amd import ops
  ops.timing_enable(True)
  try:
    out = fn()
    torch.cuda.synchronize()
    return out, [r['label'].split('|')[-1] for r in ops.timing_report() for _ in range(r['count'])]
  finally:
    ops.timing_enable(False)


def _check_labels(labels):
  apply_l = [l for l in labels if l.startswith('bn_apply')]
  bwd_l = [l for l in labels if l.startswith('bn_bwd')]
  assert len(apply_l) == 1 and apply_l[0].endswith(' frozen'), labels
  assert len(bwd_l) == 1 and bwd_l[0].endswith(' frozen'), labels
  assert not any('bn_finalize' in l or 'bnstats' in l or 'bnfused' in l for l in labels), labels
  assert any('dgrad' in l for l in labels) and any('wgrad' in l for l in labels), labels
  # the conv ran as the block's BARE launch: no statistics suffix, epilogue 0 (EP_BARE) wherever the label names one
  fwd_l = [l for l in labels if 'conv_fwd' in l]
  assert fwd_l and all('+bn' not in l and (' ep' not in l or l.endswith(' ep0')) for l in fwd_l), labels
  assert all(' ep0' in l for l in labels if l.startswith('splitk_fwd_epilogue')), labels
  return bwd_l[0]


def _case(case, seed, adverse=False, expect=None):
  """-> False where a pre-activation sits within fp32 rounding of the LeakyReLU kink (the caller draws again)."""
  from mix_stage_amd import layers
  B = case[8]
  blk = _mk(case, seed, adverse)
  assert layers.freeze_batchnorm(blk) == 1
  buf0 = [blk.norm.running_mean.clone(), blk.norm.running_var.clone(), blk.norm.num_batches_tracked.clone()]
  gen = torch.Generator().manual_seed(seed)
  xs = _inputs(case, gen, B)
  y_ref, leaves_ref, ps = _run_ref(blk, case, xs)
  gy = torch.randn(y_ref.shape, generator=gen)

  def step():
    y, leaves = _run_hip(blk, case, xs)
    y.backward(gy.to(DEV))
    return y, leaves
  (y, leaves), labels = _labels_of(step)
  figs = {'fwd': (errs_of(y, y_ref), FWD_BAR)}
  if ((y.detach().cpu() > 0) != (y_ref.detach() > 0)).any():
    assert max(figs['fwd'][0]) < FWD_BAR, figs
    return False
  y_ref.backward(gy.double())
  for i, (a, b) in enumerate(zip(leaves, leaves_ref)):
    figs['dx%d' % i] = (errs_of(a.grad, b.grad), GRAD_BAR)
  for n, t in (('w', blk.conv.weight), ('bias', blk.conv.bias), ('gamma', blk.norm.weight), ('beta', blk.norm.bias)):
    figs['d' + n] = (errs_of(t.grad, ps[n].grad), GRAD_BAR)
  print(case[0], 'adverse' if adverse else '', {k: '%.2e/%.2e' % v[0] for k, v in figs.items()})
  bad = {k: v for k, v in figs.items() if not max(v[0]) < v[1]}
  assert not bad, 'errors ((max-abs, norm), bar): %s | all: %s' % (bad, figs)
  # the statistics are read, never written; no tracked batch
  assert torch.equal(blk.norm.running_mean, buf0[0]) and torch.equal(blk.norm.running_var, buf0[1])
  assert torch.equal(blk.state_dict()['norm.num_batches_tracked'], buf0[2]) and blk._pending_batches == 0
  bwd_label = _check_labels(labels)
  if expect is not None:
    assert bwd_label.startswith(expect), (bwd_label, expect)
  # clip independence: clip 0 in a batch of 4 against clip 0 alone (to the forward / gradient bars: the tile mapping may differ)
  xs4 = _inputs(case, torch.Generator().manual_seed(seed + 1), 4)
  y4, l4 = _run_hip(blk, case, xs4)
  g4 = torch.randn(y4.shape, generator=gen)
  y4.backward(g4.to(DEV))
  y1, l1 = _run_hip(blk, case, [x[:1] for x in xs4])
  y1.backward(g4[:1].to(DEV))
  assert max(errs_of(y4[:1], y1)) < FWD_BAR
  for a, b in zip(l4, l1):
    assert max(errs_of(a.grad[:1], b.grad)) < FWD_BAR
  return True


EXPECT = {'f4_1_clip': 'bn_bwd_fused4<1>', 'f4_2_clip_b32': 'bn_bwd_fused4<2>', 'f4_4_2d': 'bn_bwd_fused4<4>', 'f_4_dconv3': 'bn_bwd_fused<4>',
          'f_8': 'bn_bwd_fused<8>', 'f_16': 'bn_bwd_fused<16>', 'f_4_hw1': 'bn_bwd_fused<4>', 'f4_2_2d_s2': 'bn_bwd_fused4<2>',
          'r4a4_2d_s2': 'bn_bwd(reduce4+apply4)', 'ra_2d_s2': 'bn_bwd(reduce+apply)', 'ra_c600_b3': 'bn_bwd(reduce+apply)',
          'ra_c3_b5': 'bn_bwd(reduce+apply)', 'up2add': 'bn_bwd_fused4<1>',
          'bcast_g2': 'bn_bwd_fused<4>', 'conv_c1': 'bn_bwd_fused4<1>', 'relu': 'bn_bwd_fused4<1>'}


def _draws(case, adverse=False, expect=None):
  for attempt in range(4):
    if _case(case, zlib.crc32(case[0].encode()) % 1000 + attempt, adverse, expect):
      return
  raise AssertionError('no draw without a sign flip at a LeakyReLU kink')


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_frozen_block_fwd_bwd_vs_fp64(case):
  _draws(case, expect=EXPECT[case[0]])


@pytest.mark.parametrize('case', [c for c in CASES if c[0] in ('ra_c600_b3', 'ra_c3_b5')], ids=lambda c: c[0])
def test_two_pass_backward_with_batch_statistics(case):
  """The two shapes of the scalar two-pass backward with BATCH statistics (the block as it trains, not frozen): forward and every
  gradient against fp64 with the bars above.  The conv bias is left out: in front of batch statistics its gradient is zero but for
  rounding, so there is no reference magnitude to hold an error against."""
  name, nd, cin, cout, k, s, g, sp, B, in_mode, leaky = case
  for attempt in range(4):
    seed = zlib.crc32(name.encode()) % 1000 + 100 + attempt
    blk = _mk(case, seed)
    gen = torch.Generator().manual_seed(seed)
    xs = _inputs(case, gen, B)
    leaves_ref = [x.double().requires_grad_() for x in xs]
    ps = {n: t.detach().double().cpu().requires_grad_() for n, t in
          (('w', blk.conv.weight), ('bias', blk.conv.bias), ('gamma', blk.norm.weight), ('beta', blk.norm.bias))}
    raw = F.conv1d(leaves_ref[0], ps['w'], ps['bias'], stride=blk.conv.stride, padding=blk.conv.padding, groups=g)
    y_ref = F.leaky_relu(F.batch_norm(raw, None, None, ps['gamma'], ps['beta'], training=True, eps=blk.norm.eps), 0.2 if leaky else 0.0)
    gy = torch.randn(y_ref.shape, generator=gen)

    def step():
      y, leaves = _run_hip(blk, case, xs)
      y.backward(gy.to(DEV))
      return y, leaves
    (y, leaves), labels = _labels_of(step)
    figs = {'fwd': (errs_of(y, y_ref), FWD_BAR)}
    if ((y.detach().cpu() > 0) != (y_ref.detach() > 0)).any():
      assert max(figs['fwd'][0]) < FWD_BAR, figs
      continue
    y_ref.backward(gy.double())
    figs['dx'] = (errs_of(leaves[0].grad, leaves_ref[0].grad), GRAD_BAR)
    for n, t in (('w', blk.conv.weight), ('gamma', blk.norm.weight), ('beta', blk.norm.bias)):
      figs['d' + n] = (errs_of(t.grad, ps[n].grad), GRAD_BAR)
    print(name, 'batch statistics', {kk: '%.2e/%.2e' % v[0] for kk, v in figs.items()})
    bad = {kk: v for kk, v in figs.items() if not max(v[0]) < v[1]}
    assert not bad, 'errors ((max-abs, norm), bar): %s | all: %s' % (bad, figs)
    bwd_l = [l for l in labels if l.startswith('bn_bwd')]
    assert len(bwd_l) == 1 and bwd_l[0].startswith('bn_bwd(reduce+apply)') and not bwd_l[0].endswith(' frozen'), labels
    return
  raise AssertionError('no draw without a sign flip at a LeakyReLU kink')


@pytest.mark.parametrize('case', [c for c in CASES if c[0] in ('f4_1_clip', 'ra_2d_s2', 'relu')], ids=lambda c: c[0])
def test_frozen_block_adverse_parameters(case):
  """gamma == 0, gamma < 0, running_var = 1e-12, |beta| >> gamma: y_raw is kept and nothing is inverted from y, so dgamma holds."""
  _draws(case, adverse=True)


@pytest.mark.parametrize('case', [c for c in CASES if c[0] in ('f4_1_clip', 'f4_4_2d')], ids=lambda c: c[0])
def test_frozen_block_bf16x6(case):
  from mix_stage_amd import _lib
  old = _lib.lib().ms_set_precision(1)
  try:
    _draws(case)
  finally:
    _lib.lib().ms_set_precision(old)


@pytest.mark.parametrize('case', [c for c in CASES if c[0] in ('f4_1_clip', 'r4a4_2d_s2', 'ra_2d_s2')], ids=lambda c: c[0])
def test_affine_off_same_bits_and_no_affine_gradient(case):
  from mix_stage_amd import layers
  seed = 5
  xs = _inputs(case, torch.Generator().manual_seed(seed), case[8])
  out = []
  for affine in (True, False):
    blk = _mk(case, seed)
    layers.freeze_batchnorm(blk)
    blk.norm.weight.requires_grad_(affine)
    blk.norm.bias.requires_grad_(affine)
    y, leaves = _run_hip(blk, case, xs)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 1))
    y.backward(gy.to(DEV))
    out.append((y.detach(), leaves[0].grad, blk.conv.weight.grad, blk.conv.bias.grad))
    assert (blk.norm.weight.grad is None) == (not affine) and (blk.norm.bias.grad is None) == (not affine)
  for a, b in zip(*out):
    assert torch.equal(a, b)


def test_unflagged_twin_behaves_as_before():
  from mix_stage_amd import layers
  case = CASES[0]
  xs = _inputs(case, torch.Generator().manual_seed(2), 2)
  plain, flagged = _mk(case, 9), _mk(case, 9)
  layers.freeze_batchnorm(flagged)
  plain.eval()
  y, _ = _run_hip(plain, case, xs)
  with pytest.raises(RuntimeError, match='eval-mode'):
    y.backward(torch.ones_like(y))
  with torch.no_grad():
    (y_f, _), labels = _labels_of(lambda: _run_hip(flagged, case, [x for x in xs]))
    y_p, _ = _run_hip(plain, case, xs)
  assert torch.equal(y_f, y_p)                          # a frozen block without gradients is the one-launch eval form
  assert not any('frozen' in l or 'bn_apply' in l for l in labels), labels
  # ... and the flag taken off again gives the batch-statistics block back
  layers.freeze_batchnorm(flagged, False)
  rm0 = flagged.norm.running_mean.clone()
  _run_hip(flagged, case, xs)
  assert not torch.equal(flagged.norm.running_mean, rm0) and flagged._pending_batches == 1


def test_c_abi_refusals():
  """MS_DT_BN_FOLDED with the flag, a missing save / y_raw, dy_is_dyr on a BN_EVAL block and the side-stream form are
  errors that say so; without the flag BN_EVAL is the eval form it always was."""
  import ctypes
  from mix_stage_amd import _lib, ops
  L = _lib.lib()
  geo = (2, 8, 1, 16, 8, 1, 1, 3, 1, 1, 0, 1, 1, 16)
  t = lambda *s: torch.randn(*s, device=DEV)
  x, w, v, y, y_raw, save = t(2, 8, 16), t(8, 8, 1, 3), t(8).abs() + 0.5, t(2, 8, 16), t(2, 8, 16), t(32)
  p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

  def fwd(dtype, y_raw_, save_):
    d = _lib.ConvDesc(*geo, _lib.MS_BN_EVAL, _lib.MS_IN_PLAIN, 0.2, 1e-5, 0.1, dtype)
    ws = torch.empty(L.ms_conv_block_fwd_workspace(ctypes.byref(d)), dtype=torch.uint8, device=DEV)
    return L.ms_conv_block_fwd(ctypes.byref(d), p(x), None, p(w), p(v), p(v), p(v), p(v), p(v), p(y_raw_), p(y), p(save_), p(ws), ws.numel(), s)
  FZ = _lib.MS_DT_BN_FROZEN
  assert fwd(_lib.MS_BF16 | _lib.MS_DT_BN_FOLDED | FZ, y_raw, save) != 0 and 'MS_DT_BN_FOLDED' in L.ms_last_error().decode()
  assert fwd(FZ, y_raw, None) != 0 and 'save' in L.ms_last_error().decode()
  assert fwd(FZ, None, save) != 0 and 'y_raw' in L.ms_last_error().decode()
  # without the flag a BN_EVAL block is the one-launch eval form, whatever y_raw / save point to: they are not written
  y_raw0, save0 = y_raw.clone(), save.clone()
  assert fwd(0, y_raw, save) == 0
  torch.cuda.synchronize()
  assert torch.equal(y_raw, y_raw0) and torch.equal(save, save0)
  y_eval = y.clone()
  assert fwd(FZ, y_raw, save) == 0
  torch.cuda.synchronize()
  assert not torch.equal(y_raw, y_raw0) and not torch.equal(save, save0)
  assert ((y - y_eval).abs().max() / y_eval.abs().max()).item() < FWD_BAR
  bad = _lib.ConvDesc(*geo, _lib.MS_BN_TRAIN, _lib.MS_IN_PLAIN, 0.2, 1e-5, 0.1, FZ)
  assert L.ms_conv_block_fwd_workspace(ctypes.byref(bad)) >= 256
  assert L.ms_stat_pair_ok(ctypes.byref(bad)) == 0 and 'MS_DT_BN_FROZEN' in L.ms_last_error().decode()

  d = _lib.ConvDesc(*geo, _lib.MS_BN_EVAL, _lib.MS_IN_PLAIN, 0.2, 1e-5, 0.1, FZ)
  ws = torch.empty(L.ms_conv_block_bwd_workspace(ctypes.byref(d)), dtype=torch.uint8, device=DEV)
  dy, dyr, dx, dw = t(2, 8, 16), t(2, 8, 16), t(2, 8, 16), t(8, 8, 1, 3)

  def bwd(opt, y_raw_=y_raw):
    return L.ms_conv_block_bwd_ex(ctypes.byref(d), p(x), None, p(w), p(v), None, None, p(y_raw_), None, p(save), p(dy), p(dyr), p(dx), None,
                                  p(dw), None, None, None, p(ws), ws.numel(), s, ctypes.byref(opt))
  o = _lib.BwdOptions(None, None, 0, None, None, 0)
  assert bwd(o) == 0
  # affine off: NULL for dgamma / dbeta -- same dy_raw / dx / dw bits as with the buffers, and a poisoned buffer that is NOT handed
  # over stays as it was (one that is handed over is written)
  torch.cuda.synchronize()
  base = [t.clone() for t in (dyr, dx, dw)]
  poison = torch.full((2, 8), float('nan'), device=DEV)
  rc = L.ms_conv_block_bwd_ex(ctypes.byref(d), p(x), None, p(w), p(v), None, None, p(y_raw), None, p(save), p(dy), p(dyr), p(dx), None,
                              p(dw), None, p(poison[0]), p(poison[1]), p(ws), ws.numel(), s, ctypes.byref(o))
  torch.cuda.synchronize()
  assert rc == 0 and torch.isfinite(poison).all() and all(torch.equal(a_, b_) for a_, b_ in zip(base, (dyr, dx, dw)))
  poison.fill_(float('nan'))
  assert bwd(o) == 0
  torch.cuda.synchronize()
  assert torch.isnan(poison).all() and all(torch.equal(a_, b_) for a_, b_ in zip(base, (dyr, dx, dw)))
  assert bwd(o, None) != 0 and 'y_raw' in L.ms_last_error().decode()
  o.dy_is_dyr = 1
  assert bwd(o) != 0 and 'dy_is_dyr' in L.ms_last_error().decode()
  side = torch.cuda.Stream()
  o2 = _lib.BwdOptions(side.cuda_stream, ws.data_ptr(), ws.numel(), None, None, 0)
  assert bwd(o2) != 0 and 'side-stream' in L.ms_last_error().decode()
  torch.cuda.synchronize()


# ---- stacks and neighbours ---------------------------------------------------------------------------------------------------------
def _unet_pair(seed):
  import mix_stage_amd as A
  hip = A.UNet1D(256, 256)
  sd = O.deterministic_state({'un%d.' % seed + k: v for k, v in hip.state_dict().items()})
  sd = {k.split('.', 1)[1]: v for k, v in sd.items()}
  gen = torch.Generator().manual_seed(seed)
  for k in sd:
    if k.endswith('running_mean'):
      sd[k] = 0.2 * torch.randn(sd[k].shape, generator=gen)
    elif k.endswith('running_var'):
      sd[k] = 0.5 + torch.rand(sd[k].shape, generator=gen)
  hip.load_state_dict(sd)
  ref = O.UNet1D(256, 256).double()
  ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
  return hip.to(DEV).train(), ref.train()


def _param_figs(hip, ref):
  """Gradient figures per parameter.  A conv bias in front of BATCH statistics has the true gradient 0 and both sides hold rounding
  noise: as in test_gpu_kernels._conv_block_case its magnitude is held against 1e-4 of the weight gradient's scale."""
  from mix_stage_amd import layers
  rp, figs = dict(ref.named_parameters()), {}
  for name, blk in hip.named_modules():
    if not isinstance(blk, layers.ConvNormRelu):
      continue
    for n, p_ in blk.named_parameters():
      full = name + '.' + n
      if n == 'conv.bias' and not getattr(blk, '_bn_frozen', False):
        scale = rp[name + '.conv.weight'].grad.abs().max().item()
        figs[full + '(~0)'] = ((p_.grad.abs().max().item(), 0.0), GRAD_BAR * max(scale, 1.0))
      else:
        figs[full] = (errs_of(p_.grad, rp[full].grad), GRAD_BAR)
  return figs


@pytest.mark.parametrize('which', ['all', 'conv1'])
def test_unet_frozen_vs_oracle(which):
  """UNet1D (256 channels, T = 64, B = 2) fully frozen, and with only the down path frozen (frozen and batch-statistics neighbours in
  both orders, the residual links through frozen blocks), against the oracle's UNet1D in float64 with the matching norm modules in
  .eval()."""
  from mix_stage_amd import layers, ops
  hip, ref = _unet_pair(3)
  roots_h = [hip] if which == 'all' else [hip.conv1]
  roots_r = [ref] if which == 'all' else [ref.conv1]
  for r in roots_h:
    layers.freeze_batchnorm(r)
  for r in roots_r:
    for m in r.modules():
      if isinstance(m, torch.nn.BatchNorm1d):
        m.eval()
  frozen = layers.frozen_batchnorm_blocks(hip)
  stats0 = [(b.norm.running_mean.clone(), b.norm.running_var.clone()) for b in frozen]
  gen = torch.Generator().manual_seed(11)
  x = torch.randn(2, 256, 64, generator=gen)
  gy = torch.randn(2, 256, 64, generator=gen)
  x64 = x.double().requires_grad_()
  y_ref = ref(x64)
  y_ref.backward(gy.double())
  xh = x.to(DEV).requires_grad_()
  links0 = ops._link_stats['in_launch']
  y = hip(xh)
  y.backward(gy.to(DEV))
  figs = {'fwd': (errs_of(y, y_ref), 2e-5 * 12), 'dx': (errs_of(xh.grad, x64.grad), GRAD_BAR)}     # (12 blocks deep: the block bar per block)
  figs.update(_param_figs(hip, ref))
  print(which, {k: '%.2e/%.2e' % v[0] for k, v in figs.items()})
  bad = {k: v for k, v in figs.items() if not max(v[0]) < v[1]}
  assert not bad, bad
  for b, (rm, rv) in zip(frozen, stats0):
    assert torch.equal(b.norm.running_mean, rm) and torch.equal(b.norm.running_var, rv) and b._pending_batches == 0
  assert all(b._pending_batches == 1 for b in hip.modules() if isinstance(b, layers.ConvNormRelu) and not any(b is f for f in frozen))
  assert ops._link_stats['in_launch'] - links0 >= 1        # the residual gradients still join inside data-gradient launches


@pytest.mark.parametrize('order', ['train_then_frozen', 'frozen_then_train'])
def test_stack_neighbours_both_orders(order):
  """A 1-D stack (the pose encoder's six k3 s1 blocks) with alternating frozen / batch-statistics blocks: a batch-statistics
  producer in front of a frozen consumer may ride in the consumer's data-gradient launch, a frozen producer never does."""
  import mix_stage_amd as A
  from mix_stage_amd import layers
  hip = A.PoseEncoder(input_channels=104)
  sd = O.deterministic_state({'pe.' + k: v for k, v in hip.state_dict().items()})
  sd = {k.split('.', 1)[1]: v for k, v in sd.items()}
  gen = torch.Generator().manual_seed(4)
  for k in sd:
    if k.endswith('running_var'):
      sd[k] = 0.5 + torch.rand(sd[k].shape, generator=gen)
  hip.load_state_dict(sd)
  ref = O.PoseEncoder(input_channels=104).double()
  ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
  hip, ref = hip.to(DEV).train(), ref.train()
  first = 1 if order == 'train_then_frozen' else 0
  for i in range(first, 6, 2):
    layers.freeze_batchnorm(hip.conv[i])
    ref.conv[i].norm.eval()
  x = torch.randn(2, 64, 104, generator=gen)
  x64 = x.double().requires_grad_()
  y_ref = ref(x64)
  gy = torch.randn(y_ref.shape, generator=gen)
  y_ref.backward(gy.double())
  xh = x.to(DEV).requires_grad_()

  def step():
    out = hip(xh)
    out.backward(gy.to(DEV))
    return out
  y, labels = _labels_of(step)
  figs = {'fwd': (errs_of(y, y_ref), 2e-5 * 6), 'dx': (errs_of(xh.grad, x64.grad), GRAD_BAR)}
  figs.update(_param_figs(hip, ref))
  print(order, {k: '%.2e/%.2e' % v[0] for k, v in figs.items()})
  bad = {k: v for k, v in figs.items() if not max(v[0]) < v[1]}
  assert not bad, bad
  assert sum(1 for l in labels if l.startswith('bn_bwd') and l.endswith(' frozen')) == 3, labels
  assert sum(1 for l in labels if l.startswith('bn_apply') and l.endswith(' frozen')) == 3, labels


def test_discriminator_pair_with_frozen_blocks_equals_two_passes():
  import mix_stage_amd as A
  from mix_stage_amd import layers
  torch.manual_seed(5)
  D = A.Speech2Gesture_D().to(DEV).train()
  layers.freeze_batchnorm(D)
  x = torch.randn(8, 104, 64, device=DEV)
  assert D.pair_supported(x)
  with torch.no_grad():
    a, b = D.forward_pair(x)
    a1, b1 = D.forward_channel_major(x[:4])[0], D.forward_channel_major(x[4:])[0]
  assert torch.equal(a, a1) and torch.equal(b, b1)
  # ... and differentiated (MS_DT_BN_FROZEN + MS_DT_STAT_PAIR: the bare conv on the batch of 2B, then the frozen apply launch): the two
  # halves are plain clips of one batch, the scores bit for bit those of the two passes
  xa = x.clone().requires_grad_()
  sa, sb = D.forward_pair(xa)
  sa1, sb1 = D.forward_channel_major(x[:4].clone().requires_grad_())[0], D.forward_channel_major(x[4:].clone().requires_grad_())[0]
  assert sa.requires_grad and sa1.requires_grad and torch.equal(sa, sa1) and torch.equal(sb, sb1)
  (sa.sum() - sb.sum()).backward()
  xb = x.clone().requires_grad_()
  (D.forward_channel_major(xb[:4])[0].sum() - D.forward_channel_major(xb[4:])[0].sum()).backward()
  assert max(errs_of(xa.grad, xb.grad)) < GRAD_BAR


# ---- 16-bit modes (bf16 / fp16 cb8) ---------------------------------------------------------------------------------------------------
# Bars: those of test_gpu_kernels16._case with bars='dtype', as applied to the BN_TRAIN block of the same geometry -- bf16: forward
# 1.2e-2 (with MS_DT_OUT_F32 too: the apply launch reads the STORED 16-bit y_raw, one 16-bit rounding in every form), gradients 2 x 2e-2 on the max (+ the 1e-6 floor) and 2e-2 in l2; fp16: the
# smaller of those / 8 and MODEL_K x the error helpers/round16_model.py emulates for the BN_TRAIN block in its two-launch form on
# this case's tensors.  The reference is float64 on the 16-bit-rounded operands; as for every block whose BatchNorm normalises the
# stored conv output, a pre-activation within one 16-bit rounding of 0 follows the device's mask (mask='device' there).
# (name, nd, B, cin, cout, groups, k, s, p, H, W, in_mode, out_f32)
CASES16 = [
    ('k3', 1, 4, 256, 256, 1, 3, 1, 1, 1, 64, 0, False),           # bn_bwd16 fused, n = 256
    ('k4s2', 1, 4, 64, 64, 1, 4, 2, 1, 1, 64, 0, False),
    ('up2add', 1, 4, 64, 64, 1, 3, 1, 1, 1, 16, 2, False),
    ('2d', 2, 2, 64, 128, 1, 3, 1, 1, 8, 16, 0, False),
    ('2d_two_pass', 2, 5, 16, 64, 1, 3, 1, 1, 24, 24, 0, False),     # n = 2880 > BN_BWD16_FUSED_MAX = 2048: bn_bwd16 reduce + apply
    ('k3_out_f32', 1, 4, 64, 64, 1, 3, 1, 1, 1, 64, 0, True),       # MS_DT_OUT_F32: fp32 y, fp32 dy
]


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('case', CASES16, ids=[c[0] for c in CASES16])
def test_frozen_block16_fwd_bwd_vs_fp64(case, dt):
  from helpers import round16_model as M16
  from mix_stage_amd import ops, ops16
  from mix_stage_amd._lib import MS_BF16, MS_BN_EVAL, MS_BN_TRAIN, MS_F16
  from test_gpu_kernels16 import MODEL_K, dtype_bar
  name, nd, B, cin, cout, groups, k, s, p, H, W, in_mode, out_f32 = case
  msdt = MS_BF16 if dt == torch.bfloat16 else MS_F16
  slope = 0.2
  opnd = M16.gen_operands(nd, B, cin, cout, groups, k, s, p, H, W, in_mode, 3, False)
  w, bias, gamma, beta, rm, rv = (opnd[n].to(DEV) for n in ('w', 'bias', 'gamma', 'beta', 'rm', 'rv'))
  rd = lambda t: t.to(dt).to(torch.float64)
  if in_mode == 2:
    a, r = opnd['a'].to(DEV).requires_grad_(), opnd['r'].to(DEV).requires_grad_()
    xa, xr = ops16.to_cb8(a, msdt), ops16.to_cb8(r, msdt)
  else:
    x = opnd['x'].to(DEV).requires_grad_()
    xc = ops16.to_cb8(x, msdt)
  wp, bp, gp, bep = (t.clone().requires_grad_() for t in (w, bias, gamma, beta))
  rm_h, rv_h = rm.clone(), rv.clone()
  geom = ops.ConvGeom(nd, groups, k, s, p, slope=slope)
  kw = dict(gamma=gp, beta=bep, running_mean=rm_h, running_var=rv_h, out_f32=out_f32, frozen=True)

  def step():
    if in_mode == 2:
      y_ = ops16.conv_block16(xa, wp, bp, geom, MS_BN_EVAL, x2=xr, in_mode=2, **kw)
    else:
      y_ = ops16.conv_block16(xc, wp, bp, geom, MS_BN_EVAL, in_mode=in_mode, **kw)
    y32_ = y_ if out_f32 else ops16.from_cb8(y_, cout * groups)
    dy_ = M16.gen_dy(opnd, y32_.shape, 1.0)
    (y32_ * dy_.to(DEV)).sum().backward()
    return y32_, dy_
  (y32, dy_cpu), labels = _labels_of(step)
  assert torch.equal(rm_h, rm) and torch.equal(rv_h, rv)
  assert sum(1 for l in labels if l.startswith('bn_apply16') and l.endswith(' frozen')) == 1, labels
  assert sum(1 for l in labels if l.startswith('bn_bwd16') and l.endswith(' frozen')) == 1, labels
  assert not any('bn_finalize' in l or 'bnstats' in l or 'bnfused' in l for l in labels), labels
  fwd_l = [l for l in labels if 'conv_fwd' in l]
  assert fwd_l and all('+bn' not in l for l in fwd_l), labels          # the conv ran as the block's BARE launch
  # float64 on the rounded operands
  w64, b64 = rd(w.cpu()).requires_grad_(), bias.cpu().double().requires_grad_()
  if in_mode == 2:
    a64, r64 = rd(a.detach().cpu()), rd(r.detach().cpu())
    xin = rd((a64.repeat_interleave(2, dim=-1) + r64).float()).requires_grad_()
  else:
    xin = rd(x.detach().cpu()).requires_grad_()
  conv = F.conv2d if nd == 2 else F.conv1d
  raw = conv(xin, w64, b64, stride=s, padding=p, groups=groups)
  g64, be64 = gamma.cpu().double().requires_grad_(), beta.cpu().double().requires_grad_()
  shape = (1, -1, 1, 1) if nd == 2 else (1, -1, 1)
  invstd = 1.0 / torch.sqrt(rv.cpu().double() + 1e-5)
  z = (raw - rm.cpu().double().view(shape)) * invstd.view(shape) * g64.view(shape) + be64.view(shape)
  pos = y32.detach().cpu() > 0
  flip = pos != (z.detach() > 0)
  u16 = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
  band = u16 * raw.detach().abs() * (g64.detach().abs() * invstd).view(shape) + 1e-5 * z.detach().abs().max().item()
  assert (flip & (z.detach().abs() > band)).sum().item() == 0 and flip.sum().item() <= 2e-3 * flip.numel()
  ref = torch.where(pos, z, slope * z)
  dy_used = dy_cpu.double() if out_f32 else rd(dy_cpu)
  (ref * dy_used).sum().backward()
  model = None
  if dt == torch.float16:
    model = M16.block_model(opnd, dy_cpu, nd, groups, s, p, MS_BN_TRAIN, in_mode, slope, out_f32, dt, 1.0, 'cpu', True, 'device', False)
  bar16 = lambda legacy, what: dtype_bar(legacy, model[what]) if model is not None else legacy
  figs = {}
  sc = ref.abs().max().item() + 1e-6
  figs['fwd'] = ((y32.detach().cpu().double() - ref.detach()).abs().max().item() / sc, bar16(1.2e-2, 'fwd'))

  def close(a_, b_, what, tol=2e-2):
    scb = b_.abs().max().item() + 1e-9
    a_ = a_.detach().cpu().double()
    figs[what] = ((a_ - b_).abs().max().item() / scb, bar16(2 * tol, what) + 1e-6 / scb)
    figs[what + ' l2'] = ((a_ - b_).norm().item() / (b_.norm().item() + 1e-12), bar16(tol, what + ' l2'))
  close(wp.grad, w64.grad, 'dw')
  close(gp.grad, g64.grad, 'dgamma')
  close(bep.grad, be64.grad, 'dbeta')
  if in_mode == 2:
    close(r.grad, xin.grad, 'dx2')
    close(a.grad, xin.grad.reshape(xin.grad.shape[0], xin.grad.shape[1], -1, 2).sum(-1), 'dx')
  else:
    close(x.grad, xin.grad, 'dx')
  # the bias gradient is a real gradient here: sum of dy_raw (the BN_TRAIN model has no figure for it: the dbeta bar, its twin)
  scb = b64.grad.abs().max().item() + 1e-9
  figs['dbias'] = ((bp.grad.cpu().double() - b64.grad).abs().max().item() / scb, figs['dbeta'][1])
  print(name, dt, {k_: '%.2e (bar %.2e)' % v for k_, v in figs.items()})
  bad = {k_: v for k_, v in figs.items() if not v[0] <= v[1]}
  assert not bad, bad
  # clip independence: clip 0 alone against clip 0 in the batch, outputs and dx to the forward bar of the dtype
  parts = [a, r] if in_mode == 2 else [x]
  alone = [t.detach()[:1].clone().requires_grad_() for t in parts]
  cb = [ops16.to_cb8(t, msdt) for t in alone]
  if in_mode == 2:
    y1 = ops16.conv_block16(cb[0], wp, bp, geom, MS_BN_EVAL, x2=cb[1], in_mode=2, **kw)
  else:
    y1 = ops16.conv_block16(cb[0], wp, bp, geom, MS_BN_EVAL, in_mode=in_mode, **kw)
  y1 = y1 if out_f32 else ops16.from_cb8(y1, cout * groups)
  (y1 * dy_cpu[:1].to(DEV)).sum().backward()
  assert max(errs_of(y32[:1], y1)) <= figs['fwd'][1]
  for t4, t1 in zip(parts, alone):
    assert max(errs_of(t4.grad[:1], t1.grad)) <= figs['fwd'][1]
