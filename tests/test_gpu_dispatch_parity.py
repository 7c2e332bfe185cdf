"""GPU: every conv-block dispatch path of tests/helpers/dispatch_table.py at the size that reaches it -- the production sizes
(B = 32; 1024 for the fp16 inference blocks) and the BatchNorm / activation thresholds -- against fp64.

Each case runs its forward and backward pass under the launch timing, asserts that the launches it exists for took place (a
case that drifts to another kernel fails and names the labels it got), and compares with fp64:
  fp32 / bf16x6   the oracle's ConvNormRelu (or conv) in float64, the bars of test_gpu_kernels._conv_block_case: forward
                  <= 2e-5, dx / dw / dgamma / dbeta <= 1e-4 relative to the tensor's max-abs, running statistics <= 1e-5,
                  the conv bias gradient (true value 0 before BatchNorm) ~ 0.
  bf16 / fp16     test_gpu_kernels16._case: fp64 on the same 16-bit-rounded operands, its bars (returned with the values);
                  bars='dtype': bf16 keeps the bars it had, the fp16 entries get the fp16-sized ones.

LeakyReLU kinks: at B = 32 some pre-activation is almost always within fp32 rounding of 0 and takes the other slope than in
fp64.  The fp64 reference therefore takes its slope mask from the sign of the device output, and the test asserts that the
elements where that sign and the fp64 sign differ are few and all within rounding of 0 -- no bar is loosened for them.

The references run on the CPU; the 2-D blocks and the large grouped 1-D blocks run torch float64 on the device (float64
arithmetic either way; the CPU would take minutes for them at B = 32)."""
import contextlib
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

from oracle import mixstage_oracle as O
from helpers.dispatch_table import TABLE

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MODES = {'BARE': 0, 'LRELU': 1, 'BN_TRAIN': 2, 'BN_EVAL': 3}
IN_MODES = {'plain': 0, 'bcast': 1, 'up2': 2}
KINK_MAX = 8                  # elements per tensor whose LeakyReLU slope may differ from fp64 (each within rounding of 0)


def rel_err(a, b):
  a, b = a.detach().double().cpu(), b.detach().double().cpu()
  assert a.shape == b.shape, (a.shape, b.shape)
  return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@contextlib.contextmanager
def _knobs(e):
  from mix_stage_amd import _lib
  L = _lib.lib()
  old = {}
  try:
    for name, v in e['knobs'].items():
      old[name] = getattr(L, name)(v)
    if e['prec'] == 'bf16x6':
      L.ms_set_precision(1)
    yield
  finally:
    L.ms_set_precision(0)
    for name, v in old.items():
      getattr(L, name)(v)


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


def _nd_kernel(e):
  k, s, p = e['k'], e['s'], e['p']
  if e['nd'] == 1:
    return k, s, p
  two = lambda v: tuple(v) if isinstance(v, tuple) else (v, v)
  return two(k), two(s), two(p)


def _deterministic(mod, prefix):
  sd = O.deterministic_state({prefix + kk: v for kk, v in mod.state_dict().items()})
  mod.load_state_dict({kk[len(prefix):]: v for kk, v in sd.items()})
  return mod


def _ref_device(e):
  """float64 reference on the CPU, or on the device for 2-D blocks and for 1-D blocks above ~0.5 GMAC."""
  k, _, _ = _nd_kernel(e)
  khw = k[0] * k[1] if isinstance(k, tuple) else k
  ow = 1
  for v in e['sp']:
    ow *= v
  macs = e['B'] * (2 if e['pair'] else 1) * e['groups'] * e['cout'] * e['cin'] * khw * ow
  return DEV if (e['nd'] == 2 or macs > 5e8) else 'cpu'


def _block_saved(y):
  """The `save` vector the conv block's autograd node keeps for its backward pass (readable until that pass has run).  (y_raw is
  no result to compare: the in-launch BatchNorm forms write it only for the channels whose map does not invert from y.)"""
  fn = y.grad_fn
  if fn is None or type(fn).__name__ not in ('_ConvBlockFnBackward', '_ConvBlock16FnBackward'):
    return None
  return fn.saved_tensors[6]


def _run_fp32(e, labels, keep=None):
  """fp32 / bf16x6 block: device output and gradients under timing, fp64 reference with the device's LeakyReLU mask.
  keep: a dict that receives the device tensors of the run (output, every gradient, running statistics, save)."""
  import mix_stage_amd as A
  from mix_stage_amd import ops
  from mix_stage_amd.layers import bare_conv
  nd, g, mode = e['nd'], e['groups'], e['mode']
  k, s, p = _nd_kernel(e)
  B = e['B'] * (2 if e['pair'] else 1)
  gen = torch.Generator().manual_seed(zlib.crc32(e['id'].encode()) % 1000)
  rdev = _ref_device(e)
  bn = mode in ('BN_TRAIN', 'BN_EVAL')
  typ = '%dd' % nd
  if bn:
    kw = dict(type=typ, leaky=True, kernel_size=k, stride=s, padding=p, groups=g)
    ref = _deterministic(O.ConvNormRelu(e['cin'], e['cout'], **kw), 'blk.').double().to(rdev)
    hip = _deterministic(A.ConvNormRelu(e['cin'], e['cout'], **kw), 'blk.').to(DEV)
    ref.train(mode == 'BN_TRAIN'); hip.train(mode == 'BN_TRAIN')
    ref_conv, hip_conv = ref.conv, hip.conv
  else:
    cls = torch.nn.Conv1d if nd == 1 else torch.nn.Conv2d
    hip_conv = _deterministic(cls(e['cin'] * g, e['cout'] * g, k, s, padding=p, groups=g), 'c.').to(DEV)
    ref_conv = _deterministic(cls(e['cin'] * g, e['cout'] * g, k, s, padding=p, groups=g), 'c.').double().to(rdev)
  sp = e['sp']
  cin_tot = e['cin'] * (1 if e['in_mode'] == 'bcast' else g)
  if e['in_mode'] == 'up2':
    xs = [torch.randn(B, cin_tot, sp[0] // 2, generator=gen), torch.randn(B, cin_tot, *sp, generator=gen)]
  else:
    xs = [torch.randn(B, cin_tot, *sp, generator=gen)]
  if e['pair']:
    # the two passes of the D-step differ in their statistics
    xs = [torch.cat([x[:B // 2], x[B // 2:] * 1.6 + 0.3]) for x in xs]
  xh = [x.to(DEV).requires_grad_() for x in xs]

  # ---- device
  with _timed(labels):
    ctx = ops.stat_pair() if e['pair'] else contextlib.nullcontext()
    with ctx:
      if not bn:
        y = bare_conv(hip_conv, xh[0], lrelu_slope=0.2 if mode == 'LRELU' else None)
      elif e['in_mode'] == 'up2':
        y = hip.forward_upsample_add(xh[0], xh[1])
      elif e['in_mode'] == 'bcast':
        y = hip.forward_broadcast(xh[0])
      else:
        y = hip(xh[0])
    gy = torch.randn(y.shape, generator=gen)
    if keep is not None:
      keep['y'] = y.detach()
      keep['save'] = _block_saved(y)
    if mode != 'BN_EVAL':
      y.backward(gy.to(DEV))
  if keep is not None:
    for i, x in enumerate(xh):
      keep['dx%d' % i] = x.grad
    keep['dw'], keep['dbias'] = hip_conv.weight.grad, hip_conv.bias.grad
    if bn:
      keep['dgamma'], keep['dbeta'] = hip.norm.weight.grad, hip.norm.bias.grad
      keep['running_mean'], keep['running_var'] = hip.norm.running_mean.detach(), hip.norm.running_var.detach()

  # ---- fp64 reference: conv (+ BatchNorm, per half for the paired pass) in float64, then the activation with the device's mask
  x64 = [x.double().to(rdev).requires_grad_() for x in xs]
  if e['in_mode'] == 'up2':
    xin = F.interpolate(x64[0], scale_factor=2, mode='nearest') + x64[1]
  elif e['in_mode'] == 'bcast':
    xin = torch.cat([x64[0]] * g, dim=1)
  else:
    xin = x64[0]
  if bn and e['pair']:
    h = B // 2
    z = torch.cat([ref.norm(ref_conv(xin[:h])), ref.norm(ref_conv(xin[h:]))])
  elif bn:
    z = ref.norm(ref_conv(xin))
  else:
    z = ref_conv(xin)
  errs = {}
  if mode == 'BARE':
    y_ref = z
  else:
    pos = (y.detach() > 0).to(rdev)
    flip = pos != (z.detach() > 0)
    zmax = z.detach().abs().max().item()
    kink = z.detach()[flip].abs().max().item() if flip.any() else 0.0
    errs['kinks (count)'] = (int(flip.sum().item()), KINK_MAX)
    errs['|z| at a kink'] = (kink / zmax, 2e-5)
    y_ref = torch.where(pos, z, 0.2 * z)
  errs['fwd'] = (rel_err(y, y_ref), 2e-5)
  if mode != 'BN_EVAL':
    y_ref.backward(gy.double().to(rdev))
    if e['in_mode'] == 'up2':
      errs['d(a)'] = (rel_err(xh[0].grad, x64[0].grad), 1e-4)
      errs['d(res)'] = (rel_err(xh[1].grad, x64[1].grad), 1e-4)
    else:
      errs['dx'] = (rel_err(xh[0].grad, x64[0].grad), 1e-4)
    errs['dw'] = (rel_err(hip_conv.weight.grad, ref_conv.weight.grad), 1e-4)
    if bn:
      errs['dgamma'] = (rel_err(hip.norm.weight.grad, ref.norm.weight.grad), 1e-4)
      errs['dbeta'] = (rel_err(hip.norm.bias.grad, ref.norm.bias.grad), 1e-4)
      scale = ref_conv.weight.grad.abs().max().item()
      errs['dbias(~0)'] = (hip_conv.bias.grad.abs().max().item(), 1e-4 * max(scale, 1.0))
    else:
      errs['dbias'] = (rel_err(hip_conv.bias.grad, ref_conv.bias.grad), 1e-4)
  if bn:
    errs['running_mean'] = (rel_err(hip.norm.running_mean, ref.norm.running_mean), 1e-5)
    errs['running_var'] = (rel_err(hip.norm.running_var, ref.norm.running_var), 1e-5)
  return errs


def _run_16(e, labels, keep=None):
  """16-bit block: test_gpu_kernels16._case (fp64 on the rounded operands, its bars) under timing.  The LeakyReLU slopes of the
  reference follow the device output's sign (_case mask='device': only elements within one 16-bit rounding of 0 may differ, and
  few of them); eval blocks have no backward pass and compare exact math."""
  from test_gpu_kernels16 import _case
  nd = e['nd']
  H, W = (e['sp'] if nd == 2 else (1, e['sp'][0]))
  dt = torch.bfloat16 if e['prec'] == 'bf16' else torch.float16
  assert not e['pair']
  with _timed(labels):
    measured = _case(nd, e['B'], e['cin'], e['cout'], e['groups'], e['k'], e['s'], e['p'], H, W, MODES[e['mode']],
                     IN_MODES[e['in_mode']], e['out_f32'], dt=dt, seed=zlib.crc32(e['id'].encode()) % 1000,
                     mask='device' if e['mode'] in ('BN_TRAIN', 'LRELU') else 'exact', ref_dev=_ref_device(e),
                     bn_folded=e['folded'], keep=keep, bars='dtype')
  return measured


def run_entry(e, keep=None):
  """-> (labels, {check: (measured, bar)}) for one table entry; keep: a dict that receives the run's device tensors."""
  labels = []
  with _knobs(e):
    errs = (_run_16 if e['prec'] in ('bf16', 'fp16') else _run_fp32)(e, labels, keep)
  return labels, errs


def check_labels(e, labels):
  missing = [rx for rx in e['expect'] if not any(re.search(rx, l) for l in labels)]
  present = [(rx, l) for rx in e['forbid'] for l in labels if re.search(rx, l)]
  assert not missing and not present, ('%s took another path: expected %s, forbidden %s; launches: %s'
                                       % (e['id'], missing, present, sorted(set(labels))))


@pytest.mark.parametrize('e', TABLE, ids=[e['id'] for e in TABLE])
def test_dispatch_path_matches_fp64(e):
  labels, errs = run_entry(e)
  check_labels(e, labels)
  bad = {kk: v for kk, v in errs.items() if not v[0] <= v[1]}
  assert not bad, 'errors (value, bar): %s | all: %s' % (bad, {kk: '%.2e' % v[0] for kk, v in errs.items()})
