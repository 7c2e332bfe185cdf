"""GPU: the 16-bit conv kernels against fp64 in every plan the planners can pick for the models' blocks and no other test shape
reaches -- the entries of tests/helpers/conv16_plan_table.py (tile, LDS-DMA ring depth, stage width, wait count and form, ring
refill, the weight gradient's tap form / slots / splits; every ragged edge of every kernel instance).

Each entry runs once in bf16 and once in fp16 through test_gpu_kernels16._case: forward, dx (dx and dx2 for the upsample-add
input), dw and dbias (dgamma / dbeta for BatchNorm blocks) against fp64 on the rounded operands, with _case's own bars -- bf16:
bars='legacy'; fp16: bars='dtype' (3 x the fp64 rounding model of helpers/round16_model.py; tests/test_round16_model_cpu.py holds
every entry and seed to the conditions under which that bar separates the types); the LeakyReLU slopes follow the device's signs
(mask='device').

The launch labels of the run must name what tests/helpers/conv16_plan_host.cpp -- the same planner, built for the host -- planned
for the shape: template arguments, tile, tw, ring depth and wait count of conv16_kernel in both directions, taps / input form /
tiles / tw / splits of the weight gradient.  A device library whose planner disagrees with the host build fails here.  The label
is the host's view: its `w` is formed by launch_conv16 from the plan, not by the kernel, so it pins the plan the device takes and
says nothing about the wait the K loop really performs.

That wait is what the second run is for.  Where a plan of the entry waits with the run-time count, or refills its ring inside
the K loop, forward + backward run a second time while a side stream copies 1 GiB buffers back and forth (the `load` fixture,
sized from the time the first run took), and every tensor of the second run must be bitwise equal to the first.  The kernels
reduce in a fixed order, so correct code repeats bitwise whatever runs beside it; a stage read before it has landed does not.
The load matters: alone on the device these shapes are cache-resident and a stage's loads land before the stage is read even when
the K loop does not wait for them at all, so an unloaded repeat (and every bar) stays green under a wrong wait count.

Tried on scratch builds (value-only mutations of the K loop's run-time branch, none committed), each library loaded through
MS_LIB_PATH and the whole file run once per library:
  unmutated                                                           72 passed
  the branch computes ring slot 0 always (positive control)           red: forward and dx of the run-time entries, far over the bars
  wait one stage short, `wait_vmcnt(wcount + per_stage)`              1 red: d_conv1_b33_256 bf16, dx differs between the two runs
                                                                      (max 25); without the load: 72 passed
  never waits for a stage, `wait_vmcnt(63)` (the tail still drains)   8 red: 1d_k4s2_8to104_g25_b33_31, d_conv1_b33_256, pse0_b33_256
                                                                      (dx differs) and 1d_k4s2_64to8_g25_b64_31 (LeakyReLU signs),
                                                                      both types; without the load: 72 passed
So the loaded repeat sees a short wait, but by timing: one case of eighteen for a wait that is one stage short.  It is a net for
this defect, not a proof of its absence; a count that is one stage short on a class with a deep ring can still pass.

Measured on one MI355X (`python -m pytest tests/test_gpu_conv16_plans.py -m gpu -s` prints every check of every case; the kernels
reduce in a fixed order, a rerun prints the same figures).  Per case and type: the check that comes closest to its bar, relative
to the reference's max-abs (l2: to its norm), the bar, and their ratio.  All 72 cases pass, every launch label equals the host
plan, and the 54 cases that repeat their run under the load (27 entries) are bitwise equal.  The file takes 15 s.

  case                               bf16: worst check  measured       bar  m/bar   fp16: worst check  measured       bar  m/bar
  ae0_b5_32x128                      fwd                4.97e-03  1.20e-02   0.41   fwd                5.91e-04  1.50e-03   0.39
  pse4_b16_4                         fwd                2.43e-03  1.20e-02   0.20   fwd                3.82e-04  1.15e-03   0.33
  cls_logits_b33_128                 dx l2              2.34e-03  1.00e-02   0.23   dx l2              2.93e-04  8.79e-04   0.33
  logits_g_b33_32_g8                 dx l2              2.35e-03  1.00e-02   0.23   dx l2              2.93e-04  8.79e-04   0.33
  1d_k4s2_8to104_g25_b33_31          fwd                2.91e-03  1.20e-02   0.24   fwd                3.59e-04  1.08e-03   0.33
  d_logits_b1_7                      dx l2              2.55e-03  1.00e-02   0.26   dx l2              2.63e-04  7.88e-04   0.33
  pse6_b49_8                         fwd                2.15e-03  1.20e-02   0.18   fwd                3.40e-04  1.02e-03   0.33
  d_conv1_b33_256                    fwd                2.95e-03  1.20e-02   0.25   fwd                3.93e-04  1.18e-03   0.33
  unet_up2_b16_2                     fwd                1.92e-03  1.20e-02   0.16   fwd                2.72e-04  8.17e-04   0.33
  unet_down2_b32_2                   fwd                2.45e-03  1.20e-02   0.20   fwd                2.32e-04  6.96e-04   0.33
  cls_logits_b33_256                 dx l2              2.35e-03  1.00e-02   0.23   dx l2              2.93e-04  8.80e-04   0.33
  ae0_b3_64x128                      fwd                4.74e-03  1.20e-02   0.39   fwd                5.74e-04  1.50e-03   0.38
  ae5_b1_8x32                        fwd                2.18e-03  1.20e-02   0.18   fwd                2.96e-04  8.87e-04   0.33
  2d_k3x8s1_8to8_b3_64x128           fwd                2.94e-03  1.20e-02   0.24   fwd                3.73e-04  1.12e-03   0.33
  logits_g_b5_32_g25                 dx l2              2.35e-03  1.00e-02   0.23   dx l2              2.94e-04  8.81e-04   0.33
  1d_k3s1_8to8_g25_b33_31            fwd                2.74e-03  1.20e-02   0.23   fwd                3.48e-04  1.04e-03   0.33
  logits_g_b33_32_g4                 dx l2              2.35e-03  1.00e-02   0.24   dx l2              2.93e-04  8.78e-04   0.33
  d_conv1_b48_256                    fwd                2.96e-03  1.20e-02   0.25   fwd                3.93e-04  1.18e-03   0.33
  pse0_b33_256                       fwd                4.61e-03  1.20e-02   0.38   fwd                5.47e-04  1.50e-03   0.36
  1d_k4s2_64to8_g8_b33_128           fwd                2.67e-03  1.20e-02   0.22   fwd                3.52e-04  1.06e-03   0.33
  1d_k3s1_104to8_g8_b33_63           fwd                3.19e-03  1.20e-02   0.27   fwd                4.34e-04  1.30e-03   0.33
  ae1_b5_32x128                      fwd                4.41e-03  1.20e-02   0.37   fwd                5.26e-04  1.50e-03   0.35
  1d_k3s1_266to1_b64_256_up2         fwd                2.98e-03  1.20e-02   0.25   fwd                3.90e-04  1.17e-03   0.33
  1d_k3s1_8to104_g8_b33_31_bcast     fwd                2.70e-03  1.20e-02   0.23   fwd                3.47e-04  1.04e-03   0.33
  2d_k4s2_256to8_b64_5x9             fwd                2.15e-03  1.20e-02   0.18   fwd                2.79e-04  8.36e-04   0.33
  2d_k3x8s1_8to8_b33_32x16           fwd                3.24e-03  1.20e-02   0.27   fwd                3.26e-04  9.79e-04   0.33
  1d_k4s2_64to8_g25_b64_31           fwd                3.42e-03  1.20e-02   0.29   fwd                3.58e-04  1.07e-03   0.33
  1d_k1s1_8to256_g25_b33_31          fwd                2.06e-03  1.20e-02   0.17   fwd                2.57e-04  7.72e-04   0.33
  unet_down128_b33_128               fwd                2.57e-03  1.20e-02   0.21   fwd                3.22e-04  9.65e-04   0.33
  2d_k3x8s1_8to256_b64_5x9           fwd                3.29e-03  1.20e-02   0.27   fwd                3.85e-04  1.16e-03   0.33
  1d_k3s1_8to128_b192_256_up2        fwd                3.13e-03  1.20e-02   0.26   dx                 3.66e-04  1.05e-03   0.35
  1d_k3s1_8to256_g25_b33_31_bcast    fwd                2.59e-03  1.20e-02   0.22   fwd                3.23e-04  9.69e-04   0.33
  2d_k3x8s1_64to8_b33_32x16          fwd                2.08e-03  1.20e-02   0.17   fwd                2.71e-04  8.13e-04   0.33
  2d_k3x8s1_8to64_b33_32x16          fwd                3.16e-03  1.20e-02   0.26   fwd                3.88e-04  1.17e-03   0.33
  2d_k3x8s1_8to128_b96_32x16         fwd                2.86e-03  1.20e-02   0.24   fwd                3.61e-04  1.08e-03   0.33
  2d_k3x8s1_256to8_b192_8x16         fwd                2.30e-03  1.20e-02   0.19   fwd                3.11e-04  9.34e-04   0.33
"""
import re
import time

import pytest
import torch

from helpers import round16_model as M
from helpers import conv16_plan_table as T
from test_conv16_plan_table_cpu import build_program, plan

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TYPES = {'bf16': (torch.bfloat16, 'bf16', 'legacy'), 'fp16': (torch.float16, 'f16', 'dtype')}

CONV_LABEL = re.compile(r'^conv16_kernel<(\w+),(\d+),(\d+),(\d+),(\d+),(\d+),(\d+)>\|conv_(fwd|dgrad)_cb8 .* tiles(\d+) tile(\d+)x(\d+) tw(\d+)'
                        r'(?: dma(\d+) w(\d+))?(?: \+\w+)?$')
WGRAD_LABEL = re.compile(r'^wgrad16_kernel<(\w+),(\d+),(\d+)>\|conv_wgrad_cb8 .* tiles(\d+) tw(\d+) splits(\d+)$')
WGRAD_C1_LABEL = re.compile(r'^wgrad16_c1_kernel<(\w+)>\|conv_wgrad_cb8 c1 .* tiles(\d+) splits(\d+)$')


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
  exe = build_program(str(tmp_path_factory.mktemp('conv16_plan') / 'conv16_plan_host'))
  assert exe is not None, 'the host planner needs a C++ compiler'
  return {c['id']: pl for c, pl in zip(T.ENTRIES, plan(exe, [T.geometry(c) for c in T.ENTRIES]))}


def _planned_conv(dtname, f):
  """What conv16_kernel's label shows of a plan: (type, KW, wm, wn, up2, dma, nwn, tiles, tile rows, tile pixels, tw, ring, wait)."""
  ring = (f['nstg'], f['wait']) if f['dma'] else (None, None)
  return (dtname, f['KW'], f['wm'], f['wn'], f['up2'], f['dma'], f['nwn'], f['tiles'], f['bm'], f['bn'], f['tw']) + ring


def check_labels(c, pl, dtname, labels):
  got = {'fwd': set(), 'dgrad': set()}
  for l in labels:
    m = CONV_LABEL.match(l)
    if m:
      g = m.groups()
      got[g[7]].add((g[0],) + tuple(int(v) for v in g[1:7]) + tuple(int(v) for v in g[8:12]) + tuple(None if v is None else int(v) for v in g[12:14]))
    else:
      assert not l.startswith('conv16_kernel<'), 'unparsed label: %s' % l
  for which in ('fwd', 'dgrad'):
    assert got[which] == {_planned_conv(dtname, pl[which])}, (c['id'], which, 'device', sorted(got[which], key=str), 'host', _planned_conv(dtname, pl[which]))
  w = pl['wgrad']
  if w['c1']:
    seen = {(m.group(1), int(m.group(2)), int(m.group(3))) for m in map(WGRAD_C1_LABEL.match, labels) if m}
    want = {(dtname, w['tiles'], w['splits'])}
  else:
    seen = {(m.group(1),) + tuple(int(v) for v in m.groups()[1:]) for m in map(WGRAD_LABEL.match, labels) if m}
    want = {(dtname, w['tp'], w['up2'], w['tiles'], w['tw'], w['splits'])}
  assert seen == want, (c['id'], 'wgrad', 'device', sorted(seen), 'host', sorted(want), sorted(set(labels)))
  if c['mode'] == 'BN_TRAIN':
    fused = any('+bnfused' in l for l in labels)
    assert fused == (c['bn_fused'] == 1), (c['id'], 'BatchNorm form', sorted(set(labels)))


def needs_repeat(pl):
  """A plan of the entry waits with the run-time count or refills its ring: classes where a race on a ring slot can live."""
  return any(pl[w]['dma'] and (pl[w]['form'] != 'lit' or pl[w]['refill']) for w in ('fwd', 'dgrad'))


def _run(c, dt, bars, keep, labels, check=True):
  from test_gpu_kernels16 import _case
  from test_gpu_dispatch_parity import _timed
  nd = c['nd']
  H, W = c['sp'] if nd == 2 else (1, c['sp'][0])
  with _timed(labels):
    return _case(nd, c['B'], c['cin'], c['cout'], c['groups'], c['k'], c['s'], c['p'], H, W, M.MODES[c['mode']], M.IN_MODES[c['in_mode']],
                 c['out_f32'], dt=dt, seed=c['seed'], slope=c['slope'], mask=c['mask'], ref_dev=DEV if c['ref_dev'] == 'device' else 'cpu',
                 keep=keep, bars=bars, two_launch=c['bn_fused'] == 0, check=check)


@pytest.fixture(scope='module')
def load():
  """load(seconds): queue about that long a run of 1 GiB device-to-device copies on a side stream -- memory traffic beside the case's
  kernels that empties the caches under them and lengthens their loads."""
  src = torch.empty(1 << 28, dtype=torch.float32, device=DEV).normal_()
  dst = torch.empty_like(src)
  side = torch.cuda.Stream()
  t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  with torch.cuda.stream(side):
    dst.copy_(src)
    t0.record()
    for _ in range(8):
      dst.copy_(src)
    t1.record()
  torch.cuda.synchronize()
  per_copy = t0.elapsed_time(t1) / 8e3

  def start(seconds):
    with torch.cuda.stream(side):
      for _ in range(min(LOAD_MAX_COPIES, int(seconds / per_copy) + 1)):
        dst.copy_(src)
  yield start
  torch.cuda.synchronize()
  del src, dst


LOAD_MAX_COPIES = 6000      # (a few seconds of copies at the most)


@pytest.mark.parametrize('prec', list(TYPES))
@pytest.mark.parametrize('c', T.ENTRIES, ids=[c['id'] for c in T.ENTRIES])
def test_plan_class_matches_fp64(c, prec, plans, load):
  dt, dtname, bars = TYPES[prec]
  pl = plans[c['id']]
  first, labels = {}, []
  torch.cuda.synchronize()
  began = time.perf_counter()
  measured = _run(c, dt, bars, first, labels)
  torch.cuda.synchronize()
  took = time.perf_counter() - began
  for k, (v, bar) in measured.items():
    print('  %-34s %-5s %-32s %9.2e %9.2e  %4.2f' % (c['id'], prec, k, v, bar, v / bar if bar else 0.0))
  bad = {k: v for k, v in measured.items() if not v[0] <= v[1]}
  assert not bad, bad
  check_labels(c, pl, dtname, labels)
  if needs_repeat(pl):
    second = {}
    load(1.25 * took)        # the copies outlast the run: its kernels start somewhere inside the time the first run took
    _run(c, dt, bars, second, [], check=False)
    torch.cuda.synchronize()
    for k, v in first.items():
      if v is not None:
        assert torch.equal(v, second[k]), (c['id'], k, 'differs between two runs', (v.float() - second[k].float()).abs().max().item())
