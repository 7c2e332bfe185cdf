"""GPU: the learning rate as a device word.  C-ABI level: ms_adam_step_segmented_lr / _scaled_lr against their by-value twins bit
for bit while the word moves, against float64, and a bad word as a bad step.  Trainer level: captured steps follow the schedule
(graph == eager == the old kernels with lr assigned by hand), fp16 with dynamic loss scaling, three epochs against the float64
oracle with torch's ExponentialLR, and the trainer's surface."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from oracle import mixstage_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BETAS, EPS, MAX_NORM = (0.9, 0.999), 1e-8, 1.0
FLOOR = 2.0 * 2.0 ** -24

# one flat buffer, 5 segments: one never used (-1), one that starts at step 2; and 2^20 + 64 elements for the element pass's grid
SMALL = ((64, 128, 64, 4096, 192), (1, -1, 2, 1, 1))
BIG = ((1 << 19, 64, 1 << 19), (1, -1, 2))
CASES = [pytest.param(SMALL, 0, id='5seg_vector'), pytest.param(SMALL, 1, id='5seg_scalar_offset_4_bytes'),
         pytest.param(BIG, 0, id='2p20_plus_64_vector'), pytest.param(BIG, 1, id='2p20_plus_64_scalar_offset_4_bytes')]
LRS = (1e-4, 9.9e-5, 9.9e-5, 3.3e-7)


def f32(v):
  return float(np.float32(v))


def _hip(M, S, dtype=None):
  import mix_stage_amd as A
  from test_gpu_model import build_hip_gan
  model = build_hip_gan(M, S)
  if dtype is not None:
    A.set_compute_dtype(model, dtype)
  return model


def _ls_words(scale, good=0, skips=0, last=0):
  w = torch.zeros(8, dtype=torch.int32)
  w.view(torch.float32)[0] = scale
  w.view(torch.float32)[1] = 1.0 / scale
  w[2], w[3], w[4] = good, skips, last
  return w.to(DEV)


class _Flat:
  """p, g, m, v, norm and the segment tables of a flat buffer, optionally on views offset by one float (the scalar path of the
  element pass); `lr_word` is the device word of the _lr entry points."""

  def __init__(self, case, offset=0, seed=0, init=None):
    from mix_stage_amd import ops
    sizes, first = case
    n = self.n = sum(sizes)
    assert all(s % 64 == 0 for s in sizes)
    self.bufs = [torch.zeros(n + 4 * offset, dtype=torch.float32, device=DEV) for _ in range(4)]
    self.p, self.g, self.m, self.v = [b[offset:offset + n] for b in self.bufs]
    assert all(t.data_ptr() % 16 == 4 * offset for t in (self.p, self.g, self.m, self.v))
    if init is None:
      self.p.copy_(torch.randn(n, generator=torch.Generator().manual_seed(seed)))
    else:
      for t, src in zip((self.p, self.m, self.v), init):
        t.copy_(src)
    self.seg_of_chunk = torch.cat([torch.full((s // 64,), i, dtype=torch.int32) for i, s in enumerate(sizes)]).to(DEV)
    self.seg_first = torch.tensor(first, dtype=torch.int32, device=DEV)
    self.seg_scratch = torch.zeros(2 * len(sizes), dtype=torch.float32, device=DEV)
    self.norm = torch.zeros(1, dtype=torch.float32, device=DEV)
    self.partials = torch.zeros(ops.lib().ms_reduce_partials_count(n), dtype=torch.float32, device=DEV)
    self.step_state = torch.zeros(4, dtype=torch.int32, device=DEV)
    self.lr_word = torch.zeros(1, dtype=torch.float32, device=DEV)

  def step(self, g, lr, by_value, ls=None, rule=None, norm=None, raw_word=False):
    """by_value: the existing entry points with `lr` as a float; else the word is written (ops.write_floats, or filled by hand
    with raw_word) and the _lr entry points read it."""
    from mix_stage_amd import ops
    self.g.copy_(g)
    if norm is None:
      ops.grad_norm(self.g, self.norm, self.partials)
    else:
      self.norm.fill_(norm)
    if not by_value:
      if raw_word:
        self.lr_word.fill_(lr)
      else:
        ops.write_floats(self.lr_word, [lr])
    args = (self.p, self.g, self.m, self.v, self.norm, MAX_NORM, lr if by_value else self.lr_word, BETAS[0], BETAS[1], EPS,
            self.step_state, self.seg_of_chunk, self.seg_first, self.seg_scratch)
    if ls is None:
      (ops.adam_step_segmented if by_value else ops.adam_step_segmented_lr)(*args)
    else:
      (ops.adam_step_segmented_scaled if by_value else ops.adam_step_segmented_scaled_lr)(*args, ls, rule.growth_interval, rule.min,
                                                                                           rule.max, None)

  def words(self):
    return dict(p=self.p, m=self.m, v=self.v, step_state=self.step_state, seg_scratch=self.seg_scratch)


def _grads(case, steps, seed=5):
  sizes, first = case
  n, gen, out = sum(sizes), torch.Generator().manual_seed(seed), []
  for _ in range(steps):
    g = torch.randn(n, generator=gen) * 10.0 ** (-4.0 * torch.rand(n, generator=gen))
    lo = 0
    for s, f in zip(sizes, first):
      if f < 0:
        g[lo:lo + s] = 0.0                              # the segment that never receives a gradient
      lo += s
    out.append(g.to(DEV))
  return out


# ------------------------------------------------------------------------------------------------ C-ABI level
@pytest.mark.parametrize('case,offset', CASES)
def test_lr_word_equals_lr_by_value_bit_for_bit_over_four_steps(case, offset):
  grads = _grads(case, len(LRS))
  ref, got = _Flat(case, offset), _Flat(case, offset)
  p0 = ref.p.clone()
  for g, lr in zip(grads, LRS):
    ref.step(g, lr, by_value=True)
    got.step(g, lr, by_value=False)
    for name, t in ref.words().items():
      assert torch.equal(t, got.words()[name]), (name, lr)
    assert torch.equal(ref.norm, got.norm)
  assert ref.step_state.tolist() == [4, ref.step_state.tolist()[1], 0, 0] and not torch.equal(ref.p, p0)
  assert float(got.lr_word) == f32(LRS[-1])
  sc = got.seg_scratch.cpu().reshape(-1, 2)
  idle = [i for i, f in enumerate(case[1]) if f < 0]
  assert all(sc[i].tolist() == [0.0, 0.0] for i in idle) and all(sc[i, 1] > 0 for i in range(len(case[1])) if i not in idle)
  # the last step's size really is the last word's: lr / (1 - beta1^t) of the float32 arguments, rounded once; t = 4 for a segment
  # that started at step 1
  live = case[1].index(1)
  assert abs(float(sc[live, 0]) - f32(LRS[-1]) / (1.0 - f32(BETAS[0]) ** 4)) <= 2.0 ** -23 * float(sc[live, 0])
  for b in got.bufs:                                    # nothing in front of an offset view was touched
    assert offset == 0 or float(b[0]) == 0.0


@pytest.mark.parametrize('S', [1.0, 2.0 ** 16], ids=['S1', 'S65536'])
@pytest.mark.parametrize('case,offset', CASES)
def test_scaled_lr_word_equals_scaled_lr_by_value_bit_for_bit(case, offset, S):
  from mix_stage_amd.loss_scale import LossScaleRule
  grads = _grads(case, len(LRS))
  rule = LossScaleRule(S)
  ref, got = _Flat(case, offset), _Flat(case, offset)
  ls_ref, ls_got = _ls_words(S), _ls_words(S)
  for g, lr in zip(grads, LRS):
    ref.step(g * S, lr, by_value=True, ls=ls_ref, rule=rule)
    got.step(g * S, lr, by_value=False, ls=ls_got, rule=rule)
    for name, t in ref.words().items():
      assert torch.equal(t, got.words()[name]), (name, lr, S)
    assert torch.equal(ref.norm, got.norm) and torch.equal(ls_ref, ls_got), (lr, S)      # the written-back (true) norm, the scale state
  assert got.step_state.tolist()[0] == 4 and got.step_state.tolist()[2:] == [0, 0]
  assert torch.equal(ls_got.cpu(), _ls_words(S, good=4).cpu())
  # ... and the scaled twin on S g is the plain twin on g (the property the by-value pair already has)
  plain = _Flat(case, offset)
  for g, lr in zip(grads, LRS):
    plain.step(g, lr, by_value=False)
  for name in ('p', 'm', 'v'):
    assert torch.equal(plain.words()[name], got.words()[name]), (name, S)


def _two_metrics(got, ref):
  got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
  assert got.shape == ref.shape and bool(torch.isfinite(got).all())
  d = (got - ref).abs()
  rms = ref.pow(2).mean().sqrt()
  return (d.max() / (ref.abs().max() + 1e-30)).item(), (d / (ref.abs() + rms + 1e-30)).max().item()


def _adam_reference(dtype, p0, m0, v0, grads, norms32, lrs, first):
  """torch.optim.Adam with clip_grad_norm_ folded in, one step count per element (t = step - first + 1; first = -1 or in the
  future: skipped) and one learning rate per step, which enters as its float32 value (it crosses the ABI as a float)."""
  b1, b2, eps = f32(BETAS[0]), f32(BETAS[1]), f32(EPS)
  p, m, v = p0.to(dtype).clone(), m0.to(dtype).clone(), v0.to(dtype).clone()
  for s, (g, nrm, lr) in enumerate(zip(grads, norms32, lrs), start=1):
    coef = torch.clamp(torch.tensor(f32(MAX_NORM), dtype=dtype) / (torch.tensor(nrm, dtype=dtype) + torch.tensor(f32(1e-6), dtype=dtype)), max=1.0)
    act = (first >= 1) & (first <= s)
    t = (s - first + 1).clamp(min=1).double()
    step_size = (f32(lr) / (1.0 - b1 ** t)).to(dtype)              # (python-double arithmetic cast once, as torch.optim.Adam does)
    bc2s = (1.0 - b2 ** t).sqrt().to(dtype)
    gi = g.to(dtype) * coef
    mn = m + (1.0 - b1) * (gi - m)
    vn = b2 * v + (1.0 - b2) * gi * gi
    pn = p - step_size * (mn / (vn.sqrt() / bc2s + eps))
    p, m, v = torch.where(act, pn, p), torch.where(act, mn, m), torch.where(act, vn, v)
  return p, m, v


@pytest.mark.parametrize('case,offset', CASES)
def test_three_steps_against_float64(case, offset):
  """DESIGN section 2's bar: the device's error against the float64 formula is at most 4 x the error of a float32 host evaluation
  of the same formula (floored at 2 * 2^-24), as a maximum over the tensor and element by element.  lr differs per step."""
  sizes, first_seg = case
  n = sum(sizes)
  gen = torch.Generator().manual_seed(31)
  p0 = torch.randn(n, generator=gen) * 0.1
  p0[::7] *= 1e-4
  m0 = torch.randn(n, generator=gen) * 0.01
  v0 = torch.rand(n, generator=gen) * 1e-4
  lrs = (1e-4, 9.9e-5, 3.3e-7)
  first = torch.tensor(first_seg).repeat_interleave(torch.tensor(sizes))
  grads = []
  for i in range(3):
    g = torch.randn(n, generator=gen) * 0.02 * torch.exp(torch.randn(n, generator=gen))
    if i == 1:
      g *= 0.5 / float(g.double().norm())               # one step under the clip threshold, two above it
    grads.append(g)
  fl = _Flat(case, offset, init=(p0, m0, v0))
  norms32 = []
  for g, lr in zip(grads, lrs):
    fl.step(g.to(DEV), lr, by_value=False)
    norms32.append(float(fl.norm))                      # the norm the device clipped with: the reference takes it as its input
  assert norms32[0] > MAX_NORM > norms32[1] and fl.step_state.tolist()[2:] == [0, 0]
  ref = _adam_reference(torch.float64, p0, m0, v0, grads, norms32, lrs, first)
  y32 = _adam_reference(torch.float32, p0, m0, v0, grads, norms32, lrs, first)
  rows = []
  for name, got, r, y in zip('pmv', (fl.p, fl.m, fl.v), ref, y32):
    mx, el = _two_metrics(got, r)
    ymx, yel = _two_metrics(y, r)
    rows += [(name + ' max', mx, 4 * max(ymx, FLOOR), ymx), (name + ' elem', el, 4 * max(yel, FLOOR), yel)]
  for name, val, bar, yard in rows:
    print('LR64 %-8s yardstick %.3e device %.3e bar %.3e' % (name, yard, val, bar))
  bad = [(nm, val, bar) for nm, val, bar, _ in rows if not val <= bar]
  assert not bad, bad
  never = ~((first >= 1) & (first <= 3))
  assert bool(never.any())
  for got, init in ((fl.p, p0), (fl.m, m0), (fl.v, v0)):
    assert torch.equal(got.cpu()[never], init[never])


@pytest.mark.parametrize('word', [float('nan'), float('inf'), 0.0, -1e-4], ids=['nan', 'inf', 'zero', 'negative'])
@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'scaled'])
def test_a_bad_lr_word_is_a_bad_step(word, scaled):
  """The word is written by hand; no launch faults or waits.  The step is refused as a non-finite gradient norm is refused: p, m,
  v bit-unchanged, word 2 set, word 3 counted, the clock advanced -- and the loss scale left alone.  A good word afterwards steps."""
  from mix_stage_amd.loss_scale import LossScaleRule
  grads = _grads(SMALL, 3)
  fl = _Flat(SMALL)
  rule = LossScaleRule(dict(init=8, growth_interval=0, min=2, max=8)) if scaled else None
  ls = _ls_words(8.0) if scaled else None
  k = 8.0 if scaled else 1.0
  fl.step(grads[0] * k, 1e-4, by_value=False, ls=ls, rule=rule)
  assert fl.step_state.tolist()[0] == 1 and fl.step_state.tolist()[2:] == [0, 0]
  before = [t.clone() for t in (fl.p, fl.m, fl.v)]
  ls_before = ls.clone() if scaled else None
  fl.step(grads[1] * k, word, by_value=False, ls=ls, rule=rule, raw_word=True)
  assert all(torch.equal(a, b) for a, b in zip(before, (fl.p, fl.m, fl.v)))
  assert fl.step_state.tolist()[0] == 2 and fl.step_state.tolist()[2:] == [1, 1]
  if scaled:
    assert torch.equal(ls, ls_before)                   # scale, its counters and the overflow-skip flag: as they were
  fl.step(grads[2] * k, 1e-4, by_value=False, ls=ls, rule=rule)
  assert fl.step_state.tolist()[0] == 3 and fl.step_state.tolist()[2:] == [0, 1]
  assert not torch.equal(fl.p, before[0]) and bool(torch.isfinite(fl.p).all())


def test_a_null_lr_word_is_an_error_and_launches_nothing():
  from mix_stage_amd import ops
  fl = _Flat(SMALL)
  fl.g.copy_(_grads(SMALL, 1)[0])
  fl.norm.fill_(1.0)
  ls = _ls_words(8.0)
  L = ops.lib()
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  head = (P(fl.p), P(fl.g), P(fl.m), P(fl.v), fl.n, P(fl.norm), MAX_NORM)
  tail = (BETAS[0], BETAS[1], EPS, P(fl.step_state), P(fl.seg_of_chunk), P(fl.seg_first), P(fl.seg_scratch), len(SMALL[0]))
  before = [t.clone() for t in (fl.p, fl.m, fl.v, fl.step_state, fl.seg_scratch)]
  ops.timing_enable(True)
  try:
    assert L.ms_adam_step_segmented_lr(*head, None, *tail, stream) != 0
    assert L.ms_adam_step_segmented_scaled_lr(*head, None, *tail, P(ls), 0, 2.0, 8.0, None, 0, stream) != 0
    torch.cuda.synchronize()
    assert [r['label'] for r in ops.timing_report()] == []
    assert L.ms_adam_step_segmented_lr(*head, P(fl.lr_word.fill_(1e-4)), *tail, stream) == 0       # the same arguments with a word
    torch.cuda.synchronize()
    assert [(r['label'], r['count']) for r in ops.timing_report()] == [('ew|ew_adam_step_segmented', 1)]
  finally:
    ops.timing_enable(False)
  assert fl.step_state.tolist()[0] == 1 and not torch.equal(fl.p, before[0])
  with pytest.raises(TypeError):
    ops.adam_step_segmented_lr(fl.p, fl.g, fl.m, fl.v, fl.norm, MAX_NORM, 1e-4, BETAS[0], BETAS[1], EPS, fl.step_state,
                               fl.seg_of_chunk, fl.seg_first, fl.seg_scratch)


def test_without_a_norm_lr_by_value_leaves_the_health_words_and_the_lr_word_form_writes_them():
  """norm = NULL at the C ABI (no clipping: the coefficient is 1), from preset health words [2] = a, [3] = 7.  With lr by value the
  prep kernel does not write words 2 and 3 at all -- a flag that is set stays set and the element pass returns on it; with lr from
  the word it always writes them, from the word alone."""
  from mix_stage_amd import ops
  L = ops.lib()
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  g = _grads(SMALL, 1)[0]
  sizes, first = SMALL
  act = (torch.tensor(first).repeat_interleave(torch.tensor(sizes)) == 1).to(DEV)      # step 1: -1 never starts, 2 is still ahead

  def run(a, lr=None, word=None, norm=None):
    fl = _Flat(SMALL)
    fl.g.copy_(g)
    fl.step_state.copy_(torch.tensor([0, 0, a, 7], dtype=torch.int32))
    before = [t.clone() for t in (fl.p, fl.m, fl.v)]
    if norm is not None:
      fl.norm.fill_(norm)
    head = (P(fl.p), P(fl.g), P(fl.m), P(fl.v), fl.n, P(fl.norm) if norm is not None else None, MAX_NORM)
    tail = (BETAS[0], BETAS[1], EPS, P(fl.step_state), P(fl.seg_of_chunk), P(fl.seg_first), P(fl.seg_scratch), len(sizes))
    if word is None:
      assert L.ms_adam_step_segmented(*head, lr, *tail, stream) == 0
    else:
      assert L.ms_adam_step_segmented_lr(*head, P(fl.lr_word.fill_(word)), *tail, stream) == 0
    torch.cuda.synchronize()
    state = fl.step_state.tolist()
    assert state[0] == 1 and float(fl.step_state.view(torch.float32)[1]) == 1.0          # the clock advanced, nothing is clipped
    moved = not torch.equal(fl.p, before[0])
    if not moved:
      assert all(torch.equal(x, y) for x, y in zip(before, (fl.p, fl.m, fl.v)))
    else:
      assert bool((fl.p != before[0])[act].any()) and torch.equal(fl.p[~act], before[0][~act])
    return fl, state[2:], moved

  fl, words, moved = run(0, lr=1e-4)
  assert words == [0, 7] and moved
  ref, ref_words, _ = run(0, lr=1e-4, norm=1e-30)       # a norm so small that the coefficient clamps to 1: the same step
  assert ref_words == [0, 7]
  for name in ('p', 'm', 'v', 'seg_scratch'):
    assert torch.equal(fl.words()[name], ref.words()[name]), name
  assert run(1, lr=1e-4)[1:] == ([1, 7], False)
  assert run(1, word=1e-4)[1:] == ([0, 7], True)
  assert run(0, word=0.0)[1:] == ([1, 8], False)


# ------------------------------------------------------------------------------------------------ trainer level
M_ = S_ = 2
GAMMA = 0.5
KINDS12 = ['G', 'D'] * 6


@functools.lru_cache(maxsize=None)
def _batch():
  return tuple(t.to(DEV) for t in O.synthetic_batch(4, M=M_, S=S_, seed=11))


def _hand_lrs(lr0, gamma, epochs):
  out, lr = [lr0], lr0
  for _ in range(epochs):
    lr = lr * gamma
    out.append(lr)
  return out


def _run(precision, mode, steps=12, loss_scale=None, kinds=None):
  """mode: 'sched_graph' | 'sched_eager' (lr_schedule=0.5, epoch_end() after every third step) | 'hand_eager' (no lr_schedule,
  eager, optim_G.lr / optim_D.lr assigned by hand at the same points to the same floats) | 'const_graph' (today's trainer).
  -> per step: losses, checksums; at the end: flat buffers, lr(), loss scales."""
  from mix_stage_amd.train_step import MixStageTrainStep
  audio, pose, labels, style = _batch()
  torch.manual_seed(5)
  model = _hip(M_, S_, None if precision == 'fp32' else precision)
  kw = dict(use_graphs=mode.endswith('graph'))
  if mode.startswith('sched'):
    kw['lr_schedule'] = GAMMA
  if loss_scale is not None:
    kw['loss_scale'] = loss_scale
  ts = MixStageTrainStep(model, **kw)
  hand = _hand_lrs(1e-4, GAMMA, steps // 3 + 1)
  losses, sums = [], []
  for i, k in enumerate((kinds or KINDS12)[:steps]):
    ts.step(audio, labels, pose, style, kind=k)
    losses.append([float(l) for l in ts.losses])
    sums.append(ts.state_checksums())
    if i % 3 == 2:
      if mode.startswith('sched'):
        assert ts.epoch_end() == (hand[i // 3 + 1],) * 2
      elif mode == 'hand_eager':
        ts.optim_G.lr = ts.optim_D.lr = hand[i // 3 + 1]
  torch.cuda.synchronize()
  ts.check_health()
  assert ts.skipped_steps == 0
  return dict(losses=losses, sums=sums, lr=ts.lr(), pG=ts.optim_G.flat_p.clone(), pD=ts.optim_D.flat_p.clone(),
              mG=ts.optim_G.exp_avg.clone(), vD=ts.optim_D.exp_avg_sq.clone(),
              scale=ts.loss_scale() if loss_scale is not None else None, word=(ts.optim_G.lr_word, ts.optim_D.lr_word))


@functools.lru_cache(maxsize=None)
def _cached(precision, mode):
  return _run(precision, mode)


def _same(a, b):
  assert a['losses'] == b['losses'], [(i, x, y) for i, (x, y) in enumerate(zip(a['losses'], b['losses'])) if x != y][:2]
  assert a['sums'] == b['sums']
  for name in ('pG', 'pD', 'mG', 'vD'):
    assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_captured_steps_follow_the_schedule_graph_equals_eager(precision):
  graph, eager = _cached(precision, 'sched_graph'), _cached(precision, 'sched_eager')
  _same(graph, eager)
  want = _hand_lrs(1e-4, GAMMA, 4)[4]
  assert graph['lr'] == eager['lr'] == (want, want) and want == 1e-4 / 16
  assert [float(w) for w in graph['word']] == [f32(want)] * 2            # what the device holds is float32(lr)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_the_new_path_equals_the_old_kernels_with_lr_assigned_by_hand(precision):
  hand = _cached(precision, 'hand_eager')
  assert hand['word'] == (None, None)                   # no device word: the by-value entry points ran
  _same(_cached(precision, 'sched_graph'), hand)
  _same(_cached(precision, 'sched_eager'), hand)


def test_the_schedule_is_actually_followed():
  """Against today's captured trainer (constant lr): identical through step 3 -- the first epoch_end() comes behind it -- and
  different from step 4 on."""
  sched, const = _cached('fp32', 'sched_graph'), _cached('fp32', 'const_graph')
  assert sched['sums'][:3] == const['sums'][:3] and sched['losses'][:3] == const['losses'][:3]
  for i in range(3, 12):
    assert sched['sums'][i] != const['sums'][i], i
  assert const['lr'] == (1e-4, 1e-4) and const['word'] == (None, None)
  print('step 3 pose loss %.9g; final checksums with the schedule %s, constant lr %s'
        % (sched['losses'][2][0], sched['sums'][-1], const['sums'][-1]))
  assert not torch.equal(sched['pG'], const['pG']) and not torch.equal(sched['pD'], const['pD'])


def test_fp16_with_dynamic_loss_scaling_graph_equals_eager():
  graph = _run('fp16', 'sched_graph', steps=8, loss_scale='dynamic')
  eager = _run('fp16', 'sched_eager', steps=8, loss_scale='dynamic')
  _same(graph, eager)
  assert graph['scale'] == eager['scale'] and graph['lr'] == eager['lr'] == (2.5e-5, 2.5e-5)
  assert all(math.isfinite(x) for row in graph['losses'] for x in row)
  const = _run('fp16', 'const_graph', steps=8, loss_scale='dynamic')
  assert const['sums'][:3] == graph['sums'][:3] and const['sums'][3:] != graph['sums'][3:]      # the scaled twin reads the word too


def test_three_epochs_vs_oracle_with_torch_exponential_lr():
  """The comparisons and bars of test_gpu_train_step.py::test_three_steps_vs_oracle_and_graph_equals_eager, on three epochs of one
  G-step and one D-step with ExponentialLR(gamma=0.5) stepped per epoch on both sides; the oracle computes in float64."""
  import warnings
  from mix_stage_amd.train_step import MixStageTrainStep
  M = S = 2
  batches = [O.synthetic_batch(4, M=M, S=S, seed=50 + i) for i in range(6)]
  kinds = ['G', 'D'] * 3
  ref = O.build_gan(M=M, S=S, dtype=torch.float64)
  og = torch.optim.Adam(ref.G.parameters(), lr=1e-4)
  od = torch.optim.Adam(ref.D.parameters(), lr=1e-4)
  sg = torch.optim.lr_scheduler.ExponentialLR(og, gamma=GAMMA)
  sd = torch.optim.lr_scheduler.ExponentialLR(od, gamma=GAMMA)
  ref_losses, ref_lrs = [], []
  for i, ((audio, pose, labels, style), k) in enumerate(zip(batches, kinds)):
    _, l, _ = O.oracle_train_step(ref, og, od, audio.double(), pose.double(), labels, style, k)
    ref_losses.append([float(x) for x in l])
    if i % 2 == 1:
      with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sg.step(); sd.step()
      ref_lrs.append((og.param_groups[0]['lr'], od.param_groups[0]['lr']))
  results = {}
  for use_graphs in (False, True):
    torch.manual_seed(99)
    model = _hip(M, S)
    ts = MixStageTrainStep(model, use_graphs=use_graphs, lr_schedule=GAMMA)
    got, lrs = [], []
    for i, ((audio, pose, labels, style), k) in enumerate(zip(batches, kinds)):
      ts.step(audio.to(DEV), labels.to(DEV), pose.to(DEV), style.to(DEV), kind=k)
      got.append([float(l) for l in ts.losses])
      if i % 2 == 1:
        lrs.append(ts.epoch_end())
    assert lrs == ref_lrs                               # the host values are torch's, bit for bit
    results[use_graphs] = (got, {k: v.clone() for k, v in model.state_dict().items()}, ts.optim_G.step_count, ts.optim_D.step_count)
  eager, graph = results[False], results[True]
  assert eager[2:] == (3, 3) and graph[2:] == (3, 3)
  # step 1 sees identical weights; later steps see weights that differ by Adam's sign-like first updates
  for i, (a, b) in enumerate(zip(eager[0], ref_losses)):
    np.testing.assert_allclose(a, b, atol=2e-4 if i == 0 else 3e-3)
  ref_sd = ref.state_dict()
  for k, v in eager[1].items():
    if v.is_floating_point():
      d = (v.cpu().double() - ref_sd[k]).abs()
      if 'running_' in k:     # batch statistics of slightly different weights: relative bar
        assert d.max().item() <= 2e-3 * (1 + ref_sd[k].abs().max().item()), (k, d.max().item())
      else:                   # parameters: the bars of the three-step test (2 Adam steps * 2 * lr): three steps per network under the
        #                       schedule move an element by at most (1 + 1/2 + 1/4) * lr = 1.75e-4, twice that is inside them
        assert d.max().item() <= 4.5e-4, (k, d.max().item())
        assert d.mean().item() <= 1e-4, (k, d.mean().item())
    else:
      assert int(v) == int(ref_sd[k]), k
  # graph replay is bit-identical to eager
  assert graph[0] == eager[0]
  for k, v in eager[1].items():
    assert torch.equal(v, graph[1][k]), k


def test_trainer_api_set_lr_state_round_trip_and_refusals():
  from mix_stage_amd.train_step import FlatAdam, MixStageTrainStep
  audio, pose, labels, style = _batch()

  def fresh(**kw):
    torch.manual_seed(5)
    return MixStageTrainStep(_hip(M_, S_), **kw)

  def run(ts, kinds):
    out = []
    for k in kinds:
      ts.step(audio, labels, pose, style, kind=k)
      out.append(([float(l) for l in ts.losses], ts.state_checksums()))
    return out

  ts = fresh(lr_schedule=GAMMA)
  assert ts.lr() == (1e-4, 1e-4) and ts.optim_G.device_lr and ts.optim_G.lr_word.data_ptr() != ts.optim_D.lr_word.data_ptr()
  assert float(ts.optim_G.lr_word) == float(ts.optim_D.lr_word) == f32(1e-4)             # written at construction
  ts.set_lr(G=2e-4)
  assert ts.lr() == (2e-4, 1e-4) and float(ts.optim_G.lr_word) == f32(2e-4) and float(ts.optim_D.lr_word) == f32(1e-4)
  ts.set_lr(D=3e-5)
  assert ts.lr() == (2e-4, 3e-5) and float(ts.optim_G.lr_word) == f32(2e-4) and float(ts.optim_D.lr_word) == f32(3e-5)
  for bad in (0.0, -1e-4, float('nan'), float('inf')):
    with pytest.raises(ValueError):
      ts.set_lr(G=bad)
  assert ts.lr() == (2e-4, 3e-5) and float(ts.optim_G.lr_word) == f32(2e-4)              # a rejected value wrote nothing
  ts.optim_G.reset_state()
  assert ts.lr()[0] == 2e-4 and float(ts.optim_G.lr_word) == f32(2e-4)                   # a hyper-parameter, not optimizer state
  ts.set_lr(G=1e-4, D=1e-4)
  # an uninterrupted run of 4 + 6 steps with an epoch end behind steps 2, 4, 7 ...
  first = run(ts, ['G', 'D'])
  ts.epoch_end()
  first += run(ts, ['G', 'D'])
  ts.epoch_end()
  st = ts.lr_state()
  assert st == dict(epoch=2, lr_G=2.5e-5, lr_D=2.5e-5, schedule=((2,), (2,)))
  snap = {k: v.clone() for k, v in ts.model.state_dict().items()}
  opt = [[t.clone() for t in (o.exp_avg, o.exp_avg_sq, o.step_state, o.seg_first)] + [list(o.host_first), o.host_step]
         for o in (ts.optim_G, ts.optim_D)]
  thresh = (ts.model.G.thresh.value, ts.model.G.thresh.iters)
  rng = torch.get_rng_state()
  tail = run(ts, ['G', 'D', 'G'])
  ts.epoch_end()
  tail += run(ts, ['D', 'G', 'D'])
  assert ts.lr() == (1.25e-5, 1.25e-5)
  # ... and the same six steps on a FRESH trainer that resumes: the caller restores weights and optimizer state, lr_state the rest
  ts2 = fresh(lr_schedule=GAMMA)
  ts2.model.load_state_dict(snap)
  for o, (m, v, state, seg_first, host_first, host_step) in zip((ts2.optim_G, ts2.optim_D), opt):
    o.exp_avg.copy_(m); o.exp_avg_sq.copy_(v); o.step_state.copy_(state); o.seg_first.copy_(seg_first)
    o.host_first, o.host_step = list(host_first), host_step
  ts2.model.G.thresh.value, ts2.model.G.thresh.iters = thresh
  torch.set_rng_state(rng)
  ts2.set_lr_state(st)
  assert ts2.lr_state() == st and ts2.lr() == (2.5e-5, 2.5e-5) and float(ts2.optim_D.lr_word) == f32(2.5e-5)
  tail2 = run(ts2, ['G', 'D', 'G'])
  ts2.epoch_end()
  tail2 += run(ts2, ['D', 'G', 'D'])
  assert tail2 == tail
  assert torch.equal(ts2.optim_G.flat_p, ts.optim_G.flat_p) and torch.equal(ts2.optim_D.flat_p, ts.optim_D.flat_p)

  # without lr_schedule: a trainer that replays graphs refuses (it used to ignore the value silently), an eager one takes the value
  plain = fresh()
  for call in (lambda: plain.set_lr(G=2e-4), plain.epoch_end, lambda: plain.set_lr_state(st)):
    with pytest.raises(RuntimeError, match='lr_schedule='):
      call()
  assert plain.lr() == (1e-4, 1e-4) and plain.optim_G.lr_word is None and not plain.optim_G.device_lr
  eager = fresh(use_graphs=False)
  eager.set_lr(G=2e-4)
  assert eager.lr() == (2e-4, 1e-4) and eager.epoch_end() == (2e-4, 1e-4) and eager.lr_state()['epoch'] == 1
  eager.set_lr(G=1e-4, D=5e-5)
  ref = fresh(lr_schedule=GAMMA)
  ref.set_lr(D=5e-5)
  assert run(eager, ['D', 'G']) == run(ref, ['D', 'G'])                                  # the eager launches honour the host value
  with pytest.raises(ValueError):
    ref.set_lr_state(eager.lr_state())                  # a state without a schedule onto a trainer with one
  # FlatAdam on its own
  w = torch.nn.Parameter(torch.ones(100, device=DEV))
  fa = FlatAdam([w], lr=3e-4, device_lr=True)
  assert float(fa.lr_word) == f32(3e-4)
  with pytest.raises(ValueError):
    FlatAdam([torch.nn.Parameter(torch.ones(4, device=DEV))], lr=0.0, device_lr=True)


def test_labelled_launch_sequence_is_the_parent_forms():
  """One eager G-step and one eager D-step: the labelled launches (every label with its count, as ms_timing_report lists them) with lr_schedule
  are those without it -- one prep launch stands for one prep launch under the same label."""
  from mix_stage_amd import ops
  from mix_stage_amd.train_step import MixStageTrainStep
  audio, pose, labels, style = _batch()
  seqs = {}
  for name, kw in (('parent', {}), ('schedule', dict(lr_schedule=0.99))):
    torch.manual_seed(5)
    ts = MixStageTrainStep(_hip(M_, S_), use_graphs=False, **kw)
    for k in ('G', 'D'):                                # (first steps create prepared weights and sync buffers: not compared)
      ts.step(audio, labels, pose, style, kind=k)
    torch.cuda.synchronize()
    rows = []
    try:
      for k in ('G', 'D'):
        ops.timing_enable(True)                         # (empties the record)
        ts.step(audio, labels, pose, style, kind=k)
        torch.cuda.synchronize()
        rows.append([(r['label'], r['count']) for r in ops.timing_report()])
    finally:
      ops.timing_enable(False)
    seqs[name] = rows
  assert seqs['parent'] == seqs['schedule']
  for rows in seqs['schedule']:
    assert sum(c for l, c in rows if l == 'ew|ew_adam_step_segmented') == 1 and len(rows) > 10
