"""GPU: the moving average (EMA) of the generator's weights.  C-ABI level: ms_adam_step_segmented_ema against the four existing
entry points bit for bit, the average against the float64 recurrence at a derived bound, vector path == scalar path, refused
steps and idle segments leave it alone, and what the entry point refuses.  Trainer level: the average is an observer (same
launches, same bits of everything else, graph == eager), ema_weights() swaps it in and out with every derived cache following,
the sampler's captured graph follows the weights, save_weights(ema=True), and a run resumes from optimizer_state()."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_ema_cpu import DECAYS, ema_bound, ema_reference64
from test_gpu_lr_schedule import BETAS, BIG, CASES, EPS, LRS, MAX_NORM, SMALL, _Flat, _hip, _ls_words
from test_gpu_lr_schedule import _grads as _make_grads

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 123.0


@functools.lru_cache(maxsize=None)
def _grads(case, steps):
  return _make_grads(case, steps)


class _FlatE(_Flat):
  """_Flat with a fifth buffer `e` of the layout of p, on a view offset like the others; the floats around it hold GUARD."""

  def __init__(self, case, offset=0, e0=None, **kw):
    super().__init__(case, offset, **kw)
    self.offset = offset
    self.ebuf = torch.full((self.n + 4 * offset,), GUARD, dtype=torch.float32, device=DEV)
    self.e = self.ebuf[offset:offset + self.n]
    assert self.e.data_ptr() % 16 == 4 * offset
    self.e.copy_(self.p if e0 is None else e0)

  def step_ema(self, g, lr, decay, lr_word=False, ls=None, rule=None, norm=None):
    from mix_stage_amd import ops
    self.g.copy_(g)
    if norm is None:
      ops.grad_norm(self.g, self.norm, self.partials)
    else:
      self.norm.fill_(norm)
    if lr_word:
      ops.write_floats(self.lr_word, [lr])
    kw = {}
    if ls is not None:
      kw = dict(loss_scale_state=ls, growth_interval=rule.growth_interval, min_scale=rule.min, max_scale=rule.max)
    ops.adam_step_segmented_ema(self.p, self.g, self.m, self.v, self.norm, MAX_NORM, None if lr_word else lr, BETAS[0], BETAS[1], EPS,
                                self.step_state, self.seg_of_chunk, self.seg_first, self.seg_scratch, self.e, decay,
                                lr_word=self.lr_word if lr_word else None, **kw)

  def guards_intact(self):
    o = self.offset
    ok = bool((self.ebuf[:o] == GUARD).all()) and bool((self.ebuf[o + self.n:] == GUARD).all())
    for b in self.bufs:                                  # p, g, m, v: zero-filled around their views
      ok = ok and bool((b[:o] == 0).all()) and bool((b[o + self.n:] == 0).all())
    return ok


def _active(case, step):
  """bool per element: the segment is updated in (1-based) step `step`."""
  sizes, first = case
  f = torch.tensor(first).repeat_interleave(torch.tensor(sizes))
  return ((f >= 1) & (f <= step)).numpy()


# ------------------------------------------------------------------------------------------------ C-ABI level
FORMS = [pytest.param(False, None, id='plain'), pytest.param(True, None, id='lr_word'), pytest.param(False, 1.0, id='scaled_S1'),
         pytest.param(False, 2.0 ** 16, id='scaled_S65536'), pytest.param(True, 1.0, id='scaled_lr_word_S1'),
         pytest.param(True, 2.0 ** 16, id='scaled_lr_word_S65536')]


@pytest.mark.parametrize('lr_word,S', FORMS)
@pytest.mark.parametrize('case,offset', CASES)
def test_everything_but_the_average_equals_the_existing_entry_point_bit_for_bit(case, offset, lr_word, S):
  from mix_stage_amd.loss_scale import LossScaleRule
  grads = _grads(case, len(LRS))
  ref, got = _Flat(case, offset), _FlatE(case, offset)
  rule = LossScaleRule(S) if S is not None else None
  ls_ref, ls_got = (_ls_words(S), _ls_words(S)) if S is not None else (None, None)
  e0 = got.e.clone()
  for g, lr in zip(grads, LRS):
    k = S if S is not None else 1.0
    ref.step(g * k, lr, by_value=not lr_word, ls=ls_ref, rule=rule)
    got.step_ema(g * k, lr, 0.999, lr_word=lr_word, ls=ls_got, rule=rule)
    for name, t in ref.words().items():
      assert torch.equal(t, got.words()[name]), (name, lr)
    assert torch.equal(ref.norm, got.norm)
    if S is not None:
      assert torch.equal(ls_ref, ls_got)
  assert got.step_state.tolist()[0] == 4 and got.step_state.tolist()[2:] == [0, 0]
  assert not torch.equal(got.e, e0) and bool(torch.isfinite(got.e).all()) and got.guards_intact()


@pytest.mark.parametrize('decay', DECAYS)
@pytest.mark.parametrize('case,offset', CASES)
def test_the_average_against_the_float64_recurrence(case, offset, decay):
  """K = 4 steps on the device's own p_k.  Bound per element: K * 2^-23 * max(|e_0|, |p_k|) + K * 2^-149 (derived in
  test_ema_cpu.ema_bound, where a float32 emulation of the update stays at half of it).  Measured on the MI355X, worst error /
  bound over the four buffers: 0.23 (decay 0.5), 0.47 (0.999), 0.45 (0.9999)."""
  K = 4
  grads = _grads(case, K)
  fl = _FlatE(case, offset)
  e0 = fl.e.cpu().numpy()
  ps = []
  for g, lr in zip(grads, LRS):
    fl.step_ema(g, lr, decay)
    ps.append(fl.p.cpu().numpy())
  act = [_active(case, s) for s in range(1, K + 1)]
  ref = ema_reference64(e0, ps, decay, act)
  err = np.abs(fl.e.cpu().numpy().astype(np.float64) - ref)
  bound = ema_bound(e0, ps, K)
  worst = float((err / bound).max())
  print('EMA64 decay %g: worst error / bound %.3f, max error %.3e' % (decay, worst, float(err.max())))
  assert worst <= 1.0
  assert float(np.abs(ref - e0).max()) > 0.0               # the average moved at all


@pytest.mark.parametrize('case', [SMALL, BIG], ids=['5seg', '2p20_plus_64'])
def test_vector_path_and_scalar_path_give_the_same_average(case):
  grads = _grads(case, 4)
  vec, sca = _FlatE(case, 0), _FlatE(case, 1)
  for g, lr in zip(grads, LRS):
    vec.step_ema(g, lr, 0.999)
    sca.step_ema(g, lr, 0.999)
  for name in ('p', 'm', 'v', 'e'):
    assert torch.equal(getattr(vec, name), getattr(sca, name)), name
  assert vec.guards_intact() and sca.guards_intact()


def test_a_refused_step_leaves_the_average_alone_and_the_next_good_step_moves_it():
  grads = _grads(SMALL, 3)
  fl = _FlatE(SMALL)
  fl.step_ema(grads[0], 1e-4, 0.9)
  before = [t.clone() for t in (fl.e, fl.p, fl.m, fl.v)]
  fl.step_ema(grads[1], 1e-4, 0.9, norm=float('nan'))      # (a value in the norm word: the prep kernel refuses the step)
  for a, b in zip(before, (fl.e, fl.p, fl.m, fl.v)):
    assert torch.equal(a, b)
  assert fl.step_state.tolist()[0] == 2 and fl.step_state.tolist()[2:] == [1, 1]
  fl.step_ema(grads[2], 1e-4, 0.9)
  assert fl.step_state.tolist()[0] == 3 and fl.step_state.tolist()[2:] == [0, 1]
  assert not torch.equal(fl.e, before[0]) and bool(torch.isfinite(fl.e).all())


def test_an_overflow_skip_leaves_the_average_alone_and_halves_the_scale():
  from mix_stage_amd.loss_scale import LossScaleRule
  grads = _grads(SMALL, 3)
  rule = LossScaleRule(dict(init=8, growth_interval=0, min=2, max=8))
  fl, ls = _FlatE(SMALL), _ls_words(8.0)
  fl.step_ema(grads[0] * 8.0, 1e-4, 0.9, ls=ls, rule=rule)
  before = [t.clone() for t in (fl.e, fl.p, fl.m, fl.v)]
  fl.step_ema(grads[1] * 8.0, 1e-4, 0.9, ls=ls, rule=rule, norm=float('inf'))
  for a, b in zip(before, (fl.e, fl.p, fl.m, fl.v)):
    assert torch.equal(a, b)
  assert torch.equal(ls.cpu(), _ls_words(4.0, good=0, skips=1, last=1).cpu())
  assert fl.step_state.tolist()[0] == 2 and fl.step_state.tolist()[2:] == [1, 0]      # an overflow skip is not a bad step
  fl.step_ema(grads[2] * 4.0, 1e-4, 0.9, ls=ls, rule=rule)
  assert fl.step_state.tolist()[2:] == [0, 0] and not torch.equal(fl.e, before[0])


@pytest.mark.parametrize('offset', [0, 1], ids=['vector', 'scalar'])
def test_idle_segments_keep_their_initial_average(offset):
  """e_0 differs from p: the never-updated segment (first step -1) keeps its bits through four steps, the segment whose first
  step is 2 keeps them through step 1 and moves in step 2."""
  sizes, first = SMALL
  n = sum(sizes)
  e0 = torch.randn(n, generator=torch.Generator().manual_seed(77)).to(DEV)
  fl = _FlatE(SMALL, offset, e0=e0)
  lo = [sum(sizes[:i]) for i in range(len(sizes))]
  never, late = first.index(-1), first.index(2)
  sl = lambda i: slice(lo[i], lo[i] + sizes[i])
  grads = _grads(SMALL, 4)
  fl.step_ema(grads[0], 1e-4, 0.5)
  assert torch.equal(fl.e[sl(never)], e0[sl(never)]) and torch.equal(fl.e[sl(late)], e0[sl(late)])
  live = first.index(1)
  assert not torch.equal(fl.e[sl(live)], e0[sl(live)])
  fl.step_ema(grads[1], 1e-4, 0.5)
  assert torch.equal(fl.e[sl(never)], e0[sl(never)]) and not torch.equal(fl.e[sl(late)], e0[sl(late)])
  for g in grads[2:]:
    fl.step_ema(g, 1e-4, 0.5)
  assert torch.equal(fl.e[sl(never)], e0[sl(never)]) and fl.guards_intact()


def test_a_null_average_and_bad_decays_are_errors_and_launch_nothing():
  from mix_stage_amd import ops
  fl = _FlatE(SMALL)
  fl.g.copy_(_grads(SMALL, 1)[0])
  fl.norm.fill_(1.0)
  ls = _ls_words(8.0)
  L = ops.lib()
  P = lambda t: ctypes.c_void_p(t.data_ptr())
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  head = (P(fl.p), P(fl.g), P(fl.m), P(fl.v), fl.n, P(fl.norm), MAX_NORM, 1e-4, None)
  mid = (BETAS[0], BETAS[1], EPS, P(fl.step_state), P(fl.seg_of_chunk), P(fl.seg_first), P(fl.seg_scratch), len(SMALL[0]))
  plain = (None, 0, 1.0, 1.0, None, 0)
  before = [t.clone() for t in (fl.p, fl.m, fl.v, fl.e, fl.step_state, fl.seg_scratch)]
  ops.timing_enable(True)
  try:
    assert L.ms_adam_step_segmented_ema(*head, *mid, *plain, None, 0.999, stream) != 0
    assert 'ema' in ops.lib().ms_last_error().decode()
    for bad in (float('nan'), 1.0, -0.1, float('inf'), float('-inf'), 1.5):
      assert L.ms_adam_step_segmented_ema(*head, *mid, *plain, P(fl.e), bad, stream) != 0, bad
      assert L.ms_adam_step_segmented_ema(*head, *mid, P(ls), 0, 2.0, 8.0, None, 0, P(fl.e), bad, stream) != 0, bad
    # the refusals of the scaled form: no norm, a bad scale range, a table without a pointer
    assert L.ms_adam_step_segmented_ema(*head[:5], None, *head[6:], *mid, P(ls), 0, 2.0, 8.0, None, 0, P(fl.e), 0.999, stream) != 0
    assert L.ms_adam_step_segmented_ema(*head, *mid, P(ls), 0, 0.0, 8.0, None, 0, P(fl.e), 0.999, stream) != 0
    assert L.ms_adam_step_segmented_ema(*head, *mid, P(ls), 0, 2.0, 8.0, None, 3, P(fl.e), 0.999, stream) != 0
    torch.cuda.synchronize()
    assert [r['label'] for r in ops.timing_report()] == []
    for a, b in zip(before, (fl.p, fl.m, fl.v, fl.e, fl.step_state, fl.seg_scratch)):
      assert torch.equal(a, b)
    assert L.ms_adam_step_segmented_ema(*head, *mid, *plain, P(fl.e), 0.999, stream) == 0      # the same arguments, a good pair
    torch.cuda.synchronize()
    assert [(r['label'], r['count']) for r in ops.timing_report()] == [('ew|ew_adam_step_segmented', 1)]
  finally:
    ops.timing_enable(False)
  assert fl.step_state.tolist()[0] == 1 and not torch.equal(fl.e, before[3])
  for bad_e in (fl.e.double(), fl.e[:-1], fl.e.cpu()):
    with pytest.raises(TypeError):
      ops.adam_step_segmented_ema(fl.p, fl.g, fl.m, fl.v, fl.norm, MAX_NORM, 1e-4, BETAS[0], BETAS[1], EPS, fl.step_state,
                                  fl.seg_of_chunk, fl.seg_first, fl.seg_scratch, bad_e, 0.999)
  with pytest.raises(ValueError):
    ops.adam_step_segmented_ema(fl.p, fl.g, fl.m, fl.v, fl.norm, MAX_NORM, 1e-4, BETAS[0], BETAS[1], EPS, fl.step_state,
                                fl.seg_of_chunk, fl.seg_first, fl.seg_scratch, fl.e, 1.0)


def test_flat_adam_owns_the_average_and_restarts_it_on_demand():
  from mix_stage_amd.train_step import FlatAdam
  w = torch.nn.Parameter(torch.randn(100, generator=torch.Generator().manual_seed(3)).to(DEV))
  fa = FlatAdam([w], ema_decay=0.5)
  assert fa.ema.dtype == torch.float32 and fa.ema.shape == fa.flat_p.shape and torch.equal(fa.ema, fa.flat_p)
  assert fa.ema.data_ptr() != fa.flat_p.data_ptr()

  def step():
    fa.zero_grad()
    fa.flat_g[:100].fill_(0.25)
    fa.mark_active([0])
    fa.clip_and_step()

  p0 = fa.flat_p.clone()
  step()
  # one step at decay 0.5: the average sits halfway between the start and the new weights (exactly: a halving and one rounding)
  assert not torch.equal(fa.flat_p, p0)
  want = (p0.double() + 0.5 * (fa.flat_p.double() - p0.double()))
  assert float((fa.ema.double() - want).abs().max()) <= 2.0 ** -23 * float(p0.abs().max())
  assert torch.equal(fa.ema[100:], p0[100:])               # the padding behind the parameter
  fa.ema_reset()
  assert torch.equal(fa.ema, fa.flat_p)
  step()
  assert not torch.equal(fa.ema, fa.flat_p)
  fa.reset_state()
  assert torch.equal(fa.ema, fa.flat_p) and fa.step_count == 0 and float(fa.exp_avg.abs().max()) == 0.0
  st = fa.optimizer_state()
  assert sorted(st) == ['ema', 'exp_avg', 'exp_avg_sq', 'host_first', 'host_step', 'step_state', 'total']
  plain = FlatAdam([torch.nn.Parameter(torch.ones(8, device=DEV))])
  assert plain.ema is None and plain.ema_decay is None and plain.optimizer_state()['ema'] is None
  with pytest.raises(RuntimeError):
    plain.ema_reset()


# ------------------------------------------------------------------------------------------------ trainer level
M_ = S_ = 2
DECAY = 0.9
KINDS12 = ['G', 'D'] * 6


@functools.lru_cache(maxsize=None)
def _batch():
  from oracle import mixstage_oracle as O
  return tuple(t.to(DEV) for t in O.synthetic_batch(4, M=M_, S=S_, seed=11))


def _trainer(precision, graph, ema, loss_scale=None):
  from mix_stage_amd.train_step import MixStageTrainStep
  torch.manual_seed(5)
  model = _hip(M_, S_, None if precision == 'fp32' else precision)
  kw = dict(use_graphs=graph)
  if ema is not None:
    kw['ema_decay'] = ema
  if loss_scale is not None:
    kw['loss_scale'] = loss_scale
  return MixStageTrainStep(model, **kw)


def _steps(ts, kinds):
  audio, pose, labels, style = _batch()
  out = []
  for k in kinds:
    ts.step(audio, labels, pose, style, kind=k)
    out.append(([float(l) for l in ts.losses], ts.state_checksums()))
  return out


def _state(ts):
  d = {}
  for n, o in (('G', ts.optim_G), ('D', ts.optim_D)):
    d['p' + n], d['m' + n], d['v' + n] = o.flat_p.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone()
    d['clock' + n] = (int(o.step_state[0]), o.host_step, list(o.host_first))
  d['ema'] = ts.optim_G.ema.clone() if ts.optim_G.ema is not None else None
  return d


def _run(precision, graph, ema, steps=12, loss_scale=None):
  """-> per step (losses, checksums); the flat buffers at the end; with an average in fp32: its start, and G's weights (behind
  G-steps) and the average behind every step.  One run per configuration, shared by the tests."""
  return _run_cached(precision, graph, ema, steps, loss_scale)


@functools.lru_cache(maxsize=None)
def _run_cached(precision, graph, ema, steps, loss_scale):
  ts = _trainer(precision, graph, ema, loss_scale)
  track = ema is not None and precision == 'fp32' and graph and steps == 12
  rows, trace = [], []
  e0 = ts.optim_G.ema.cpu().numpy() if track else None
  for k in KINDS12[:steps]:
    rows += _steps(ts, [k])
    if track:
      trace.append((k, ts.optim_G.flat_p.cpu().numpy() if k == 'G' else None, ts.optim_G.ema.clone()))
  torch.cuda.synchronize()
  ts.check_health()
  assert ts.skipped_steps == 0
  out = dict(rows=rows, trace=trace, e0=e0, first=(list(ts.optim_G.host_first), list(ts.optim_G.offsets),
                                            [p.numel() for p in ts.optim_G.params], ts.optim_G.total))
  out.update(_state(ts))
  return out


def _same(a, b, names=('pG', 'mG', 'vG', 'pD', 'mD', 'vD')):
  assert a['rows'] == b['rows'], [(i, x, y) for i, (x, y) in enumerate(zip(a['rows'], b['rows'])) if x != y][:1]
  for name in names:
    assert torch.equal(a[name], b[name]), name
  assert a['clockG'] == b['clockG'] and a['clockD'] == b['clockD']


def test_labelled_launch_sequence_is_the_parent_one():
  """One eager G-step and one eager D-step: label for label the launches without the average, one optimizer launch pair each."""
  from mix_stage_amd import ops
  audio, pose, labels, style = _batch()
  seqs = {}
  for name, ema in (('parent', None), ('ema', DECAY)):
    ts = _trainer('fp32', False, ema)
    for k in ('G', 'D'):                                # (first steps create prepared weights and sync buffers: not compared)
      ts.step(audio, labels, pose, style, kind=k)
    torch.cuda.synchronize()
    rows = []
    try:
      for k in ('G', 'D'):
        ops.timing_enable(True)
        ts.step(audio, labels, pose, style, kind=k)
        torch.cuda.synchronize()
        rows.append([(r['label'], r['count']) for r in ops.timing_report()])
    finally:
      ops.timing_enable(False)
    seqs[name] = rows
  assert seqs['parent'] == seqs['ema']
  for rows in seqs['ema']:
    assert sum(c for l, c in rows if l == 'ew|ew_adam_step_segmented') == 1 and len(rows) > 10


@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_the_average_is_an_observer(precision, graph):
  with_ema, without = _run(precision, graph, DECAY), _run(precision, graph, None)
  _same(with_ema, without)
  assert without['ema'] is None and with_ema['ema'] is not None
  assert not torch.equal(with_ema['ema'], with_ema['pG']) and bool(torch.isfinite(with_ema['ema']).all())


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_the_average_is_the_same_for_graph_and_eager(precision):
  graph, eager = _run(precision, True, DECAY), _run(precision, False, DECAY)
  _same(graph, eager)
  assert torch.equal(graph['ema'], eager['ema'])


def test_fp16_with_dynamic_loss_scaling_the_average_is_the_same_for_graph_and_eager():
  graph = _run('fp16', True, DECAY, steps=6, loss_scale='dynamic')
  eager = _run('fp16', False, DECAY, steps=6, loss_scale='dynamic')
  _same(graph, eager)
  assert torch.equal(graph['ema'], eager['ema']) and not torch.equal(graph['ema'], graph['pG'])
  plain = _run('fp16', True, None, steps=6, loss_scale='dynamic')
  _same(graph, plain)


def test_trainer_average_against_float64_and_d_steps_never_move_it():
  """The bound of the C-ABI test with K = 6 G-steps (measured: worst error / bound 0.36); bitwise unchanged across every D-step."""
  r = _run('fp32', True, DECAY)
  host_first, offsets, numels, total = r['first']
  first = np.full(total, -1, dtype=np.int64)
  for f, o, n in zip(host_first, offsets, numels):
    first[o:o + (n + 63) // 64 * 64] = f
  e0 = r['e0']                                             # the average started as the initial weights
  ps, act, prev, g_step = [], [], None, 0
  for kind, p, e in r['trace']:
    if kind == 'D':
      assert torch.equal(e, prev), 'a D-step moved the average'
    else:
      g_step += 1
      ps.append(p)
      act.append((first >= 1) & (first <= g_step))
      assert prev is None or not torch.equal(e, prev)
    prev = e
  K = len(ps)
  assert K == 6 and bool(act[0].any()) and not bool(act[-1].all())      # some parameters of G never get a gradient on this path
  ref = ema_reference64(e0, ps, DECAY, act)
  err = np.abs(r['ema'].cpu().numpy().astype(np.float64) - ref)
  worst = float((err / ema_bound(e0, ps, K)).max())
  print('EMA64 trainer: worst error / bound %.3f, max error %.3e' % (worst, float(err.max())))
  assert worst <= 1.0
  idle = ~act[-1]
  assert np.array_equal(r['ema'].cpu().numpy()[idle], e0[idle])


def _windows():
  audio, pose, labels, style = _batch()
  return audio[:2].contiguous(), labels[:2].contiguous(), pose[:2].contiguous(), torch.full_like(style[:2], 1)


def _sample(sampler):
  torch.manual_seed(5)
  out = sampler.sample_interval(*_windows(), all_styles=True)
  return [(name, y.clone(), [l.clone() for l in losses]) for name, y, losses in out]


def _same_samples(a, b):
  assert len(a) == len(b) == S_
  for (na, ya, la), (nb, yb, lb) in zip(a, b):
    assert na == nb and torch.equal(ya, yb) and all(torch.equal(x, y) for x, y in zip(la, lb))


def _host_state(ts):
  m = ts.model
  return dict(rng=torch.get_rng_state(), thresh=(m.G.thresh.value, m.G.thresh.iters), sched=m.lambda_scheduler.state(),
              lam=(m.lambda_D, m.lambda_gan), flags=(m.G_flag, m.fake_flag))


def _set_host_state(ts, h):
  m = ts.model
  torch.set_rng_state(h['rng'])
  m.G.thresh.value, m.G.thresh.iters = h['thresh']
  m.lambda_scheduler.set_state(h['sched'])
  m.lambda_D, m.lambda_gan = h['lam']
  m.G_flag, m.fake_flag = h['flags']


def _fresh_model_on_the_average(ts, precision):
  """A model of its own whose G parameters are the average, everything else the trainer's live state."""
  sd = {k: v.clone() for k, v in ts.model.state_dict().items()}
  avg = ts.ema_state_dict()
  assert list(avg.keys()) == list(ts.model.G.state_dict().keys())
  for k, v in avg.items():
    sd['G.' + k] = v
  fresh = _hip(M_, S_, None if precision == 'fp32' else precision)
  fresh.load_state_dict(sd, strict=True)
  return fresh


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_ema_weights_swaps_the_average_in_and_out(precision):
  from mix_stage_amd.sample import StyleTransferSampler
  ts = _trainer(precision, True, DECAY)
  _steps(ts, ['G', 'D', 'G', 'D'])
  live, avg = ts.optim_G.flat_p.clone(), ts.optim_G.ema.clone()
  pD = ts.optim_D.flat_p.clone()
  fresh = _fresh_model_on_the_average(ts, precision)     # (reads state_dict(): the pending BatchNorm batch counts are folded in)
  bufs = {n: b.clone() for n, b in ts.model.named_buffers()}
  host = _host_state(ts)
  with ts.ema_weights() as inside:
    assert inside is ts
    assert torch.equal(ts.optim_G.flat_p, avg) and torch.equal(ts.optim_G.ema, live)
    names = dict(ts.model.G.named_parameters())
    sd_avg = ts.ema_state_dict()
    assert all(torch.equal(names[k].data, sd_avg[k]) for k in names)          # parameter by parameter, the average
    assert torch.equal(ts.optim_D.flat_p, pD)
    assert all(torch.equal(b, bufs[n]) for n, b in ts.model.named_buffers())
    got = _sample(StyleTransferSampler(ts.model, num_styles=S_, use_graphs=False))
    want = _sample(StyleTransferSampler(fresh, num_styles=S_, use_graphs=False))
    _same_samples(got, want)
    assert all(torch.equal(b, bufs[n]) for n, b in ts.model.named_buffers())
    with pytest.raises(RuntimeError, match='ema_weights'):
      ts.step(*[_batch()[i] for i in (0, 2, 1, 3)], kind='G')
    with pytest.raises(RuntimeError, match='re-entrant'):
      with ts.ema_weights():
        pass
    assert torch.equal(ts.optim_G.flat_p, avg)               # the refused calls changed nothing
  assert torch.equal(ts.optim_G.flat_p, live) and torch.equal(ts.optim_G.ema, avg)
  # the eval forward on the live weights differs from the one on the average: the caches followed both ways
  back = _sample(StyleTransferSampler(ts.model, num_styles=S_, use_graphs=False))
  assert not torch.equal(back[0][1], got[0][1])
  _set_host_state(ts, host)
  tail = _steps(ts, ['G', 'D'])
  straight = _run(precision, True, DECAY, steps=6)
  assert tail == straight['rows'][4:6]
  now = _state(ts)
  for name in ('pG', 'mG', 'vG', 'pD', 'mD', 'vD', 'ema'):
    assert torch.equal(now[name], straight[name]), name


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_a_captured_sampler_follows_the_weights(precision):
  from mix_stage_amd.checkpoint import load_weights
  from mix_stage_amd.sample import StyleTransferSampler
  ts = _trainer(precision, True, DECAY)
  _steps(ts, ['G', 'D', 'G', 'D'])
  sampler = StyleTransferSampler(ts.model, num_styles=S_, use_graphs=True)
  first = _sample(sampler)                                 # captures on the live weights
  assert len(sampler._graphs) == 1
  fresh = _fresh_model_on_the_average(ts, precision)
  on_avg = _sample(StyleTransferSampler(fresh, num_styles=S_, use_graphs=False))
  assert not torch.equal(on_avg[0][1], first[0][1])
  with ts.ema_weights():
    _same_samples(_sample(sampler), on_avg)
  _same_samples(_sample(sampler), first)
  assert len(sampler._graphs) == 1                         # replays of the one capture throughout
  # other weights through load_weights: the same graph, their output
  load_weights(ts.model, {k: v.clone() for k, v in fresh.state_dict().items()})
  _same_samples(_sample(sampler), on_avg)
  assert len(sampler._graphs) == 1


def test_save_weights_ema_writes_the_average_for_g_and_live_values_for_the_rest(tmp_path):
  from mix_stage_amd.checkpoint import load_weights, save_weights
  ts = _trainer('fp32', True, DECAY)
  _steps(ts, ['G', 'D', 'G'])
  path = tmp_path / 'ema_weights.p'
  save_weights(ts.model, path, train_step=ts, ema=True)
  fresh = _hip(M_, S_)
  load_weights(fresh, path, strict=True)
  live, avg = ts.model.state_dict(), ts.ema_state_dict()
  g_params = set('G.' + n for n, _ in ts.model.G.named_parameters())
  got, moved = fresh.state_dict(), 0
  for k, v in live.items():
    if k in g_params:
      assert torch.equal(got[k], avg[k[2:]]), k
      moved += int(not torch.equal(got[k], v))
    else:
      assert torch.equal(got[k], v), k
  assert moved > 10                                        # the average really differs from the live weights
  plain = tmp_path / 'live_weights.p'
  save_weights(ts.model, plain, train_step=ts)
  on_disk = torch.load(plain, weights_only=True)
  assert all(torch.equal(v.cpu(), on_disk[k]) for k, v in live.items())
  with pytest.raises(ValueError, match='ema_decay'):
    save_weights(ts.model, path, train_step=_trainer('fp32', False, None), ema=True)


@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'eager'])
def test_a_run_resumes_from_optimizer_state(graph):
  """G, D, G; the caller's checkpoint (weights, optimizer_state(), its own host state); a FRESH model and trainer run D, G, G from
  it and end where the uninterrupted six steps end, bit for bit."""
  ts = _trainer('fp32', graph, DECAY)
  _steps(ts, ['G', 'D', 'G'])
  snap = {k: v.clone() for k, v in ts.model.state_dict().items()}
  ost, host = ts.optimizer_state(), _host_state(ts)
  assert ost['G']['ema'] is not None and ost['D']['ema'] is None and not ost['G']['exp_avg'].is_cuda
  assert ost['G']['step_state'] == (2, 0) and ost['D']['step_state'] == (1, 0) and ost['G']['host_step'] == 2
  tail = _steps(ts, ['D', 'G', 'G'])
  want = _state(ts)
  ts2 = _trainer('fp32', graph, DECAY)
  ts2.model.load_state_dict(snap)
  ts2.set_optimizer_state(ost)
  _set_host_state(ts2, host)
  assert _steps(ts2, ['D', 'G', 'G']) == tail
  got = _state(ts2)
  for name in ('pG', 'mG', 'vG', 'pD', 'mD', 'vD', 'ema'):
    assert torch.equal(got[name], want[name]), name
  assert got['clockG'] == want['clockG'] and got['clockD'] == want['clockD']
  # refusals
  bad = ts.optimizer_state()
  bad['G']['total'] += 64
  with pytest.raises(ValueError):
    ts2.set_optimizer_state(bad)
  no_avg = _trainer('fp32', False, None)
  with pytest.raises(ValueError, match='average'):
    no_avg.set_optimizer_state(ost)
  with pytest.raises(ValueError, match='average'):
    ts2.set_optimizer_state(no_avg.optimizer_state())
  with pytest.raises(ValueError):
    short = ts.optim_G.optimizer_state()
    short['exp_avg'] = short['exp_avg'][:-64]
    ts2.optim_G.set_optimizer_state(short)
  assert torch.equal(ts2.optim_G.ema, want['ema'])         # a refused state wrote nothing
  with pytest.raises(RuntimeError):
    no_avg.ema_state_dict()
  with pytest.raises(RuntimeError):
    with no_avg.ema_weights():
      pass
