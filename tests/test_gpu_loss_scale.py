"""GPU: dynamic loss scaling for fp16 training -- the scaled optimizer entry point against the unscaled one bit for bit, its state
machine against the Python mirror word for word, the trainer's surface, eager == captured steps through an overflow skip, fp16
against bf16 at step level, and a short training run."""
import math

import pytest
import torch

from oracle import mixstage_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BETAS, EPS, LR, MAX_NORM = (0.9, 0.999), 1e-8, 1e-4, 1.0


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
  """p, g, m, v, norm and the segment tables of a flat buffer of n elements, optionally on views offset by one float."""

  def __init__(self, n, seg_sizes, seg_first, offset=0, seed=0):
    from mix_stage_amd import ops
    gen = torch.Generator().manual_seed(seed)
    self.n = n
    self.bufs = [torch.zeros(n + offset, dtype=torch.float32, device=DEV) for _ in range(4)]
    self.p, self.g, self.m, self.v = [b[offset:] for b in self.bufs]
    self.p.copy_(torch.randn(n, generator=gen))
    seg = torch.cat([torch.full((s // 64,), i, dtype=torch.int32) for i, s in enumerate(seg_sizes)])
    assert sum(seg_sizes) == n and all(s % 64 == 0 for s in seg_sizes)
    self.seg_of_chunk = seg.to(DEV)
    self.seg_first = torch.tensor(seg_first, dtype=torch.int32, device=DEV)
    self.seg_scratch = torch.zeros(2 * len(seg_sizes), dtype=torch.float32, device=DEV)
    self.norm = torch.zeros(1, dtype=torch.float32, device=DEV)
    self.partials = torch.zeros(ops.lib().ms_reduce_partials_count(n), dtype=torch.float32, device=DEV)
    self.step_state = torch.zeros(4, dtype=torch.int32, device=DEV)

  def step(self, g, ls=None, rule=None, norm=None, meeting_table=None):
    from mix_stage_amd import ops
    self.g.copy_(g)
    if norm is None:
      ops.grad_norm(self.g, self.norm, self.partials)
    else:
      self.norm.fill_(norm)
    args = (self.p, self.g, self.m, self.v, self.norm, MAX_NORM, LR, BETAS[0], BETAS[1], EPS, self.step_state, self.seg_of_chunk,
            self.seg_first, self.seg_scratch)
    if ls is None:
      ops.adam_step_segmented(*args)
    else:
      ops.adam_step_segmented_scaled(*args, ls, rule.growth_interval, rule.min, rule.max, meeting_table)


@pytest.mark.parametrize('n,sizes,first,offset', [(64 * 37, (64 * 10, 64 * 20, 64 * 7), (1, -1, 2), 0), (64, (64,), (1,), 1)],
                         ids=['n2368_3seg_one_idle', 'n64_offset_scalar_path'])
def test_scaled_step_on_scaled_gradients_equals_the_plain_step_bit_for_bit(n, sizes, first, offset):
  """S = 2^k only rescales: ms_sqnorm returns exactly S * ||g||, the un-scaled norm and the coefficient are exact rescalings and
  (S g)(coef / S) rounds like g coef -- so p, m, v, the step word and the written-back norm equal ms_adam_step_segmented's on g."""
  from mix_stage_amd.loss_scale import LossScaleRule
  gen = torch.Generator().manual_seed(5)
  grads = []
  for _ in range(3):
    g = torch.randn(n, generator=gen) * 10.0 ** (-4.0 * torch.rand(n, generator=gen))
    if len(sizes) == 3:
      g[sizes[0]:sizes[0] + sizes[1]] = 0.0           # the segment that never receives a gradient
    grads.append(g.to(DEV))
  ref = _Flat(n, sizes, first, offset)
  ref_norms = []
  for g in grads:
    ref.step(g)
    ref_norms.append(ref.norm.clone())
  assert int(ref.step_state[0]) == 3 and not torch.equal(ref.p, _Flat(n, sizes, first, offset).p)
  if len(sizes) == 3:
    lo, hi = sizes[0], sizes[0] + sizes[1]
    assert torch.equal(ref.p[lo:hi], _Flat(n, sizes, first, offset).p[lo:hi]) and not ref.m[lo:hi].any()    # skipped as torch skips grad None
  for S in (1.0, 2.0 ** 8, 2.0 ** 16):
    rule = LossScaleRule(S)
    got = _Flat(n, sizes, first, offset)
    ls = _ls_words(S)
    for g, rn in zip(grads, ref_norms):
      got.step(g * S, ls, rule)
      assert torch.equal(got.norm, rn), (S, float(got.norm), float(rn))
    for name in ('p', 'm', 'v'):
      assert torch.equal(getattr(got, name), getattr(ref, name)), (S, name)
    assert int(got.step_state[0]) == 3 and got.step_state.tolist()[2:] == [0, 0]
    assert torch.equal(ls.cpu(), _ls_words(S, good=3).cpu())
    for b in got.bufs:                                  # nothing in front of an offset view was touched
      assert offset == 0 or float(b[0]) == 0.0


def test_state_machine_follows_the_python_mirror_word_for_word():
  from mix_stage_amd.loss_scale import LossScaleRule, state_words
  rule = LossScaleRule(dict(init=8, growth_interval=3, min=2, max=32))
  n, sizes = 64 * 4, (64 * 3, 64)
  fl = _Flat(n, sizes, (1, 1))
  g = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(DEV)
  st = rule.initial_state()
  ls = _ls_words(st['scale'])
  bad_steps, scales = 0, []
  seq = ['F'] * 9 + ['N'] * 5 + ['F']
  for i, c in enumerate(seq):
    before = [t.clone() for t in (fl.p, fl.m, fl.v)]
    S_in = st['scale']
    raw = 3.0 * S_in if c == 'F' else (float('inf'), float('nan'), -float('inf'))[i % 3]
    fl.step(g * S_in, ls, rule, norm=raw)
    st, applied, bad = rule.step(st, c == 'F')
    bad_steps += int(bad)
    scales.append(st['scale'])
    f, ints = state_words(st)
    w = ls.cpu()
    assert tuple(w.view(torch.float32)[0:2].tolist()) == f and tuple(w[2:8].tolist()) == ints, (i, c, w.tolist(), st)
    assert fl.step_state.tolist()[0] == i + 1 and fl.step_state.tolist()[2:] == [0 if applied else 1, bad_steps], (i, fl.step_state.tolist())
    same = all(torch.equal(a, b) for a, b in zip(before, (fl.p, fl.m, fl.v)))
    assert same == (not applied), (i, c)
    if c == 'F':
      assert float(fl.norm) == 3.0                    # the true norm, written back
  assert scales == [8, 8, 16, 16, 16, 32, 32, 32, 32, 16, 8, 4, 2, 2, 2]
  assert st['overflow_skips'] == 4 and bad_steps == 1   # the fifth N, at the floor: a bad step, not an overflow skip


def test_a_raised_meeting_error_word_is_a_bad_step_at_any_scale_and_the_scale_stays():
  """The error word of an in-launch meeting is written by hand (no launch waits for anything): a non-finite step behind it is a bad
  step -- step word 3 -- that neither halves the scale nor counts as an overflow skip; once the word is cleared the same norm is an
  overflow skip again; a finite step is applied whatever the word says.  The table may hold unused (zero) entries."""
  from mix_stage_amd.loss_scale import LossScaleRule, state_words
  rule = LossScaleRule(dict(init=8, growth_interval=3, min=2, max=32))
  fl = _Flat(64 * 4, (64 * 3, 64), (1, 1))
  g = torch.randn(fl.n, generator=torch.Generator().manual_seed(2)).to(DEV)
  words = [torch.zeros(4, dtype=torch.int32, device=DEV) for _ in range(2)]
  table = torch.tensor([words[0].data_ptr(), 0, words[1].data_ptr(), 0], dtype=torch.int64, device=DEV)
  st, ls, bad_steps = rule.initial_state(), _ls_words(8.0), 0
  #          norm          error word raised in buffer   (None: none)
  seq = [(3.0, None), (float('inf'), 1), (float('nan'), 0), (float('inf'), None), (3.0, 1), (float('inf'), None)]
  for i, (raw, which) in enumerate(seq):
    for w in words:
      w.zero_()
    if which is not None:
      words[which][0] = 7
    before = [t.clone() for t in (fl.p, fl.m, fl.v)]
    finite = raw == 3.0
    fl.step(g * st['scale'], ls, rule, norm=raw * st['scale'] if finite else raw, meeting_table=table)
    st, applied, bad = rule.step(st, finite, meeting_error=which is not None)
    bad_steps += int(bad)
    f, ints = state_words(st)
    w = ls.cpu()
    assert tuple(w.view(torch.float32)[0:2].tolist()) == f and tuple(w[2:8].tolist()) == ints, (i, w.tolist(), st)
    assert fl.step_state.tolist()[2:] == [0 if applied else 1, bad_steps], (i, fl.step_state.tolist())
    assert all(torch.equal(a, b) for a, b in zip(before, (fl.p, fl.m, fl.v))) == (not applied), i
    assert [int(x[0]) for x in words] == [7 if which == k else 0 for k in range(2)]          # the words are only read
  assert (st['scale'], st['overflow_skips'], bad_steps) == (2.0, 2, 2)       # 8 -(word)- 8 -(word)- 8 -> 4 ... -> 2


@pytest.mark.parametrize('use_graphs', [False, True], ids=['eager', 'graph'])
def test_trainer_reports_a_raised_meeting_word_at_once_and_keeps_the_scale(use_graphs):
  """Trainer level: the error word of every sync buffer the step uses is raised by hand, and the step's pose carries a NaN so that
  the step is not finite whatever the launches make of the word.  Without the word this is an overflow skip (the test above this
  one in the file); with it, it is a bad step -- reported by check_health as without a scale -- and the scale stays at 2^16."""
  import warnings
  from mix_stage_amd import ops16
  from mix_stage_amd.train_step import MixStageTrainStep
  M = S = 2
  audio, pose, labels, style = [t.to(DEV) for t in O.synthetic_batch(4, M=M, S=S, seed=11)]
  bad_pose = pose.clone()
  bad_pose[1, 5, 7] = float('nan')
  ts = MixStageTrainStep(_hip(M, S, 'fp16'), use_graphs=use_graphs, loss_scale='dynamic')
  ts.on_bad_step = 'skip'
  og = ts.optim_G
  ts.step(audio, labels, pose, style, kind='G')
  torch.cuda.synchronize()
  assert ops16._bn_sync and ts.loss_scale()['G'] == dict(scale=65536.0, good_steps=1, overflow_skips=0)
  snap = [t.clone() for t in (og.flat_p, og.exp_avg, og.exp_avg_sq)]
  for b in ops16._bn_sync.values():
    b[0] = 1
  with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter('always')
    ts.step(audio, labels, bad_pose, style, kind='G')
    torch.cuda.synchronize()
    assert og.step_state.tolist()[2:] == [1, 1] and int(og.ls_state[4]) == 0
    assert ts.loss_scale()['G'] == dict(scale=65536.0, good_steps=0, overflow_skips=0)
    ts.check_health()                                   # 'skip': warns, clears the words and re-arms the counters
  assert ts.skipped_steps == 1 and any('refused' in str(w.message) and 'meeting' in str(w.message) for w in caught)
  assert all(torch.equal(a, b) for a, b in zip(snap, (og.flat_p, og.exp_avg, og.exp_avg_sq)))
  assert not ops16.bn_sync_error()
  ts.step(audio, labels, pose, style, kind='G')         # training goes on, at the scale it had
  torch.cuda.synchronize()
  ts.check_health()
  assert ts.skipped_steps == 1 and not torch.equal(og.flat_p, snap[0]) and torch.isfinite(og.flat_p).all()
  assert ts.loss_scale()['G'] == dict(scale=65536.0, good_steps=1, overflow_skips=0)


def test_trainer_surface():
  from mix_stage_amd.train_step import MixStageTrainStep
  ts = MixStageTrainStep(_hip(2, 2, 'fp16'), use_graphs=False, loss_scale='dynamic')
  want = dict(scale=65536.0, good_steps=0, overflow_skips=0)
  assert ts.loss_scale() == {'G': want, 'D': want}
  assert ts.optim_G.seed().dim() == 0 and ts.optim_G.seed().dtype == torch.float32 and float(ts.optim_G.seed()) == 65536.0
  assert ts.optim_G.seed().data_ptr() == ts.optim_G.ls_state.data_ptr() != ts.optim_D.seed().data_ptr()
  ts.optim_D.set_loss_scale_state(dict(scale=512.0, good_steps=7, overflow_skips=3))
  assert ts.loss_scale()['D'] == dict(scale=512.0, good_steps=7, overflow_skips=3) and float(ts.optim_D.seed()) == 512.0
  ts.optim_D.reset_state()
  assert ts.loss_scale()['D'] == want
  for bad in (dict(scale=3.0, good_steps=0, overflow_skips=0), dict(scale=8.0, good_steps=-1, overflow_skips=0),
              dict(scale=8.0, good_steps=0, overflow_skips=1.5)):
    with pytest.raises(ValueError):
      ts.optim_D.set_loss_scale_state(bad)
  assert ts.loss_scale()['D'] == want                                           # a rejected state wrote nothing
  st = MixStageTrainStep(_hip(2, 2, 'fp16'), use_graphs=False, loss_scale=1024.0)
  assert st.loss_scale()['G']['scale'] == 1024.0 and (st.optim_G.loss_scale.min, st.optim_G.loss_scale.growth_interval) == (1024.0, 0)
  with pytest.raises(ValueError):
    MixStageTrainStep(_hip(2, 2, 'fp16'), use_graphs=False, loss_scale=1000.0)
  for dtype in ('bf16', None):
    with pytest.raises(ValueError):
      MixStageTrainStep(_hip(2, 2, dtype), use_graphs=False, loss_scale='dynamic')
  with pytest.raises(NotImplementedError):
    MixStageTrainStep(_hip(2, 2, 'fp16'), use_graphs=False, loss_scale='dynamic', bn_sync='global')
  with pytest.raises(NotImplementedError):
    MixStageTrainStep(_hip(2, 2, 'fp16'), use_graphs=False)                     # without the option: refused as before
  plain = MixStageTrainStep(_hip(2, 2, 'bf16'), use_graphs=False)
  assert plain.optim_G.ls_state is None
  with pytest.raises(RuntimeError):
    plain.loss_scale()


def test_eager_equals_graph_and_an_overflow_skip_is_not_a_bad_step():
  from mix_stage_amd.train_step import MixStageTrainStep
  M = S = 2
  audio, pose, labels, style = [t.to(DEV) for t in O.synthetic_batch(4, M=M, S=S, seed=11)]
  bad_pose = pose.clone()
  bad_pose[1, 5, 7] = float('nan')
  kinds = ['G', 'D', 'G', 'G', 'D', 'D']
  results = {}
  for use_graphs in (False, True):
    ts = MixStageTrainStep(_hip(M, S, 'fp16'), use_graphs=use_graphs, loss_scale='dynamic')
    assert ts.on_bad_step == 'raise'
    og, od = ts.optim_G, ts.optim_D
    for i, k in enumerate(kinds):
      if i == 2:
        snap = [t.clone() for t in (og.flat_p, og.exp_avg, og.exp_avg_sq)]
        before = ts.loss_scale()
      if i == 3:
        p3 = og.flat_p.clone()
      ts.step(audio, labels, bad_pose if i == 2 else pose, style, kind=k)
      if i == 2:
        after = ts.loss_scale()
        assert all(torch.equal(a, b) for a, b in zip(snap, (og.flat_p, og.exp_avg, og.exp_avg_sq))), 'the skipped step moved G'
        assert after['G']['overflow_skips'] == before['G']['overflow_skips'] + 1 == 1, (before, after)
        assert after['G']['scale'] == before['G']['scale'] / 2 and after['G']['good_steps'] == 0 and after['D'] == before['D'], (before, after)
        assert og.step_state.tolist()[2:] == [1, 0] and int(og.ls_state[4]) == 1
      if i == 3:
        assert not torch.equal(og.flat_p, p3) and torch.isfinite(og.flat_p).all() and int(og.ls_state[4]) == 0
    torch.cuda.synchronize()
    ts.check_health()                                   # raises on a bad step: an overflow skip is none
    assert ts.skipped_steps == 0 and not ts.degraded
    assert og.step_count == 3 and od.step_count == 3    # a skipped step advances the step clocks
    results[use_graphs] = dict(pG=og.flat_p.clone(), mG=og.exp_avg.clone(), vG=og.exp_avg_sq.clone(), pD=od.flat_p.clone(),
                               mD=od.exp_avg.clone(), vD=od.exp_avg_sq.clone(), lsG=og.ls_state.clone(), lsD=od.ls_state.clone(),
                               losses=[float(l) for l in ts.losses])
  print('scale states: G %s  D %s' % (results[True]['lsG'].tolist(), results[True]['lsD'].tolist()))
  for name, v in results[False].items():
    w = results[True][name]
    assert (v == w) if name == 'losses' else torch.equal(v, w), name


def test_fp16_is_the_more_accurate_16bit_mode_at_step_level():
  """One G-step each on seeds 3, 7, 11 from identical weights, against the fp32 HIP path: e = relative L2 distance of the unscaled G
  gradient over the live prefix, l = pose L1 of fake_pose.  Asserted: sum e and sum l of fp16 + dynamic scaling do not exceed bf16's.
  fp16 with a static scale of 1 (no scaling at all) is printed beside them, not asserted."""
  from mix_stage_amd.train_step import MixStageTrainStep
  M = S = 2
  seeds = (3, 7, 11)
  batches = [[t.to(DEV) for t in O.synthetic_batch(4, M=M, S=S, seed=s)] for s in seeds]
  configs = [('fp32', None, None), ('bf16', 'bf16', None), ('fp16_dynamic', 'fp16', 'dynamic'), ('fp16_static_1', 'fp16', 1.0)]
  out = {}
  for name, dtype, ls in configs:
    model = _hip(M, S, dtype)
    ts = MixStageTrainStep(model, use_graphs=False, **({'loss_scale': ls} if ls is not None else {}))
    og = ts.optim_G
    rows = []
    for audio, pose, labels, style in batches:
      model.load_state_dict(O.deterministic_state(model.state_dict()))
      og.reset_state(); ts.optim_D.reset_state()
      S_in = float(og.seed()) if ls is not None else 1.0
      ts.step(audio, labels, pose, style, kind='G')
      live = og.live_elems(og.active_params())
      rows.append(dict(g=og.flat_g[:live].double() / S_in, fake=ts.fake_pose.detach().double().clone(), norm=float(og.norm)))
      if name == 'fp16_dynamic':
        st = og.loss_scale_state()
        assert st['overflow_skips'] == 0 and og.step_state.tolist()[2:] == [0, 0], (name, st)     # no step here is skipped
        assert st['scale'] == S_in
    out[name] = rows
  ref = out['fp32']
  for r in ref:
    assert math.isfinite(r['norm']) and r['norm'] > 0 and math.isfinite(float(r['g'].norm())) and float(r['g'].norm()) > 0
  assert len({r['g'].numel() for rows in out.values() for r in rows}) == 1
  e, l = {}, {}
  for name in ('bf16', 'fp16_dynamic', 'fp16_static_1'):
    e[name] = [float((r['g'] - q['g']).norm() / q['g'].norm()) for r, q in zip(out[name], ref)]
    l[name] = [float((r['fake'] - q['fake']).abs().mean()) for r, q in zip(out[name], ref)]
    print('%-14s grad rel-L2 per seed %s sum %.4g | pose L1 per seed %s sum %.4g' %
          (name, ['%.4g' % x for x in e[name]], sum(e[name]), ['%.4g' % x for x in l[name]], sum(l[name])))
  assert all(math.isfinite(x) for x in e['fp16_dynamic'] + e['bf16'] + l['fp16_dynamic'] + l['bf16'])
  assert sum(l['fp16_dynamic']) <= sum(l['bf16']), (l['fp16_dynamic'], l['bf16'])
  assert sum(e['fp16_dynamic']) <= sum(e['bf16']), (e['fp16_dynamic'], e['bf16'])


def test_fp16_trains_30_captured_steps_with_dynamic_scaling():
  """Reference coin flip, B = 4: every loss finite, no bad step, and at most one overflow skip in the last 10 steps -- once a scale
  is under its overflow threshold it cannot grow back within 2000 steps; one step is slack."""
  from mix_stage_amd.train_step import MixStageTrainStep
  M = S = 2
  torch.manual_seed(17)
  audio, pose, labels, style = [t.to(DEV) for t in O.synthetic_batch(4, M=M, S=S, seed=21)]
  ts = MixStageTrainStep(_hip(M, S, 'fp16'), use_graphs=True, loss_scale='dynamic')
  p0 = (ts.optim_G.flat_p.clone(), ts.optim_D.flat_p.clone())
  traj = []
  for i in range(30):
    k = ts.step(audio, labels, pose, style)
    losses = [float(x) for x in ts.losses]
    assert all(math.isfinite(x) for x in losses), (i, k, losses)
    st = ts.loss_scale()
    traj.append((i, k, st['G']['scale'], st['D']['scale'], st['G']['overflow_skips'] + st['D']['overflow_skips'], round(losses[0], 4)))
  for row in traj:
    print('step %2d %s  S_G %-8g S_D %-8g overflow skips %d  loss0 %s' % row)
  ts.check_health()
  assert ts.skipped_steps == 0
  assert int(ts.optim_G.step_state[3]) == 0 and int(ts.optim_D.step_state[3]) == 0
  assert {r[1] for r in traj} == {'G', 'D'}
  assert traj[29][4] - traj[19][4] <= 1, traj
  assert not torch.equal(ts.optim_G.flat_p, p0[0]) and not torch.equal(ts.optim_D.flat_p, p0[1])
  assert torch.isfinite(ts.optim_G.flat_p).all() and torch.isfinite(ts.optim_D.flat_p).all()
