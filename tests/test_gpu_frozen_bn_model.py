"""GPU: frozen BatchNorm statistics at the model and trainer level: a G-step and a D-step of GAN(G, D) against the float64
oracle with the matching norm modules in .eval(), MixStageTrainStep(freeze_bn=) eager against graph replay, re-capture after a
freeze_batchnorm call between steps, B = 1 without a single in-launch meeting, a .double() model, bf16 against the fp32 path and fp16 with
dynamic loss scaling.  Golden size B = 4, T = 64, M = S = 8 as tests/test_gpu_model.py, whose
helpers and bars are used as they are: pose L1 <= 1e-4, losses <= 1e-4, gradients within 2e-3 of the parameter's max |grad| on a
flip-free draw (else 3 % relative L2 and a 15 % per-element cap), style-id argmax equal.  A conv bias in front of batch statistics
has the true gradient 0 (5e-5 absolute, as there); in front of FROZEN statistics it is a gradient like any other."""
import pytest
import torch

from oracle import mixstage_oracle as O
from test_gpu_model import DEV, _count_kink_flips, _record_block_outputs, _step, build_hip_gan

pytestmark = pytest.mark.gpu

M = S = 8
B = 4
ENCODERS = ['G.audio_encoder', 'G.unet']


def _freeze_oracle(ref, names):
  """The oracle's norm modules under `names` in .eval(), pinned there: oracle_train_step and _step call model.train()."""
  frozen = set()
  for name in names:
    root = ref if name == '' else ref.get_submodule(name)
    for m in root.modules():
      if isinstance(m, O.ConvNormRelu):
        m.norm.eval()
        m.norm.train = lambda mode=True, _m=m.norm: _m
        frozen.add(m)
  return frozen


def _stir_statistics(hip, ref, seed):
  """Running statistics that are not the initial ones, the same in both models."""
  gen = torch.Generator().manual_seed(seed)
  sd = ref.state_dict()
  with torch.no_grad():
    for k, v in hip.state_dict().items():
      if k.endswith('running_mean'):
        t = 0.1 * torch.randn(v.shape, generator=gen)
      elif k.endswith('running_var'):
        t = 0.5 + torch.rand(v.shape, generator=gen)
      else:
        continue
      v.copy_(t.to(v.device))
      sd[k].copy_(t.to(sd[k].dtype))


@pytest.mark.parametrize('which', ['all', 'encoders'])
@pytest.mark.parametrize('kind', ['G', 'D'])
def test_frozen_step_matches_oracle(which, kind):
  import mix_stage_amd as A
  from mix_stage_amd import layers
  batch = O.synthetic_batch(B, M=M, S=S, seed=77)
  ref = O.build_gan(M=M, S=S, dtype=torch.float64)
  hip = build_hip_gan(M, S)
  _stir_statistics(hip, ref, 5)
  names = [''] if which == 'all' else ENCODERS
  frozen_ref = _freeze_oracle(ref, names)
  for r in layers.freeze_bn_roots(hip, True if which == 'all' else names):
    layers.freeze_batchnorm(r)
  frozen_hip = layers.frozen_batchnorm_blocks(hip)
  assert len(frozen_hip) == len(frozen_ref) > 0
  buf0 = {k: v.clone() for k, v in hip.state_dict().items() if 'norm.' in k and 'weight' not in k and 'bias' not in k}
  rec_r, h_r = _record_block_outputs(ref, lambda m: isinstance(m, O.ConvNormRelu))
  rec_h, h_h = _record_block_outputs(hip, lambda m: isinstance(m, A.ConvNormRelu))
  pse = {}

  def _pse_hook(k):
    def hook(mod, i, o):
      pse.setdefault(k, o.detach().cpu().double())          # the first call of a step: the scores of the ground-truth pose
    return hook
  hooks = [m.G.pose_style_encoder.register_forward_hook(_pse_hook(k)) for k, m in (('ref', ref), ('hip', hip))]
  f_ref, l_ref = _step(ref, [t.double() if t.is_floating_point() else t for t in batch], kind, 'cpu')
  f_hip, l_hip = _step(hip, batch, kind, DEV)
  for h in h_r + h_h + hooks:
    h.remove()
  flips = _count_kink_flips(rec_h, rec_r)
  l1 = (f_hip.detach().cpu().double() - f_ref.detach()).abs().mean().item()
  print(which, kind, 'pose L1 %.3g flips %d' % (l1, flips))
  assert l1 <= 1e-4, 'pose L1 %g' % l1
  for a, b in zip(l_hip, l_ref):
    assert abs(float(a) - float(b)) <= 1e-4, (float(a), float(b))
  assert torch.equal(pse['hip'].argmax(-1), pse['ref'].argmax(-1))
  frozen_bias = set(n + '.conv.bias' for n, m in hip.named_modules() if any(m is f for f in frozen_hip))
  bad = []
  for (n, p), (_, q) in zip(hip.named_parameters(), ref.named_parameters()):
    if q.grad is None or p.grad is None:
      if (q.grad is None) != (p.grad is None or p.grad.abs().max().item() == 0) and not (kind == 'G' and n.startswith('D.')):
        bad.append((n, 'gradient on one side only'))
      continue
    scale = q.grad.abs().max().item()
    diff = p.grad.cpu().double() - q.grad
    err = diff.abs().max().item()
    if n.endswith('conv.bias') and n not in frozen_bias:
      if err > 5e-5:
        bad.append((n, err, scale))
    elif not flips:
      if err > 2e-3 * scale + 1e-7:
        bad.append((n, err, scale))
    else:
      l2 = diff.norm().item() / (q.grad.norm().item() + 1e-30)
      if err > 0.15 * scale + 1e-7 or l2 > 3e-2:
        bad.append((n, err, scale, l2))
  assert not bad, 'flips=%d %s' % (flips, bad[:8])
  # frozen blocks: statistics and batch counts bit-unchanged; the others moved as the oracle's did (the bar of _compare_step)
  after, ref_after = hip.state_dict(), ref.state_dict()
  frozen_prefix = tuple(n + '.norm.' for n, m in hip.named_modules() if any(m is f for f in frozen_hip))
  moved = 0
  for k, v in buf0.items():
    if k.startswith(frozen_prefix):
      assert torch.equal(after[k], v), k
    elif k.endswith('num_batches_tracked'):
      assert int(after[k]) == int(ref_after[k]), k
    else:
      assert (after[k].cpu().double() - ref_after[k]).abs().max().item() <= 1e-4 * (1 + ref_after[k].abs().max().item()), k
      moved += int(not torch.equal(after[k], v))
  assert which == 'all' or moved > 0


def _run_steps(use_graphs, freeze_bn, kinds, batches, refreeze_at=None, **kw):
  from mix_stage_amd import layers
  from mix_stage_amd.train_step import MixStageTrainStep
  torch.manual_seed(99)
  model = build_hip_gan(M, S)
  ts = MixStageTrainStep(model, use_graphs=use_graphs, freeze_bn=freeze_bn, **kw)
  losses = []
  for rep in range(2 if use_graphs else 1):          # (graphs: the second round is pure replay)
    if rep == 1:
      model.load_state_dict(O.deterministic_state(model.state_dict()))
      for o in (ts.optim_G, ts.optim_D):
        o.reset_state()
      if refreeze_at is not None:
        layers.freeze_batchnorm(model.D, False)
      losses = []
    for i, ((audio, pose, labels, style), k) in enumerate(zip(batches, kinds)):
      if i == refreeze_at:
        layers.freeze_batchnorm(model.D)
      ts.step(audio.to(DEV), labels.to(DEV), pose.to(DEV), style.to(DEV), kind=k)
      losses.append([float(l) for l in ts.losses])
  return losses, {k: v.clone() for k, v in model.state_dict().items()}, model, ts


def test_trainer_freeze_bn_graph_equals_eager_and_buffers():
  from mix_stage_amd import layers
  batches = [O.synthetic_batch(B, M=M, S=S, seed=60 + i) for i in range(4)]
  kinds = ['G', 'D', 'G', 'D']
  eager = _run_steps(False, ENCODERS, kinds, batches)
  graph = _run_steps(True, ENCODERS, kinds, batches)
  assert eager[0] == graph[0]
  for k, v in eager[1].items():
    assert torch.equal(v, graph[1][k]), k
  model = eager[2]
  init = O.deterministic_state(model.state_dict())
  frozen = layers.frozen_batchnorm_blocks(model)
  names = {n for n, m in model.named_modules() if any(m is f for f in frozen)}
  assert names and all(n.startswith(('G.audio_encoder', 'G.unet')) for n in names)
  moved = 0
  for k, v in eager[1].items():
    if '.norm.running_' in k or k.endswith('num_batches_tracked'):
      if k.split('.norm.')[0] in names:
        assert torch.equal(v.cpu(), init[k].cpu()), k                # bit-unchanged after four steps
      elif not torch.equal(v.cpu(), init[k].cpu()):
        moved += 1
  assert moved >= 3 * 4                                        # the decoder's, the classifier's, D's ... buffers moved


def test_freezing_between_steps_recaptures():
  """D is frozen after the second step: the captured D-step of before must not be replayed for the fourth."""
  batches = [O.synthetic_batch(B, M=M, S=S, seed=60 + i) for i in range(4)]
  kinds = ['G', 'D', 'G', 'D']
  eager = _run_steps(False, 'G', kinds, batches, refreeze_at=2)
  graph = _run_steps(True, 'G', kinds, batches, refreeze_at=2)
  assert eager[0] == graph[0]
  for k, v in eager[1].items():
    assert torch.equal(v, graph[1][k]), k
  assert len(graph[3]._graphs) >= 4                            # G, D, and both again under the other flags


def test_batch_of_one_everything_frozen_meets_nobody():
  """B = 1, every block frozen.  The G-step differentiates every block, so none of its launches meets inside a launch: with the
  in-launch meetings switched off it is the same step bit for bit.  The D-step's generator pass runs WITHOUT gradients, where a
  frozen block is the eval launch it always was -- the chained eval decoder at T = 64 included, a one-launch form that the
  switch replaces by the blocks one by one: equal to the forward bar of the fp32 kernels (2e-5, test_gpu_kernels), not bitwise."""
  from mix_stage_amd import ops16
  batches = [O.synthetic_batch(1, M=M, S=S, seed=70 + i) for i in range(2)]
  runs = {}
  old = ops16.in_launch_meetings()
  for meetings in (True, False):
    ops16.set_in_launch_meetings(meetings)
    try:
      runs[meetings] = (_run_steps(False, True, ['G'], batches[:1]), _run_steps(False, True, ['D'], batches[1:]))
      ops16.check_meetings()
    finally:
      ops16.set_in_launch_meetings(old)
  (g_on, d_on), (g_off, d_off) = runs[True], runs[False]
  assert g_on[0] == g_off[0]
  for k, v in g_on[1].items():
    assert torch.equal(v, g_off[1][k]), k
  assert all(torch.isfinite(torch.tensor(l)).all() for l in g_on[0] + d_on[0])
  for a, b in zip(d_on[0][0], d_off[0][0]):
    assert abs(a - b) <= 2e-5 * max(abs(b), 1.0), (a, b)


def test_double_model_with_frozen_statistics():
  """A .double() model (fp32 kernels behind float64 boundaries; the trainer's flat optimizer takes float32 parameters only, so the
  step is the model's own forward / backward as in test_gpu_model's .double() test) with every block frozen: the fp32 bars."""
  from mix_stage_amd import layers
  batch = O.synthetic_batch(B, M=M, S=S, seed=81)
  batch64 = [t.double() if t.is_floating_point() else t for t in batch]
  ref = O.build_gan(M=M, S=S, dtype=torch.float64)
  _freeze_oracle(ref, [''])
  hip = build_hip_gan(M, S).double()
  layers.freeze_batchnorm(hip)
  buf0 = {k: v.clone() for k, v in hip.state_dict().items() if 'running_' in k or k.endswith('num_batches_tracked')}
  f_ref, l_ref = _step(ref, batch64, 'G', 'cpu')
  f_hip, l_hip = _step(hip, batch64, 'G', DEV)
  l1 = (f_hip.detach().cpu().double() - f_ref.detach()).abs().mean().item()
  assert f_hip.dtype == torch.float64 and l1 <= 1e-4, l1
  for a, b in zip(l_hip, l_ref):
    assert abs(float(a) - float(b)) <= 1e-4, (float(a), float(b))
  g_h, g_r = hip.G.unet.conv1[0].norm.weight.grad, ref.G.unet.conv1[0].norm.weight.grad
  assert g_h.dtype == torch.float64 and (g_h.cpu() - g_r).abs().max().item() <= 0.15 * g_r.abs().max().item() + 1e-7
  after = hip.state_dict()
  assert all(torch.equal(after[k], v) for k, v in buf0.items())


def _hip16(dtype, freeze):
  import mix_stage_amd as A
  from mix_stage_amd import layers
  model = build_hip_gan(M, S)
  if dtype != 'fp32':
    A.set_compute_dtype(model, dtype)
  if freeze:
    layers.freeze_batchnorm(model)
  return model


@pytest.mark.parametrize('kind', ['G', 'D'])
def test_bf16_frozen_step_against_the_fp32_path(kind):
  """bf16 against the fp32 HIP path of the same frozen model, one step.  The bar is the pose L1 that the UNFROZEN bf16 step
  measures against the unfrozen fp32 step beside it (the comparison of profiles/fp16_train.json); profiles/frozen_bn.json holds
  both figures as measured."""
  batch = O.synthetic_batch(B, M=M, S=S, seed=77)
  l1 = {}
  for freeze in (False, True):
    f32, _ = _step(_hip16('fp32', freeze), batch, kind, DEV)
    f16, losses = _step(_hip16('bf16', freeze), batch, kind, DEV)
    assert all(torch.isfinite(l).all() for l in losses)
    l1[freeze] = (f16.detach().double() - f32.detach().double()).abs().mean().item()
  print('bf16 vs fp32 pose L1, %s-step: frozen %.4g, unfrozen (the bar) %.4g' % (kind, l1[True], l1[False]))
  assert l1[True] <= l1[False], l1


def test_fp16_dynamic_loss_scale_with_frozen_statistics():
  """fp16 with loss_scale='dynamic' and every block frozen: the step applies, the scale state moves as without the option, and the
  table of meeting error words copes with a step that creates no meeting buffer of its own."""
  from mix_stage_amd.train_step import MixStageTrainStep
  batch = O.synthetic_batch(B, M=M, S=S, seed=78)
  audio, pose, labels, style = [t.to(DEV) for t in batch]
  states = {}
  for freeze in (None, True):
    model = _hip16('fp16', False)
    ts = MixStageTrainStep(model, use_graphs=True, loss_scale='dynamic', freeze_bn=freeze)
    p0 = ts.optim_G.flat_p.clone()
    for k in ('G', 'D', 'G'):
      ts.step(audio, labels, pose, style, kind=k)
    torch.cuda.synchronize()
    ts.check_health()
    states[freeze] = ts.loss_scale()
    assert not torch.equal(ts.optim_G.flat_p, p0) and torch.isfinite(ts.optim_G.flat_p).all()
    assert all(torch.isfinite(l).all() for l in ts.losses)
  # the scale state moves by its rule in either run (which steps overflow depends on the gradients, and those differ between a
  # frozen and an unfrozen model): every step is a good step or an overflow skip, each skip halves the scale from 2^16
  for st in states.values():
    for who, steps in (('G', 2), ('D', 1)):
      assert st[who]['good_steps'] + st[who]['overflow_skips'] == steps and st[who]['scale'] == 65536.0 / 2 ** st[who]['overflow_skips'], st
  assert states[True]['G']['good_steps'] >= 1


def test_captured_batch_of_one_and_the_other_trainer_options():
  """A captured B = 1 fully-frozen G- and D-step equal the eager ones bit for bit; freeze_bn composes with lr_schedule, ema_decay and
  on_bad_step (graph == eager, the average moves on G-steps)."""
  b1 = [O.synthetic_batch(1, M=M, S=S, seed=70 + i) for i in range(2)]
  eager = _run_steps(False, True, ['G', 'D'], b1)
  graph = _run_steps(True, True, ['G', 'D'], b1)
  assert eager[0] == graph[0]
  for k, v in eager[1].items():
    assert torch.equal(v, graph[1][k]), k
  batches = [O.synthetic_batch(B, M=M, S=S, seed=60 + i) for i in range(3)]
  from mix_stage_amd.train_step import MixStageTrainStep
  runs = []
  for use_graphs in (False, True):
    torch.manual_seed(99)
    model = build_hip_gan(M, S)
    ts = MixStageTrainStep(model, use_graphs=use_graphs, freeze_bn=ENCODERS, lr_schedule=0.9, ema_decay=0.99)
    ts.on_bad_step = 'skip'
    losses = []
    for i, k in enumerate(['G', 'D', 'G', 'G', 'D']):            # (graphs: the third step on is replay)
      if i == 3:
        ts.epoch_end()
      audio, pose, labels, style = [t.to(DEV) for t in batches[i % 3]]
      ts.step(audio, labels, pose, style, kind=k)
      losses.append([float(l) for l in ts.losses])
    torch.cuda.synchronize()
    ts.check_health()
    assert ts.skipped_steps == 0
    runs.append((losses, ts.lr(), {k: v.clone() for k, v in model.state_dict().items()},
                 {k: v.clone() for k, v in ts.ema_state_dict().items()}))
  assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
  for k, v in runs[0][2].items():
    assert torch.equal(v, runs[1][2][k]), k
  for k, v in runs[0][3].items():
    assert torch.equal(v, runs[1][3][k]), k
  live = dict(runs[0][2])
  assert any(not torch.equal(v, live['G.' + k]) for k, v in runs[0][3].items() if v.is_floating_point() and 'G.' + k in live)
