"""GPU: style mixing -- float style weights on the HIP path (ms_concat_style_soft_fwd/bwd behind ops.concat_style_soft), in the
generator (every 'lin' case of JointLateClusterSoftStyle4_G.forward), in the trainer (argmax=0 / softmax=0) and in the sampler
(StyleTransferSampler.sample_mixed).

Kernel level: float64 of the same formula is the reference; the bar is DESIGN section 2's rule for an entry point without a bar of
its own -- the device error, relative to the largest reference value and element by element (relative to |ref| + rms(ref)), stays
within 4x the error of a float32 evaluation of the same formula on the host (with the floor of two float32 roundings that
tests/test_gpu_ew_parity.py uses).  Copies (dx, the content channels of out) and one-hot rows are exact.
Model level: the fp64 oracle, at the bars of test_gpu_model._compare_step."""
import functools

import pytest
import torch

from oracle import mixstage_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FLOOR = 2.0 * 2.0 ** -24
M_ = S_ = 3


# ------------------------------------------------------------------------------------------------ kernel level
def _two_metrics(got, ref):
  got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
  assert got.shape == ref.shape, (got.shape, ref.shape)
  assert bool(torch.isfinite(got).all()), 'non-finite values in the device result'
  d = (got - ref).abs()
  rms = ref.pow(2).mean().sqrt()
  return (d.max() / (ref.abs().max() + 1e-30)).item(), (d / (ref.abs() + rms + 1e-30)).max().item()


def _derived(name, got, ref, ref32, rows):
  mx, el = _two_metrics(got, ref)
  ymx, yel = _two_metrics(ref32, ref)
  rows += [(name + ' max', mx, 4 * max(ymx, FLOOR), ymx), (name + ' elem', el, 4 * max(yel, FLOOR), yel)]


def _finish(case, rows):
  for name, v, bar, yard in rows:
    print('MIX %-22s %-12s yardstick %.3e device %.3e bar %.3e' % (case, name, yard, v, bar))
  bad = [(n, v, b) for n, v, b, _ in rows if not v <= b]
  assert not bad, '%s: (check, measured, bar) %s' % (case, bad)


def _formula(x, E, w, gy, dtype):
  """[x ; (w @ E)^T] and its gradients on the host in `dtype`; a (B,S) w is one row per clip."""
  x_, E_, w_ = (t.detach().cpu().to(dtype).requires_grad_() for t in (x, E, w))
  B, _, T = x_.shape
  wf = w_ if w_.dim() == 3 else w_.unsqueeze(1).expand(B, T, w_.shape[-1])
  out = torch.cat([x_, wf.matmul(E_).transpose(2, 1)], dim=1)
  out.backward(gy.detach().cpu().to(dtype))
  return out.detach(), x_.grad, E_.grad, w_.grad


def _inputs(B, C, D, T, S, per_clip, seed):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(B, C, T, generator=g)
  E = torch.randn(S, D, generator=g) + torch.arange(S).float().reshape(S, 1)       # a swapped row moves the result by O(1)
  w = torch.randn((B, S) if per_clip else (B, T, S), generator=g)                    # any float: rows are not normalised
  gy = torch.randn(B, C + D, T, generator=g)
  return x, E, w, gy


def _device_run(x, E, w, gy):
  from mix_stage_amd import ops
  xh, Eh, wh = (t.detach().clone().to(DEV).requires_grad_() for t in (x, E, w))      # fresh leaves, whatever came in
  out = ops.concat_style_soft(xh, Eh, wh)
  out.backward(gy.to(DEV))
  return out.detach(), xh.grad, Eh.grad, wh.grad


def _check_case(case, x, E, w, gy, got=None):
  C = x.shape[1]
  out, dx, demb, dw = got if got is not None else _device_run(x, E, w, gy)
  r = _formula(x, E, w, gy, torch.float64)
  r32 = _formula(x, E, w, gy, torch.float32)
  assert out.shape == r[0].shape and dw.shape == w.shape and demb.shape == E.shape and dx.shape == x.shape
  assert torch.equal(out[:, :C].cpu(), x), 'the content channels are a copy'
  assert torch.equal(dx.cpu(), gy[:, :C]), 'dx is a copy'
  rows = []
  _derived('out', out[:, C:], r[0][:, C:], r32[0][:, C:], rows)
  _derived('demb', demb, r[2], r32[2], rows)
  _derived('dw', dw, r[3], r32[3], rows)
  _finish(case, rows)
  return out, dx, demb, dw


@pytest.mark.parametrize('B,C,D,T,S,per_clip', [
    (32, 256, 10, 64, 25, True),      # forward and dx above the 2048 x 256 cap: the grid-stride loops run (the id twin's ew_table sizes)
    (32, 256, 10, 65, 25, False),
    (2, 5, 3, 7, 1, True),            # one style, one block, odd sizes
    (2, 5, 3, 7, 1, False),
    (3, 7, 17, 9, 9, False),          # D and S one past the groups of loads in flight (16 and 8)
    (3, 7, 17, 300, 9, True),         # D * T and B * T past one pass of the block reductions (1024 terms)
], ids=lambda v: str(v))
def test_kernels_match_fp64(B, C, D, T, S, per_clip):
  assert (B * (C + D) * T + 255) // 256 > 2048 or B < 32
  _check_case('B%d_C%d_D%d_T%d_S%d_%s' % (B, C, D, T, S, 'clip' if per_clip else 'frame'), *_inputs(B, C, D, T, S, per_clip, 7 + T + S))


@pytest.mark.parametrize('per_clip', [True, False])
def test_weights_as_a_slice_of_a_wider_tensor_and_a_style_nobody_uses(per_clip):
  """S = 8 weights as columns 3..10 of a 16-wide tensor (no copy: the strides go to the kernel), one style with weight 0 everywhere:
  its embedding row gets a gradient of exact zeros; the gradient arrives in the wide tensor's columns 3..10 only."""
  from mix_stage_amd import ops
  B, C, D, T, S, unused = 3, 7, 10, 9, 8, 5
  x, E, _, gy = _inputs(B, C, D, T, S, per_clip, 21)
  wide = torch.randn((B, 16) if per_clip else (B, T, 16), generator=torch.Generator().manual_seed(22))
  wide[..., 3 + unused] = 0
  xh, Eh, wideh = (t.to(DEV).requires_grad_() for t in (x, E, wide))
  wh = wideh[..., 3:11]
  assert not wh.is_contiguous() and wh.stride(-1) == 1
  out = ops.concat_style_soft(xh, Eh, wh)
  out.backward(gy.to(DEV))
  gw = wideh.grad
  assert not bool(gw[..., :3].any()) and not bool(gw[..., 11:].any())
  _check_case('slice_%s' % ('clip' if per_clip else 'frame'), x, E, wide[..., 3:11], gy, got=(out.detach(), xh.grad, Eh.grad, gw[..., 3:11]))
  assert not bool(Eh.grad[unused].any()) and bool(Eh.grad[unused - 1].any())
  # an expanded view (stride 0 over T) without a gradient: the per-clip result, bit for bit
  if per_clip:
    with torch.no_grad():
      out_e = ops.concat_style_soft(xh, Eh, wh.unsqueeze(1).expand(B, T, S))
    assert torch.equal(out_e, out)
    w_leaf = wide[..., 3:11].to(DEV).requires_grad_()
    ops.concat_style_soft(xh.detach(), Eh.detach(), w_leaf.unsqueeze(1).expand(B, T, S)).backward(gy.to(DEV))
    assert torch.equal(w_leaf.grad, gw[..., 3:11])


def test_directional_derivative_on_the_small_shape():
  """gradcheck-style: <gradients, v> for a random direction v against the central difference of the float64 formula (exact up to
  rounding: the function is linear in x and bilinear in (w, E), its third derivative vanishes), at the same 4x bar."""
  rows = []
  for per_clip in (True, False):
    B, C, D, T, S = 2, 5, 3, 7, 4
    x, E, w, gy = _inputs(B, C, D, T, S, per_clip, 33)
    g = torch.Generator().manual_seed(34)
    v = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in (x, E, w)]

    def loss(sign, h=2.0 ** -10):
      x_, E_, w_ = (t.double() + sign * h * d for t, d in zip((x, E, w), v))
      wf = w_ if w_.dim() == 3 else w_.unsqueeze(1).expand(B, T, S)
      return (torch.cat([x_, wf.matmul(E_).transpose(2, 1)], dim=1) * gy.double()).sum().item()
    fd = (loss(1) - loss(-1)) / (2 * 2.0 ** -10)
    dirs = lambda grads: sum((gr.detach().cpu().double() * d).sum().item() for gr, d in zip(grads, v))
    dev = dirs(_device_run(x, E, w, gy)[1:])
    host = dirs(_formula(x, E, w, gy, torch.float32)[1:])
    yard = abs(host - fd) / abs(fd)
    rows.append(('clip' if per_clip else 'frame', abs(dev - fd) / abs(fd), 4 * max(yard, FLOOR), yard))
  _finish('directional', rows)


@pytest.mark.parametrize('per_clip', [True, False])
def test_one_hot_weights_equal_the_id_kernel(per_clip):
  from mix_stage_amd import ops
  B, C, D, T, S = 4, 33, 10, 65, 25
  x, E, _, gy = _inputs(B, C, D, T, S, per_clip, 41)
  ids = torch.randint(0, S, (B, 1) if per_clip else (B, T), generator=torch.Generator().manual_seed(42))
  w = torch.nn.functional.one_hot(ids.reshape(B, -1), S).float()
  w = w[:, 0] if per_clip else w
  out, dx, demb, _ = _device_run(x, E, w, gy)
  xh, Eh = x.to(DEV).requires_grad_(), E.to(DEV).requires_grad_()
  out_id = ops.concat_style(xh, Eh, ids.to(DEV).expand(B, T))
  out_id.backward(gy.to(DEV))
  assert torch.equal(out, out_id.detach()) and torch.equal(dx, xh.grad)
  # demb: the same sum in another order (the id kernel skips, the float kernel adds exact zeros) -> the 4x rule, not bits
  r, r32 = _formula(x, E, w, gy, torch.float64)[2], _formula(x, E, w, gy, torch.float32)[2]
  rows = []
  _derived('demb', demb, r, r32, rows)
  _derived('demb of the id kernel', Eh.grad, r, r32, rows)
  _finish('one_hot_%s' % ('clip' if per_clip else 'frame'), rows)


@pytest.mark.parametrize('per_clip', [True, False])
def test_two_runs_and_a_graph_replay_are_bitwise_equal(per_clip):
  """Two eager runs, and one replay of a captured forward + backward.  The capture holds the kernels and nothing else: the forward
  through the op without a tape, the backward through the C entry point the op's backward calls, warm-up and capture on one stream
  (the captured training steps of test_captured_soft_style_steps_equal_eager_steps go through autograd, as the trainer does)."""
  import ctypes
  from mix_stage_amd import _lib, ops
  B, C, D, T, S = 32, 256, 10, 65, 25
  x, E, w, gy = (t.to(DEV) for t in _inputs(B, C, D, T, S, per_clip, 51))
  a = _device_run(x, E, w, gy)
  b = _device_run(x, E, w, gy)
  assert all(p is not q and torch.equal(p, q) for p, q in zip(a, b))
  dx, demb, dw = torch.empty_like(x), torch.empty_like(E), torch.empty_like(w)
  P = lambda t: ctypes.c_void_p(t.data_ptr())

  def run():
    out = ops.concat_style_soft(x, E, w)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().ms_concat_style_soft_bwd(P(gy), P(E), P(w), w.stride(0), 0 if per_clip else w.stride(1), P(dx), P(demb), P(dw),
                                             B, C, D, T, S, stream)
    assert rc == 0, _lib.lib().ms_last_error()
    return out
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side), torch.no_grad():
    out = run()
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  assert all(torch.equal(p, q) for p, q in zip(a, (out, dx, demb, dw)))           # the direct call is what the op's backward does
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=side), torch.no_grad():
    out = run()
  for t in (dx, demb, dw):
    t.zero_()
  torch.cuda.synchronize()
  g.replay()
  torch.cuda.synchronize()
  assert all(torch.equal(p, q) for p, q in zip(a, (out, dx, demb, dw)))


def test_refusals():
  from mix_stage_amd import _lib, ops
  x, E = torch.randn(2, 5, 7, device=DEV), torch.randn(4, 3, device=DEV)
  w = torch.rand(2, 7, 4, device=DEV)
  assert ops.concat_style_soft(x, E, w).shape == (2, 8, 7)
  with pytest.raises(TypeError):
    ops.concat_style_soft(x, E, w.cpu())                            # a CPU tensor
  with pytest.raises((TypeError, _lib.MixStageLibError)):
    ops.concat_style_soft(x.cpu(), E, w)
  with pytest.raises(TypeError):
    ops._ConcatStyleSoftFn.apply(x, E, w.double())                  # float64 outside the float64 boundary
  with pytest.raises(TypeError):
    ops._ConcatStyleSoftFn.apply(x.double(), E, w)
  with pytest.raises(TypeError):
    ops.concat_style_soft(x, E, w[0, 0])                            # rank 1
  with pytest.raises(TypeError):
    ops.concat_style_soft(x, E, torch.rand(2, 7, 5, device=DEV))    # S of the weights != rows of the embedding
  with pytest.raises(TypeError):
    ops.concat_style_soft(x, E, torch.rand(2, 6, 4, device=DEV))    # T
  with pytest.raises(TypeError):
    ops.concat_style_soft(x, E, torch.rand(2, 7, 8, device=DEV)[..., ::2])     # last axis not contiguous
  with pytest.raises(TypeError):
    ops.concat_style_soft(x, E, torch.zeros(2, 7, 4, dtype=torch.int64, device=DEV))
  # the float64 boundary itself: float64 in, float64 out, fp32 arithmetic
  out64 = ops.concat_style_soft(x.double(), E.double(), w.double())
  assert out64.dtype == torch.float64 and torch.equal(out64.float(), ops.concat_style_soft(x, E, w))


# ------------------------------------------------------------------------------------------------ model level
def _hip(precision=None):
  from test_gpu_model import build_hip_gan
  import mix_stage_amd as A
  m = build_hip_gan(M_, S_)
  if precision:
    A.set_compute_dtype(m, precision)
  return m


@functools.lru_cache(maxsize=None)
def _batch(B=2):
  return O.synthetic_batch(B, M=M_, S=S_, seed=77)


def _mixture(shape, seed):
  return torch.softmax(torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2, dim=-1)


def _eval_forward(model, style, dev, dtype):
  audio, pose, labels, _ = _batch()
  kw = O.model_kwargs(style.to(dev))
  kw['sample_flag'] = 1
  with torch.no_grad():
    y, losses, _ = model([audio.to(dev, dtype), labels.to(dev)], pose.to(dev, dtype), **kw)
  return y, [float(l) for l in losses], model.G.labels_cap_soft


@functools.lru_cache(maxsize=None)
def _oracle_eval(per_clip):
  """The fp64 oracle on a random softmax mixture: (weights as the HIP model gets them, pose, losses, labels_cap_soft)."""
  B, T = 2, 64
  w = _mixture((B, S_) if per_clip else (B, T, S_), 5 + per_clip)
  ref = O.build_gan(M=M_, S=S_, dtype=torch.float64).eval()
  y, l, soft = _eval_forward(ref, w.unsqueeze(1).expand(B, T, S_) if per_clip else w, 'cpu', torch.float64)
  return w, y, l, soft.detach()


@pytest.mark.parametrize('per_clip', [False, True])
def test_eval_forward_with_a_mixture_matches_the_oracle(per_clip):
  w, y_ref, l_ref, soft_ref = _oracle_eval(per_clip)
  hip = _hip().eval()
  y, l, soft = _eval_forward(hip, w.float(), DEV, torch.float32)
  l1 = (y.cpu().double() - y_ref).abs().mean().item()
  dl = max(abs(a - b) for a, b in zip(l, l_ref))
  ds = (soft.cpu().double() - soft_ref).abs().max().item()
  print('MIX eval %s: pose L1 %.3e, losses %.3e, labels_cap_soft %.3e' % ('clip' if per_clip else 'frame', l1, dl, ds))
  assert l1 <= 1e-4 and dl <= 1e-4 and ds <= 1e-4 and len(l) == len(l_ref) >= 3
  # the mixture is not a no-op: the fp64 oracle moves the pose by ~7e-2 between a mixture and a single style
  ids = torch.zeros(2, 64, dtype=torch.int64)
  y_id = _eval_forward(hip, ids, DEV, torch.float32)[0]
  assert (y - y_id).abs().mean().item() >= 1e-3


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_one_hot_float_style_is_the_id_forward(precision):
  hip = _hip(None if precision == 'fp32' else precision).eval()
  ids = torch.randint(0, S_, (2, 64), generator=torch.Generator().manual_seed(3))
  y_id, l_id, soft_id = _eval_forward(hip, ids, DEV, torch.float32)
  soft_id = soft_id.clone()
  y, l, soft = _eval_forward(hip, torch.nn.functional.one_hot(ids, S_).float(), DEV, torch.float32)
  assert torch.equal(y, y_id) and l == l_id and torch.equal(soft, soft_id)
  per_clip = ids[:, :1].expand(2, 64)
  y_c = _eval_forward(hip, torch.nn.functional.one_hot(per_clip[:, 0], S_).float(), DEV, torch.float32)[0]
  assert torch.equal(y_c, _eval_forward(hip, per_clip, DEV, torch.float32)[0])


def _labels_of(fn):
  from mix_stage_amd import ops
  ops.timing_enable(True)
  try:
    fn()
    torch.cuda.synchronize()
    rows = ops.timing_report()
  finally:
    ops.timing_enable(False)
  return {r['label']: r['count'] for r in rows if 'concat_style' in r['label']}


def test_a_soft_style_forward_is_one_concat_launch_and_none_with_the_switch_off():
  from mix_stage_amd import ops
  hip = _hip().eval()
  w = _mixture((2, 64, S_), 9).float()
  run = lambda: _eval_forward(hip, w, DEV, torch.float32)[0]
  y = run()
  assert _labels_of(run) == {'ew|ew_concat_style_fwd': 1}
  old = ops.enable_style_soft(False)
  try:
    assert _labels_of(run) == {}
    y_old = run()
  finally:
    ops.enable_style_soft(old)
  assert ops.style_soft_active() and (y - y_old).abs().mean().item() <= 1e-4      # the matmul + cat route: the same pose at the L1 bar


def _compare_soft_step(kind, softmax, seed=1234):
  """test_gpu_model._compare_step with argmax = 0 (the training branch feeds softmax(scores) or, softmax = 0, the scores themselves
  as per-clip style weights): same bars."""
  import mix_stage_amd as A
  from test_gpu_model import _count_kink_flips, _record_block_outputs, _step
  batch = O.synthetic_batch(2, M=M_, S=S_, seed=seed)
  ref = O.build_gan(M=M_, S=S_, dtype=torch.float64)
  hip = _hip()
  for m in (ref, hip):
    m.G.argmax, m.G.softmax = 0, softmax
  rec_r, h_r = _record_block_outputs(ref, lambda m: isinstance(m, O.ConvNormRelu))
  rec_h, h_h = _record_block_outputs(hip, lambda m: isinstance(m, A.ConvNormRelu))
  f_ref, l_ref = _step(ref, [t.double() if t.is_floating_point() else t for t in batch], kind, 'cpu')
  box = []
  launches = _labels_of(lambda: box.extend(_step(hip, batch, kind, DEV)))
  f_hip, l_hip = box
  for h in h_r + h_h:
    h.remove()
  flips = _count_kink_flips(rec_h, rec_r)
  l1 = (f_hip.detach().cpu().double() - f_ref.detach()).abs().mean().item()
  assert l1 <= 1e-4, 'pose L1 %g' % l1
  for a, b in zip(l_hip, l_ref):
    assert abs(float(a) - float(b)) <= 1e-4, (float(a), float(b))
  assert (hip.G.labels_cap_soft.cpu().double() - ref.G.labels_cap_soft.detach()).abs().max().item() <= 1e-4
  assert hip.G_flag == ref.G_flag
  bad, seen = [], set()
  for (n, p), (_, q) in zip(hip.named_parameters(), ref.named_parameters()):
    skipped_by_design = kind == 'G' and n.startswith('D.')
    if q.grad is None:
      if p.grad is not None and p.grad.abs().max().item() != 0 and not skipped_by_design:
        bad.append((n, 'unexpected grad'))
      continue
    if p.grad is None:
      if not skipped_by_design:
        bad.append((n, 'missing grad'))
      continue
    seen.add(n)
    scale = q.grad.abs().max().item()
    diff = p.grad.cpu().double() - q.grad
    err = diff.abs().max().item()
    if n.endswith('conv.bias'):
      if err > 5e-5:
        bad.append((n, err, scale))
      continue
    if not flips:
      if err > 2e-3 * scale + 1e-7:
        bad.append((n, err, scale))
    else:
      l2 = diff.norm().item() / (q.grad.norm().item() + 1e-30)
      if err > 0.15 * scale + 1e-7 or l2 > 3e-2:
        bad.append((n, err, scale, l2))
  assert not bad, 'flips=%d %s' % (flips, bad[:8])
  if kind == 'G':
    # the parameters only this route reaches: the embedding through demb, the style encoder through dw
    named = ['G.style_emb.emb.weight'] + [n for n, _ in hip.named_parameters() if n.startswith('G.pose_style_encoder.')]
    assert len(named) > 1 and all(n in seen for n in named), sorted(set(named) - seen)
    grads = dict(ref.named_parameters())
    assert grads['G.style_emb.emb.weight'].grad.abs().max().item() > 0
    assert any(grads[n].grad.abs().max().item() > 1e-6 for n in named[1:] if not n.endswith('conv.bias'))
  for (k, a), (_, b) in zip(hip.state_dict().items(), ref.state_dict().items()):
    if 'running_' in k:
      assert (a.cpu().double() - b).abs().max().item() <= 1e-4 * (1 + b.abs().max().item()), k
  return launches


@pytest.mark.parametrize('softmax', [1, 0])
@pytest.mark.parametrize('kind', ['G', 'D'])
def test_training_step_with_soft_style_matches_the_oracle(kind, softmax):
  launches = _compare_soft_step(kind, softmax)
  if kind == 'G':
    assert launches == {'ew|ew_concat_style_fwd': 1, 'ew|ew_concat_style_bwd': 1}, launches
  else:
    assert launches.get('ew|ew_concat_style_fwd') == 1, launches


@pytest.mark.parametrize('softmax', [1, 0])
def test_captured_soft_style_steps_equal_eager_steps(softmax):
  from mix_stage_amd.train_step import MixStageTrainStep
  kinds = ['G', 'D', 'G', 'G', 'D', 'G']              # the last three are pure replays
  batches = [[t.to(DEV) for t in O.synthetic_batch(2, M=M_, S=S_, seed=60 + i)] for i in range(3)]
  got = {}
  for use_graphs in (False, True):
    torch.manual_seed(99)
    model = _hip()
    model.G.argmax, model.G.softmax = 0, softmax
    ts = MixStageTrainStep(model, use_graphs=use_graphs)
    w0 = model.G.style_emb.emb.weight.detach().clone()
    seq = []
    for i, k in enumerate(kinds):
      audio, pose, labels, style = batches[i % 3]
      ts.step(audio, labels, pose, style, kind=k)
      seq.append(([float(l) for l in ts.losses], ts.state_checksums()))
    torch.cuda.synchronize()
    got[use_graphs] = (seq, model.G.style_emb.emb.weight.detach().clone())
    assert (got[use_graphs][1] - w0).abs().max().item() >= 1e-4        # the embedding trains (4 Adam steps of ~lr each)
  assert got[True][0] == got[False][0]
  assert torch.equal(got[True][1], got[False][1])


# ------------------------------------------------------------------------------------------------ sampler
N_WIN = 3


def _interval(n=N_WIN):
  audio, pose, labels, _ = O.synthetic_batch(n, M=M_, S=S_, seed=91)
  return audio, labels, pose


def _mixes(T):
  sched = _mixture((T, S_), 13).float()
  return [('own', {1: 1.0}), ('half', {0: 0.5, 2: 0.5}), ('ramp', ('ramp', {0: 1.0}, [0.0, 0.25, 0.75])), ('sched', sched)]


def _sample(sampler, mixes, n=N_WIN, seed=5):
  audio, labels, pose = _interval(n)
  torch.manual_seed(seed)
  return sampler.sample_mixed(audio.to(DEV), labels.to(DEV), pose.to(DEV), mixes)


def test_sample_mixed_matches_the_oracle_and_the_id_form():
  from mix_stage_amd.sample import StyleTransferSampler
  T = N_WIN * 64
  hip = _hip()
  sampler = StyleTransferSampler(hip, num_styles=S_, use_graphs=True)
  mixes = _mixes(T)
  got = _sample(sampler, mixes)
  assert [g[0] for g in got] == ['own', 'half', 'ramp', 'sched']
  ref = O.build_gan(M=M_, S=S_, dtype=torch.float64).eval()
  audio, labels, pose = _interval()
  for (name, spec), (_, y_hip, l_hip) in zip(mixes, got):
    w = sampler.mix_weights(spec, T)
    assert w.shape == (1, T, S_) and w.dtype == torch.float32
    kw = O.model_kwargs(w.double(), T=T)
    kw.update(sample_flag=1, desc='test', description='test')
    with torch.no_grad():
      y_ref, l_ref, _ = ref([audio.double().reshape(1, -1, 128), labels.reshape(1, -1)], pose.double().reshape(1, -1, 104), **kw)
    l1 = (y_hip.cpu().double() - y_ref).abs().mean().item()
    print('MIX sample_mixed %s: pose L1 %.3e' % (name, l1))
    assert y_hip.shape == (1, T, 104) and l1 <= 1e-4, (name, l1)
    assert abs(float(l_hip[0]) - float(l_ref[0])) <= 1e-4
  # {k: 1.0} is sample_interval's result for target style k, bit for bit (graph of the id form against graph of the float form)
  torch.manual_seed(5)
  by_id = sampler.sample_interval(audio.to(DEV), labels.to(DEV), pose.to(DEV), torch.full((N_WIN, 64), 1, dtype=torch.int64, device=DEV),
                                  all_styles=False)
  assert by_id[0][0] is None and torch.equal(by_id[0][1], got[0][1])
  assert len(sampler._graphs) == 2                       # the two forms are keyed apart


def test_sample_mixed_graph_replay_equals_eager_and_captures_once_per_length():
  from mix_stage_amd.sample import StyleTransferSampler
  hip = _hip()
  eager = StyleTransferSampler(hip, num_styles=S_, use_graphs=False)
  graph = StyleTransferSampler(hip, num_styles=S_, use_graphs=True)
  T = N_WIN * 64
  calls = [_mixes(T)[:2], _mixes(T)[2:]]                  # two calls with different mixtures
  captured = None
  for mixes in calls:
    a, b = _sample(eager, mixes), _sample(graph, mixes)
    for (na, ya, la), (nb, yb, lb) in zip(a, b):
      assert na == nb and torch.equal(ya, yb) and [float(v) for v in la] == [float(v) for v in lb]
    assert len(graph._graphs) == 1 and not eager._graphs
    entry = next(iter(graph._graphs.values()))
    assert captured is None or entry['graph'] is captured, 'the second call captured again'
    captured = entry['graph']
    assert entry['static']['style'].shape == (1, T, S_) and entry['static']['style'].dtype == torch.float32
  assert not torch.equal(a[0][1], a[1][1])                # different mixtures, different poses
  # another sequence length: its own graph, the first one kept
  short = [('half', {0: 0.5, 2: 0.5})]
  a, b = _sample(eager, short, n=2), _sample(graph, short, n=2)
  assert torch.equal(a[0][1], b[0][1]) and a[0][1].shape == (1, 128, 104)
  assert len(graph._graphs) == 2 and any(e['graph'] is captured for e in graph._graphs.values())
