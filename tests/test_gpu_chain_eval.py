"""GPU: the wait-free eval form of the chained pose decoder (ms_decoder_chain_eval_fwd) -- decoder.0-3 + logits + softmax mixture
for any batch size and sequence length in inference -- against float64 arithmetic, against the blocks one by one, in the 16-bit
modes with and without BatchNorm folding, repeated / replayed / with the in-launch meetings switched off, and through the
sampling driver.  The shapes the one-launch train/eval chain serves keep that kernel."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_gpu_chain import _build, _close, _inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (B, M, T, clips checked against float64)
SHAPES = [(1, 8, 640, 1), (1, 25, 1000, 1), (3, 4, 72, 3), (2, 2, 61, 2), (64, 8, 64, 64), (1024, 8, 64, 48), (5, 1, 200, 5)]
SHAPES16 = [(1, 8, 640, 1), (1024, 8, 64, 48), (3, 3, 72, 3)]
_ids = lambda s: 'b%d_m%d_t%d' % s[:3]


def _segment_eval_float64(blocks, logits, x, score, M, P, round_to=None):
  """The segment in float64 with running-statistics BatchNorm; round_to: operands (weights, input) rounded to a 16-bit type."""
  r = (lambda t: t.detach().to(round_to).double().cpu()) if round_to is not None else (lambda t: t.detach().double().cpu())
  f = lambda t: t.detach().double().cpu()
  B, _, T = x.shape
  h = torch.cat([r(x)] * M, 1)
  for m in blocks:
    c, n = m.conv, m.norm
    h = F.conv1d(h, r(c.weight), f(c.bias), padding=1, groups=M)
    h = (h - f(n.running_mean).view(1, -1, 1)) / torch.sqrt(f(n.running_var).view(1, -1, 1) + n.eps) * f(n.weight).view(1, -1, 1) + f(n.bias).view(1, -1, 1)
    h = F.leaky_relu(h, 0.2)
  z = F.conv1d(h, r(logits.weight), f(logits.bias), groups=M)
  soft = torch.softmax(f(score).transpose(1, 2), -1)
  return torch.einsum('bgpt,btg->btp', z.view(B, M, P, T), soft), soft


def _eval(blocks, logits, x, score, P, eval_form, dt_name=None, folded=False):
  """One eval forward of the segment: through decoder_chain(16) with the eval form switched on, or with it off -- then the
  function must decline and the blocks run one by one."""
  import mix_stage_amd as A
  from mix_stage_amd import ops, ops16
  from mix_stage_amd.layers import bare_conv
  mods = nn.ModuleList(list(blocks) + [logits])
  if dt_name:
    A.set_compute_dtype(mods, dt_name)
  A.set_inference_folding(mods, folded)
  for m in blocks:
    m.eval()
  prev = ops.USE_DECODER_CHAIN_EVAL
  ops.USE_DECODER_CHAIN_EVAL = eval_form
  try:
    with torch.no_grad():
      xin = ops16.to_cb8(x, ops16.NAME_DT[dt_name]) if dt_name else x
      res = (ops16.decoder_chain16 if dt_name else ops.decoder_chain)(xin, blocks, logits, score, P)
      assert (res is not None) == eval_form
      if res is None:
        z = blocks[0].forward_broadcast(xin)
        for m in blocks[1:]:
          z = m(z)
        z = bare_conv(logits, z, out_f32=True)
        res = ops.softmax_mix(z, score, P)
  finally:
    ops.USE_DECODER_CHAIN_EVAL = prev
    A.set_inference_folding(mods, False)
  torch.cuda.synchronize()
  return res


def _running(blocks):
  return [t.clone() for m in blocks for t in (m.norm.running_mean, m.norm.running_var)]


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_eval_form_fp32_against_float64_and_the_blocks(shape):
  """fp32: against the segment in float64 (mean |err| <= 2e-6, max error <= 2e-5 of max |ref| over EVERY frame: a seam or mask
  mistake is an O(1) error in a few frames) and against the blocks one by one; the running statistics are not written."""
  B, M, T, nchk = shape
  P = 104
  blocks, logits = _build(M, P, 10, seed=41)
  x, score = _inputs(B, M, 266, seed=41, T=T)
  before = _running(blocks)
  out, soft = _eval(blocks, logits, x, score, P, True)
  assert out.shape == (B, T, P) and soft.shape == (B, T, M)
  assert all(torch.equal(a, b) for a, b in zip(before, _running(blocks)))
  ref, soft_ref = _segment_eval_float64(blocks, logits, x[:nchk], score[:nchk], M, P)
  got = out[:nchk].cpu().double()
  mean_err = float((got - ref).abs().mean())
  scale = float(ref.abs().max())
  print('%s fp32: mean |err| %.3e, max err %.3e of max |ref| %.3e' % (_ids(shape), mean_err, float((got - ref).abs().max()) / scale, scale))
  assert torch.isfinite(out).all()
  assert mean_err <= 2e-6
  _close(got, ref, 2e-5, 'mixture vs float64')
  _close(soft[:nchk].cpu().double(), soft_ref, 1e-6, 'softmax vs float64')
  out_b, soft_b = _eval(blocks, logits, x, score, P, False)
  assert all(torch.equal(a, b) for a, b in zip(before, _running(blocks)))
  _close(out, out_b, 2e-5, 'mixture vs the blocks one by one')
  _close(soft, soft_b, 1e-6, 'softmax vs the blocks one by one')


@pytest.mark.parametrize('folded', [False, True], ids=['unfolded', 'folded'])
@pytest.mark.parametrize('dt_name', ['bf16', 'fp16'])
@pytest.mark.parametrize('shape', SHAPES16, ids=_ids)
def test_eval_form_16bit_against_float64(shape, dt_name, folded):
  """16-bit: both the eval form and the blocks one by one against exact arithmetic on the rounded operands; the eval form is
  no farther from it than 1.5 x the per-block path (+ 1e-4 of the scale) and inside the dtype's bar.  With folding requested
  the blocks fold the BatchNorm scale into 16-bit weights; the eval form keeps the scale in fp32."""
  B, M, T, nchk = shape
  P = 104 if M != 3 else 16
  extra = 10 if M != 3 else 16
  tdt = torch.bfloat16 if dt_name == 'bf16' else torch.float16
  blocks, logits = _build(M, P, extra, seed=43)
  x, score = _inputs(B, M, 256 + extra, seed=43, T=T)
  out, soft = _eval(blocks, logits, x, score, P, True, dt_name, folded)
  out_b, soft_b = _eval(blocks, logits, x, score, P, False, dt_name, folded)
  ref, _ = _segment_eval_float64(blocks, logits, x[:nchk], score[:nchk], M, P, tdt)
  ea = float((out[:nchk].cpu().double() - ref).abs().mean())
  eb = float((out_b[:nchk].cpu().double() - ref).abs().mean())
  scale = float(ref.abs().mean())
  print('%s %s %s: eval form %.3e, blocks %.3e of mean |out| %.3e' % (_ids(shape), dt_name, 'folded' if folded else 'unfolded', ea, eb, scale))
  assert torch.isfinite(out).all()
  assert ea <= 1.5 * eb + 1e-4 * scale and ea <= (3e-2 if dt_name == 'bf16' else 5e-3) * scale
  _close(soft, soft_b, 1e-6, 'softmax')


@pytest.mark.parametrize('dt_name', [None, 'bf16'], ids=['fp32', 'bf16'])
def test_shapes_of_the_one_launch_chain_keep_it(dt_name):
  """(32, 8, 64) eval: the existing launch runs, whatever the eval switch says -- same bits, and its own timing label."""
  from mix_stage_amd import ops
  B, M, T, P = 32, 8, 64, 104
  blocks, logits = _build(M, P, 10, seed=45)
  x, score = _inputs(B, M, 266, seed=45)
  import mix_stage_amd as A
  from mix_stage_amd import ops16
  if dt_name:
    A.set_compute_dtype(nn.ModuleList(list(blocks) + [logits]), dt_name)
  for m in blocks:
    m.eval()
  fn = ops16.decoder_chain16 if dt_name else ops.decoder_chain
  outs = []
  ops.timing_enable(True)
  try:
    ops.timing_report()
    for on in (True, False):
      prev = ops.USE_DECODER_CHAIN_EVAL
      ops.USE_DECODER_CHAIN_EVAL = on
      try:
        with torch.no_grad():
          xin = ops16.to_cb8(x, ops16.NAME_DT[dt_name]) if dt_name else x
          res = fn(xin, blocks, logits, score, P)
      finally:
        ops.USE_DECODER_CHAIN_EVAL = prev
      assert res is not None
      outs.append(res[0].clone())
    torch.cuda.synchronize()
    labels = [r['label'] for r in ops.timing_report()]
  finally:
    ops.timing_enable(False)
  assert torch.equal(outs[0], outs[1])
  assert any('decoder_chain_fwd' in l for l in labels), labels
  assert not any('decoder_chain_eval_fwd' in l for l in labels), labels
  # train mode outside the one-launch shapes still declines
  for m in blocks:
    m.train()
  if not dt_name:
    x2, score2 = _inputs(2, M, 266, seed=46, T=128)
    assert ops.decoder_chain(x2, blocks, logits, score2, P) is None
    with torch.no_grad():
      assert ops.decoder_chain(x2, blocks, logits, score2, P) is None


def test_eval_form_label_is_its_own():
  from mix_stage_amd import ops
  blocks, logits = _build(4, 104, 10, seed=47)
  x, score = _inputs(2, 4, 266, seed=47, T=100)
  ops.timing_enable(True)
  try:
    ops.timing_report()
    _eval(blocks, logits, x, score, 104, True)
    labels = [r['label'] for r in ops.timing_report()]
  finally:
    ops.timing_enable(False)
  assert any('decoder_chain_eval_fwd' in l for l in labels), labels
  assert not any('decoder_chain_fwd' in l for l in labels), labels


@pytest.mark.parametrize('case', [(1, 8, 640, None), (1024, 8, 64, 'fp16')], ids=['b1_t640_fp32', 'b1024_t64_fp16'])
def test_repeatability_eager_graph_and_meetings_off(case):
  """Same shape -> same bits: 12 eager runs beside a busy side stream, 5 replays of a captured graph, and with the in-launch
  meetings switched off (the eval form meets nobody) -- while (32, 8, 64) eval then declines as it always did."""
  from mix_stage_amd import ops, ops16
  B, M, T, dt_name = case
  P = 104
  blocks, logits = _build(M, P, 10, seed=49)
  x, score = _inputs(B, M, 266, seed=49, T=T)
  first, _ = _eval(blocks, logits, x, score, P, True, dt_name)
  first = first.clone()
  side = torch.cuda.Stream()
  big = torch.randn(32 << 20, device=DEV)
  with torch.cuda.stream(side):
    for _ in range(8):
      big = big * 1.0001 + 0.5
  for rep in range(12):
    out, _ = _eval(blocks, logits, x, score, P, True, dt_name)
    assert torch.equal(out, first), rep
  torch.cuda.synchronize()
  # graph: warm-up on a side stream, capture, replay
  fn = ops16.decoder_chain16 if dt_name else ops.decoder_chain
  with torch.no_grad():
    xin = ops16.to_cb8(x, ops16.NAME_DT[dt_name]) if dt_name else x
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
      fn(xin, blocks, logits, score, P)
    torch.cuda.current_stream().wait_stream(s2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
      res = fn(xin, blocks, logits, score, P)
    assert res is not None
    for rep in range(5):
      g.replay()
      torch.cuda.synchronize()
      assert torch.equal(res[0], first), rep
  ops16.set_in_launch_meetings(False)
  try:
    out, _ = _eval(blocks, logits, x, score, P, True, dt_name)
    assert torch.equal(out, first)
    b32, l32 = _build(8, P, 10, seed=50)
    for m in b32:
      m.eval()
    x32, s32 = _inputs(32, 8, 266, seed=50)
    with torch.no_grad():
      assert ops.decoder_chain(x32, b32, l32, s32, P) is None
  finally:
    ops16.set_in_launch_meetings(True)


@pytest.mark.parametrize('use_graphs', [False, True], ids=['eager', 'graphs'])
def test_sampler_long_sequence_takes_the_eval_form(use_graphs, monkeypatch):
  """StyleTransferSampler.sample_interval on n = 10 windows (T = 640), M = S = 8, all styles: pose L1 vs the float64 oracle
  <= 1e-4, the mixture's argmax as the oracle's wherever its top-2 margin exceeds 1e-4, and decoder_chain serves T = 640."""
  from oracle import mixstage_oracle as O
  from test_gpu_model import build_hip_gan
  from mix_stage_amd import ops
  from mix_stage_amd.sample import StyleTransferSampler
  M = S = 8
  n = 10
  audio, pose, labels, style = O.synthetic_batch(n, M=M, S=S)
  style = torch.full_like(style, 2)
  ref = O.build_gan(M=M, S=S, dtype=torch.float64).eval()
  hip = build_hip_gan(M, S)
  seen = []
  real = ops.decoder_chain

  def spy(x, *a, **k):
    res = real(x, *a, **k)
    seen.append((x.shape[-1], res is not None))
    return res
  monkeypatch.setattr(ops, 'decoder_chain', spy)
  sampler = StyleTransferSampler(hip, num_styles=S, use_graphs=use_graphs)
  torch.manual_seed(5)
  got = sampler.sample_interval(audio.to(DEV), labels.to(DEV), pose.to(DEV), style.to(DEV))
  assert len(got) == S
  assert seen and all(T == n * 64 and served for T, served in seen), seen
  torch.manual_seed(5)
  for (name, y_hip, l_hip), shift in zip(got, range(S)):
    kw = O.model_kwargs(((style + shift) % S).reshape(1, -1), T=n * 64)
    kw.update(sample_flag=1, desc='test', description='test')
    with torch.no_grad():
      y_ref, _, _ = ref([audio.reshape(1, -1, 128).double(), labels.reshape(1, -1)], pose.reshape(1, -1, 104).double(), **kw)
    l1 = (y_hip.cpu().double() - y_ref).abs().mean().item()
    print('sampler n=10 style shift %d: pose L1 vs float64 %.3e' % (shift, l1))
    assert y_hip.shape == (1, n * 64, 104)
    assert l1 <= 1e-4, name
  # the mixture weights of the last style, where the oracle's choice is not a tie
  soft_ref = ref.G.labels_cap_soft
  top2 = soft_ref.topk(2, -1).values
  clear = (top2[..., 0] - top2[..., 1]) > 1e-4
  assert clear.any()
  assert torch.equal(hip.G.labels_cap_soft.argmax(-1).cpu()[clear], soft_ref.argmax(-1)[clear])


def test_config4_shape_fp16_folded_takes_the_eval_form(monkeypatch):
  """BASELINE configs[4] (B = 1024, M = 8, fp16, folding requested): the decoder runs as the eval form; pose L1 of the first 48
  clips against the float64 oracle within the 2e-2 bar, printed beside the per-block path's on the same inputs."""
  import mix_stage_amd as A
  from oracle import mixstage_oracle as O
  from test_gpu_model16 import _hip_gan
  from mix_stage_amd import ops, ops16
  B, M, S, NCHK = 1024, 8, 8, 48
  audio, pose, labels, style = O.synthetic_batch(B, M=M, S=S)
  style = (style + 3) % S
  hip = _hip_gan(M, S, dtype='fp16').eval()
  A.set_inference_folding(hip, True)
  kw = O.model_kwargs(style.to(DEV)); kw['sample_flag'] = 1
  st = [audio.to(DEV), labels.to(DEV), pose.to(DEV)]
  seen = []
  real = ops16.decoder_chain16

  def spy(x, *a, **k):
    res = real(x, *a, **k)
    seen.append(res is not None)
    return res
  monkeypatch.setattr(ops16, 'decoder_chain16', spy)
  ref = O.build_gan(M=M, S=S, dtype=torch.float64).eval()
  kw_r = O.model_kwargs(style[:NCHK]); kw_r['sample_flag'] = 1
  with torch.no_grad():
    f_ref, _, _ = ref([audio[:NCHK].double(), labels[:NCHK]], pose[:NCHK].double(), **kw_r)
  l1 = {}
  for on in (True, False):
    monkeypatch.setattr(ops, 'USE_DECODER_CHAIN_EVAL', on)
    del seen[:]
    with torch.no_grad():
      y_cap, _, _ = hip([st[0], st[1]], st[2], **kw)
    torch.cuda.synchronize()
    assert seen == [on]
    l1[on] = (y_cap[:NCHK].cpu().double() - f_ref).abs().mean().item()
  print('configs[4] fp16 folded: pose L1 vs float64, eval form %.3e, blocks one by one %.3e' % (l1[True], l1[False]))
  assert l1[True] <= 2e-2


@pytest.mark.parametrize('dt_name', [None, 'bf16'], ids=['fp32', 'bf16'])
def test_optional_logits_output_through_the_c_abi(dt_name):
  """ms_decoder_chain_eval_fwd called directly with the optional z (B, M*P, T): every frame written once, by the tile that owns
  it; out and soft as through the dispatch; with a plan that spreads the groups of a tile over workgroups (B = 2, T = 100)."""
  import mix_stage_amd as A
  from mix_stage_amd import _lib, ops, ops16
  B, M, T, P = 2, 3, 100, 16
  blocks, logits = _build(M, P, 16, seed=51)
  x, score = _inputs(B, M, 272, seed=51, T=T)
  out_d, soft_d = _eval(blocks, logits, x, score, P, True, dt_name)
  L = _lib.lib()
  dt = ops16.NAME_DT[dt_name] if dt_name else 0
  xin = ops16.to_cb8(x, dt) if dt_name else x
  d = ops._chain_desc(B, M, T, 272, P, _lib.MS_BN_EVAL, blocks[0], dt)
  assert L.ms_decoder_chain_eval_supported(ctypes.byref(d)) == 1
  prepared = ops._chain_prepared(d, [m.conv.weight for m in blocks] + [logits.weight])
  words = L.ms_decoder_chain_eval_sync_words(ctypes.byref(d))
  assert words > 0                                                   # (4 work units: one group per workgroup)
  sync = torch.zeros(32 + words, dtype=torch.int32, device=DEV)
  wsp = torch.empty(L.ms_decoder_chain_eval_workspace(ctypes.byref(d)), dtype=torch.uint8, device=DEV)
  z = torch.full((B, M * P, T), float('nan'), device=DEV)
  out = torch.full((B, T, P), float('nan'), device=DEV)
  soft = torch.full((B, T, M), float('nan'), device=DEV)
  tn = _lib.ChainTensors()
  tn.x, tn.score = xin.data_ptr(), score.data_ptr()
  for l, m in enumerate(blocks):
    tn.w[l], tn.bias[l] = m.conv.weight.data_ptr(), m.conv.bias.data_ptr()
    tn.gamma[l], tn.beta[l] = m.norm.weight.data_ptr(), m.norm.bias.data_ptr()
    tn.running_mean[l], tn.running_var[l] = m.norm.running_mean.data_ptr(), m.norm.running_var.data_ptr()
  tn.w_logits, tn.bias_logits = logits.weight.data_ptr(), logits.bias.data_ptr()
  tn.z, tn.soft, tn.out, tn.prepared = z.data_ptr(), soft.data_ptr(), out.data_ptr(), prepared.data_ptr()
  tn.sync, tn.sync_words = sync.data_ptr(), sync.numel()
  for rep in range(2):                                               # (the counters are monotonic: a second launch on them)
    out.fill_(float('nan'))
    _lib.check(L.ms_decoder_chain_eval_fwd(ctypes.byref(d), ctypes.byref(tn), wsp.data_ptr(), wsp.numel(), None), 'ms_decoder_chain_eval_fwd')
    torch.cuda.synchronize()
    assert torch.equal(out, out_d) and torch.equal(soft, soft_d), rep
  assert torch.isfinite(z).all()
  # the mixture recomputed from z and soft in float64 is the kernel's out
  mix = torch.einsum('bgpt,btg->btp', z.double().view(B, M, P, T), soft.double())
  _close(out.double(), mix, 1e-6, 'mixture of the stored logits')
  tdt = torch.bfloat16 if dt_name else None
  ref, _ = _segment_eval_float64(blocks, logits, x, score, M, P, tdt)
  # (bf16, max over all elements: five roundings of 2^-8 -- the input and four block outputs -- each carried through the
  # following layers with a gain of at most ~2: 5 * 3.9e-3 * 2)
  _close(mix.cpu(), ref, 2e-5 if not dt_name else 4e-2, 'stored logits vs float64')
  # train mode is refused
  d.mode = _lib.MS_BN_TRAIN
  assert L.ms_decoder_chain_eval_fwd(ctypes.byref(d), ctypes.byref(tn), wsp.data_ptr(), wsp.numel(), None) != 0
