"""CPU: style mixing without a GPU -- StyleTransferSampler.mix_weights against values computed by hand and every refusal of it;
the refusals of the two C entry points (they answer before anything is launched) and of ops.concat_style_soft; what the source of
the kernels promises by construction (no atomics, the id twin's two launch labels and no other); the MS_STYLE_SOFT switch."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sampler(S=3, names=None):
  from mix_stage_amd.sample import StyleTransferSampler
  return StyleTransferSampler(model=None, num_styles=S, speaker_names=names)


def test_mix_weights_dict_vector_and_schedule():
  s = _sampler(3, ['oliver', 'maher', 'chemistry'])
  w = s.mix_weights({0: 0.25, 'chemistry': 0.75}, 4)
  assert w.shape == (1, 4, 3) and w.dtype == torch.float32 and w.is_contiguous()
  assert torch.equal(w, torch.tensor([0.25, 0.0, 0.75]).expand(1, 4, 3))
  assert torch.equal(s.mix_weights({'maher': 2.0}, 1), torch.tensor([[[0.0, 2.0, 0.0]]]))       # used as given: not normalised
  assert torch.equal(s.mix_weights({}, 2), torch.zeros(1, 2, 3))
  for vec in ([0.5, 0.5, 0.0], (0.5, 0.5, 0.0), torch.tensor([0.5, 0.5, 0.0]), torch.tensor([0.5, 0.5, 0.0], dtype=torch.float64)):
    assert torch.equal(s.mix_weights(vec, 5), torch.tensor([0.5, 0.5, 0.0]).expand(1, 5, 3))
  assert torch.equal(s.mix_weights([-1.0, 3.0, 0.0], 2)[0, 1], torch.tensor([-1.0, 3.0, 0.0]))  # any finite float
  sched = torch.arange(12, dtype=torch.float32).reshape(4, 3)
  assert torch.equal(s.mix_weights(sched, 4), sched.reshape(1, 4, 3))
  windows = torch.arange(2 * 64 * 3, dtype=torch.float32).reshape(2, 64, 3)
  assert torch.equal(s.mix_weights(windows, 128), windows.reshape(1, 128, 3))                   # windows concatenated like the inputs
  assert torch.equal(_sampler(2).mix_weights({'1': 1.0}, 1), torch.tensor([[[0.0, 1.0]]]))     # default names are the ids as strings


def test_mix_weights_ramp():
  s = _sampler(3)
  w = s.mix_weights(('ramp', {0: 1.0}, {2: 1.0}), 5)
  hand = torch.tensor([[1.0, 0, 0], [0.75, 0, 0.25], [0.5, 0, 0.5], [0.25, 0, 0.75], [0, 0, 1.0]])
  assert torch.equal(w, hand.reshape(1, 5, 3))                       # a_t = t / 4: dyadic, exact; both endpoints exact
  w = s.mix_weights(('ramp', [0.2, 0.3, 0.5], [0.6, 0.1, 0.3]), 4)
  assert torch.equal(w[0, 0], torch.tensor([0.2, 0.3, 0.5])) and torch.equal(w[0, 3], torch.tensor([0.6, 0.1, 0.3]))
  a, b = torch.tensor([0.2, 0.3, 0.5], dtype=torch.float64), torch.tensor([0.6, 0.1, 0.3], dtype=torch.float64)
  assert torch.equal(w[0, 1], ((1.0 - 1.0 / 3.0) * a + (1.0 / 3.0) * b).float())                # float64, then cast
  assert torch.equal(s.mix_weights(('ramp', {0: 1.0}, {2: 1.0}), 1), torch.tensor([[[1.0, 0.0, 0.0]]]))    # T == 1: a = 0
  # a ramp between two schedules, and a ramp whose end is a ramp
  up = torch.arange(6, dtype=torch.float32).reshape(2, 3)
  assert torch.equal(s.mix_weights(('ramp', up, torch.zeros(2, 3)), 2), torch.tensor([[[0.0, 1.0, 2.0], [0.0, 0.0, 0.0]]]))
  nested = s.mix_weights(('ramp', {0: 1.0}, ('ramp', {0: 1.0}, {1: 1.0})), 3)
  assert torch.equal(nested, torch.tensor([[[1.0, 0, 0], [0.75, 0.25, 0], [0, 1.0, 0]]]))


@pytest.mark.parametrize('spec,T', [
    ({'nobody': 1.0}, 4),                      # unknown name
    ({3: 1.0}, 4), ({-1: 1.0}, 4), ({0.5: 1.0}, 4), ({True: 1.0}, 4),      # ids outside 0..S-1 / not integers
    ([0.5, 0.5], 4), ([0.25] * 4, 4),         # wrong length
    (torch.zeros(5, 3), 4), (torch.zeros(4, 2), 4), (torch.zeros(2, 64, 3), 64), (torch.zeros(1, 1, 4, 3), 4),
    ([0.5, float('nan'), 0.5], 4), ({0: float('inf')}, 4), (torch.full((4, 3), float('-inf')), 4),
    (('ramp', {0: 1.0}), 4), (('ramp', {0: 1.0}, {1: 1.0}, {2: 1.0}), 4), (('step', {0: 1.0}, {1: 1.0}), 4),
    (('ramp', {0: 1.0}, [1.0, 0.0]), 4),      # a refusal inside a ramp
    ('oliver', 4), (None, 4),
    ({0: 1.0}, 0), ({0: 1.0}, 2.5),
])
def test_mix_weights_refusals(spec, T):
  with pytest.raises(ValueError):
    _sampler(3, ['oliver', 'maher', 'chemistry']).mix_weights(spec, T)


def test_c_entry_points_refuse_before_they_launch():
  from mix_stage_amd import _lib
  L = _lib.lib()
  fwd = lambda B, C, D, T, S, sb, st: L.ms_concat_style_soft_fwd(None, None, None, sb, st, None, B, C, D, T, S, None)
  bwd = lambda B, C, D, T, S, sb, st: L.ms_concat_style_soft_bwd(None, None, None, sb, st, None, None, None, B, C, D, T, S, None)
  for call in (fwd, bwd):
    for args, word in (((2, 5, 3, 7, 0, 0, 0), 'S=0'), ((2, 5, 0, 7, 4, 4, 0), 'D=0'), ((2, 5, 3, 7, 4, -4, 0), 'negative'),
                       ((2, 5, 3, 7, 4, 28, -4), 'negative'), ((2, 5, 3, 7, 70000, 0, 0), 'S=70000'), ((0, 5, 3, 7, 4, 4, 0), 'B=0')):
      assert call(*args) != 0, args
      assert word in L.ms_last_error().decode(), (args, L.ms_last_error().decode())
  assert fwd(2, 5, 3, 7, 4, 28, 4) != 0 and 'required' in L.ms_last_error().decode()           # good sizes, no tensors
  assert L.ms_abi_version() == 4


def test_op_refuses_cpu_and_wrong_tensors_without_a_gpu():
  from mix_stage_amd import _lib, ops
  x, E = torch.randn(2, 5, 7), torch.randn(4, 3)
  with pytest.raises(TypeError, match='on the device'):
    ops.concat_style_soft(x, E, torch.rand(2, 7, 4))
  with pytest.raises(TypeError):
    ops.concat_style_soft(x, E, [0.5, 0.5])
  import mix_stage_amd as A
  G = A.JointLateClusterSoftStyle4_G(time_steps=64, out_feats=6, num_clusters=2, style_dict={0: 0, 1: 1}, style_dim=10, shape={})
  assert G.style_emb.num_embeddings == 2 and list(G.style_emb.state_dict()) == ['emb.weight']
  assert issubclass(_lib.MixStageLibError, RuntimeError)


def test_kernel_source_has_no_atomics_and_only_the_twin_labels():
  src = open(os.path.join(ROOT, 'mix_stage_amd', 'csrc', 'style_mix.hip')).read()
  code = re.sub(r'//[^\n]*', '', src)
  assert 'atomic' not in code.lower()
  assert sorted(re.findall(r'TimingScope\s+\w+\s*\([^;"]*"([^"]+)"\);', code)) == ['ew|ew_concat_style_bwd', 'ew|ew_concat_style_fwd']
  assert len(re.findall(r'\(total \+ 255\) / 256, 2048\)', code)) == 3          # forward, dx, per-frame dw: the id kernels' grid cap
  for twin in ('elementwise.hip', 'elementwise16.hip'):
    assert 'ms_concat_style_soft' not in open(os.path.join(ROOT, 'mix_stage_amd', 'csrc', twin)).read()
  assert 'style_mix.hip' in open(os.path.join(ROOT, 'mix_stage_amd', 'csrc', 'Makefile')).read()


def test_style_soft_switch_is_read_from_the_environment():
  code = 'from mix_stage_amd import ops; print(int(ops.style_soft_active()))'
  outs = []
  for val in (None, '0'):
    env = dict(os.environ)
    env.pop('MS_STYLE_SOFT', None)
    if val is not None:
      env['MS_STYLE_SOFT'] = val
    outs.append(subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout.strip())
  assert outs == ['1', '0']
  from mix_stage_amd import ops
  old = ops.enable_style_soft(False)
  try:
    assert not ops.style_soft_active()
  finally:
    ops.enable_style_soft(old)
  assert ops.style_soft_active() == old
