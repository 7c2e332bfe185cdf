"""CPU: the moving average of the generator's weights -- the C-ABI declaration against _lib.SIGNATURES, the decay checks of FlatAdam
and MixStageTrainStep, save_weights(ema=True) without a trainer, and the float64 recurrence the GPU tests compare the device with,
against a float32 emulation of the kernel's update."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAYS = (0.5, 0.999, 0.9999)
BAD_DECAYS = (float('nan'), 1.0, -0.1, float('inf'), float('-inf'), 1.5)


def ema_reference64(e0, ps, decay, active=None):
  """The recurrence in float64 on the weights `ps` (one array per step): e += (1 - float64(float32(decay))) * (p_k - e), for the
  elements of `active[k]` (a bool array per step; None: all).  numpy arrays in, a float64 array out."""
  om = 1.0 - float(np.float32(decay))
  e = np.asarray(e0, dtype=np.float64).copy()
  for k, p in enumerate(ps):
    new = e + om * (np.asarray(p, dtype=np.float64) - e)
    e = new if active is None else np.where(active[k], new, e)
  return e


def ema_bound(e0, ps, K):
  """Per element: K * 2^-23 * max(|e0|, |p_1|, ..., |p_K|) + K * 2^-149.  Derived: 1.0f - d is exact for d >= 0.5; per step the
  rounding of p - e (|p - e| <= 2 max, times om <= 0.5) and the rounding of the fma (|e'| <= max, a convex combination) cost at
  most 2^-24 max each; the earlier error carries with factor d <= 1; 2^-149 per step covers a subnormal result."""
  mx = np.abs(np.asarray(e0, dtype=np.float64))
  for p in ps:
    mx = np.maximum(mx, np.abs(np.asarray(p, dtype=np.float64)))
  return K * 2.0 ** -23 * mx + K * 2.0 ** -149


def ema_emulate32(e0, ps, decay):
  """The kernel's arithmetic in float32: om = 1.0f - d; t = fl(p - e); e' = fma(om, t, e).  numpy has no fma: the product of two
  float32 is exact in float64, the sum is rounded to float64 and then to float32 (a double rounding, off by at most 2^-53
  relative from the single one)."""
  om = np.float32(1.0) - np.float32(decay)
  e = np.asarray(e0, dtype=np.float32).copy()
  for p in ps:
    t = (np.asarray(p, dtype=np.float32) - e).astype(np.float32)
    e = (om.astype(np.float64) * t.astype(np.float64) + e.astype(np.float64)).astype(np.float32)
  return e


def _decl(name):
  hdr = open(os.path.join(ROOT, 'include', 'mixstage.h')).read()
  hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
  m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, hdr, flags=re.S)
  assert m, '%s is not declared in include/mixstage.h' % name
  return [a.strip() for a in m.group(1).split(',')]


def test_header_declares_the_entry_point_with_the_arguments_signatures_lists():
  import ctypes
  from mix_stage_amd import _lib
  args = _decl('ms_adam_step_segmented_ema')
  restype, argtypes = _lib.SIGNATURES['ms_adam_step_segmented_ema']
  assert restype is ctypes.c_int and len(args) == len(argtypes) == 26
  # pointers where the header has pointers, floats where it has floats
  for a, t in zip(args, argtypes):
    if '*' in a:
      assert t is ctypes.c_void_p, a
    elif a.startswith('float '):
      assert t is ctypes.c_float, a
    elif a.startswith('size_t '):
      assert t is ctypes.c_size_t, a
    else:
      assert t in (ctypes.c_int, ctypes.c_int32), a
  assert args[7] == 'float lr' and args[8] == 'const float* lr_dev' and args[-3] == 'float* ema' and args[-2] == 'float ema_decay'
  # the twins it stands in for are untouched
  assert len(_decl('ms_adam_step_segmented')) == 17 and len(_decl('ms_adam_step_segmented_scaled_lr')) == 23
  assert hasattr(_lib.lib(), 'ms_adam_step_segmented_ema') and _lib.lib().ms_abi_version() == 4


def test_the_sources_keep_the_new_entry_point_out_of_the_elementwise_files():
  csrc = os.path.join(ROOT, 'mix_stage_amd', 'csrc')
  adam = open(os.path.join(csrc, 'adam.hip')).read()
  assert 'int ms_adam_step_segmented_ema(' in adam and '"ew|ew_adam_step_segmented"' in adam
  for fn in ('elementwise.hip', 'elementwise16.hip'):
    assert 'ms_adam_step_segmented_ema' not in open(os.path.join(csrc, fn)).read()
  assert 'adam.hip' in open(os.path.join(csrc, 'Makefile')).read()


@pytest.mark.parametrize('bad', BAD_DECAYS, ids=[repr(b) for b in BAD_DECAYS])
def test_bad_decays_are_rejected_before_anything_touches_the_device(bad):
  from mix_stage_amd import ops
  from mix_stage_amd.train_step import FlatAdam, MixStageTrainStep
  with pytest.raises(ValueError):
    ops.check_ema_decay(bad, 'test')
  w = torch.nn.Parameter(torch.ones(8))              # a CPU parameter: the decay is checked before the device is
  with pytest.raises(ValueError):
    FlatAdam([w], ema_decay=bad)
  with pytest.raises(ValueError):
    MixStageTrainStep(torch.nn.Linear(2, 2), ema_decay=bad)


def test_good_decays_pass_and_a_decay_that_rounds_to_one_in_float32_does_not():
  from mix_stage_amd import ops
  for d in DECAYS + (0.0, 0.25):
    assert ops.check_ema_decay(d, 'test') == d
  with pytest.raises(ValueError):
    ops.check_ema_decay(1.0 - 2.0 ** -30, 'test')    # the kernel argument is float32: this one is 1.0f
  with pytest.raises(ValueError):
    ops.check_ema_decay('fast', 'test')
  w = torch.nn.Parameter(torch.ones(8))
  from mix_stage_amd.train_step import FlatAdam
  with pytest.raises(RuntimeError, match='MI355X'):   # a good decay gets as far as the device check
    FlatAdam([w], ema_decay=0.999)


def test_save_weights_ema_without_a_trainer_raises(tmp_path):
  from mix_stage_amd.checkpoint import save_weights
  model = torch.nn.Linear(2, 2)
  path = tmp_path / 'w.p'
  with pytest.raises(ValueError, match='ema_decay'):
    save_weights(model, path, ema=True)

  class NoAverage:
    ema_decay = None
    model = None

  with pytest.raises(ValueError, match='ema_decay'):
    save_weights(model, path, train_step=NoAverage(), ema=True)
  assert not path.exists()
  save_weights(model, path)                            # the default is today's call
  assert sorted(torch.load(path, weights_only=True)) == ['bias', 'weight']


def _walk(n, steps, seed):
  """Weights that move like a trained parameter: a start of mixed magnitudes (zeros and subnormals among them), steps of ~1e-4."""
  rng = np.random.default_rng(seed)
  p = (rng.standard_normal(n) * 10.0 ** (-3.0 * rng.random(n))).astype(np.float32)
  p[::97] = 0.0
  p[5::1013] = np.float32(2.0 ** -140)
  ps = []
  for _ in range(steps):
    p = (p + (1e-4 * np.sign(rng.standard_normal(n))).astype(np.float32)).astype(np.float32)
    ps.append(p)
  return ps


@pytest.mark.parametrize('decay', DECAYS)
def test_float64_recurrence_against_the_float32_emulation(decay):
  """2^20 elements, 8 steps: the float32 update stays within half of the derived bound of the float64 recurrence."""
  n, K = 1 << 20, 8
  ps = _walk(n, K + 1, seed=3)
  e0, ps = ps[0], ps[1:]
  ref = ema_reference64(e0, ps, decay)
  got = ema_emulate32(e0, ps, decay)
  err, bound = np.abs(got.astype(np.float64) - ref), ema_bound(e0, ps, K)
  worst = float((err / bound).max())
  print('EMA32 decay %g: worst error / bound %.3f' % (decay, worst))
  assert worst <= 0.5
  assert float(np.float32(1.0) - np.float32(decay)) == 1.0 - float(np.float32(decay))      # 1.0f - d is exact for d >= 0.5
  # the recurrence itself: one step by hand, and the closed form for constant weights
  one = ema_reference64(np.array([1.0]), [np.array([3.0])], 0.5)
  assert one[0] == 2.0
  const = ema_reference64(np.array([0.0]), [np.array([1.0])] * 5, decay)
  assert math.isclose(const[0], 1.0 - float(np.float32(decay)) ** 5, rel_tol=1e-12)
  # masked steps leave the element alone
  act = [np.array([True, False])] * 2
  m = ema_reference64(np.array([0.0, 0.0]), [np.array([1.0, 1.0])] * 2, 0.5, act)
  assert m.tolist() == [0.75, 0.0]
