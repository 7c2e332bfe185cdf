"""CPU: the loss-scale rule of fp16 training -- the pure-Python mirror (mix_stage_amd/loss_scale.py) of what the device applies
(csrc/adam.hip), against hand-written sequences: growth at the interval, the cap at max, halving, the floor turning a skip into
a bad step, the static form; and the configurations the trainer accepts or rejects.  tests/test_gpu_loss_scale.py holds the device
to the same mirror word for word."""
import os
import re

import pytest

from mix_stage_amd.loss_scale import DYNAMIC, LossScaleRule, state_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(rule, seq):
  """seq of 'F' (finite) / 'N' (not finite) -> [(scale, good_steps, overflow_skips, last, applied, bad)] after every step."""
  st, out = rule.initial_state(), []
  for c in seq:
    st, applied, bad = rule.step(st, c == 'F')
    out.append((st['scale'], st['good_steps'], st['overflow_skips'], st['last_was_overflow_skip'], applied, bad))
  return out


def test_growth_at_the_interval_and_cap_at_max():
  rule = LossScaleRule(dict(init=8, growth_interval=3, min=2, max=32))
  got = _run(rule, 'F' * 9)
  assert [g[:2] for g in got] == [(8, 1), (8, 2), (16, 0), (16, 1), (16, 2), (32, 0), (32, 1), (32, 2), (32, 3)]
  assert all(g[2:] == (0, 0, True, False) for g in got)
  # at the cap the count keeps running and the scale stays
  assert [g[:2] for g in _run(rule, 'F' * 12)[9:]] == [(32, 4), (32, 5), (32, 6)]


def test_halving_and_the_floor_turns_a_skip_into_a_bad_step():
  rule = LossScaleRule(dict(init=8, growth_interval=3, min=2, max=32))
  got = _run(rule, 'FF' + 'NNN' + 'N' + 'F')
  #                 scale good skips last applied bad
  assert got == [(8, 1, 0, 0, True, False), (8, 2, 0, 0, True, False),
                 (4, 0, 1, 1, False, False), (2, 0, 2, 1, False, False),        # overflow skips: halve, count, no bad step
                 (2, 0, 2, 0, False, True), (2, 0, 2, 0, False, True),          # at the floor: a bad step, the skip count stays
                 (2, 1, 2, 0, True, False)]
  # a non-finite step restarts the run of finite steps the growth waits for
  assert [g[:2] for g in _run(rule, 'FFNFFF')] == [(8, 1), (8, 2), (4, 0), (4, 1), (4, 2), (8, 0)]


def test_a_raised_meeting_error_word_makes_a_bad_step_and_leaves_the_scale():
  rule = LossScaleRule(dict(init=8, growth_interval=3, min=2, max=32))
  st = dict(rule.initial_state(), good_steps=2)
  st, applied, bad = rule.step(st, False, meeting_error=True)          # above the floor, yet a bad step: the scale is not the cause
  assert (st['scale'], st['good_steps'], st['overflow_skips'], st['last_was_overflow_skip'], applied, bad) == (8, 0, 0, 0, False, True)
  st, applied, bad = rule.step(st, False)                              # the same without the word: an overflow skip
  assert (st['scale'], st['overflow_skips'], st['last_was_overflow_skip'], applied, bad) == (4, 1, 1, False, False)
  st, applied, bad = rule.step(st, True, meeting_error=True)           # a finite step is applied whatever the word says
  assert (st['scale'], st['good_steps'], applied, bad) == (4, 1, True, False)


def test_the_issue_sequence_of_the_device_test():
  rule = LossScaleRule(dict(init=8, growth_interval=3, min=2, max=32))
  got = _run(rule, 'F' * 9 + 'N' * 5 + 'F')
  assert [g[0] for g in got] == [8, 8, 16, 16, 16, 32, 32, 32, 32, 16, 8, 4, 2, 2, 2]
  assert [g[2] for g in got][9:] == [1, 2, 3, 4, 4, 4] and [g[5] for g in got][9:] == [False, False, False, False, True, False]


def test_static_scale_never_moves_and_every_non_finite_step_is_bad():
  rule = LossScaleRule(1024.0)
  assert (rule.init, rule.min, rule.max, rule.growth_interval) == (1024.0, 1024.0, 1024.0, 0)
  got = _run(rule, 'FFNFN' + 'F' * 5)
  assert all(g[0] == 1024.0 and g[2] == 0 and g[3] == 0 for g in got)
  assert [g[5] for g in got] == [False, False, True, False, True] + [False] * 5
  assert LossScaleRule(1).init == 1.0 and LossScaleRule(2.0 ** -3).init == 0.125


def test_dynamic_defaults_and_explicit_values():
  rule = LossScaleRule('dynamic')
  assert (rule.init, rule.growth_interval, rule.min, rule.max) == (65536.0, 2000, 1.0, 2.0 ** 24) == tuple(DYNAMIC[k] for k in ('init', 'growth_interval', 'min', 'max'))
  got = _run(rule, 'F' * 2000)
  assert got[1998][:2] == (65536.0, 1999) and got[1999][:2] == (131072.0, 0)
  st = rule.initial_state()
  for _ in range(20):                           # 16 halvings reach the floor, then bad steps
    st, _, bad = rule.step(st, False)
  assert st['scale'] == 1.0 and st['overflow_skips'] == 16 and bad
  r2 = LossScaleRule(dict(init=256, growth_interval=0))
  assert (r2.init, r2.growth_interval, r2.min, r2.max) == (256.0, 0, 1.0, 2.0 ** 24)
  assert all(g[0] == 256.0 for g in _run(r2, 'F' * 50))                 # interval 0: never grows
  assert LossScaleRule(r2).init == 256.0
  assert state_words(dict(scale=4.0, good_steps=5, overflow_skips=2)) == ((4.0, 0.25), (5, 2, 0, 0, 0, 0))


@pytest.mark.parametrize('bad', [3.0, 65535, 0.3, 0, -2.0, float('inf'), float('nan'), True, None, 'static', [8],
                                 dict(init=3), dict(min=0.75), dict(max=100), dict(init=4, min=8), dict(init=64, max=32),
                                 dict(growth_interval=-1), dict(growth_interval=2.5), dict(scale=8)])
def test_non_power_of_two_scales_and_malformed_rules_are_rejected(bad):
  with pytest.raises(ValueError):
    LossScaleRule(bad)


def test_header_library_and_binding_agree_on_the_new_entry_point():
  from mix_stage_amd import _lib, ops
  hdr = open(os.path.join(ROOT, 'include', 'mixstage.h')).read()
  m = re.search(r'int ms_adam_step_segmented_scaled\(([^;]*)\);', hdr)
  assert m, 'include/mixstage.h declares ms_adam_step_segmented_scaled'
  assert len(m.group(1).split(',')) == len(_lib.SIGNATURES['ms_adam_step_segmented_scaled'][1]) == 23
  assert hasattr(_lib.lib(), 'ms_adam_step_segmented_scaled') and callable(ops.adam_step_segmented_scaled)
  assert _lib.lib().ms_abi_version() == 4                  # additive


def test_flat_adam_and_trainer_take_the_argument():
  import inspect
  from mix_stage_amd.train_step import FlatAdam, MixStageTrainStep
  assert inspect.signature(FlatAdam.__init__).parameters['loss_scale'].default is None
  assert inspect.signature(MixStageTrainStep.__init__).parameters['loss_scale'].default is None
  for name in ('seed', 'loss_scale_state', 'set_loss_scale_state'):
    assert callable(getattr(FlatAdam, name))
  assert callable(MixStageTrainStep.loss_scale)
