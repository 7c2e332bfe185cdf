"""Dynamic loss scaling for fp16 training: the configuration the trainer accepts and a pure-Python mirror of the rule the device
applies (csrc/adam.hip: adam_prep_seg_kernel<true, *>, adam_scaled_tail; include/mixstage.h: ms_adam_step_segmented_scaled).

The scale S multiplies the backward seed, so every activation gradient of the step is S times the true one -- out of fp16's
subnormal range -- and the optimizer's clip coefficient carries 1/S back.  S is a power of two and moves by factors of 2 only:
every rescaling is exact."""
import math

DYNAMIC = dict(init=2.0 ** 16, growth_interval=2000, min=1.0, max=2.0 ** 24)


def _pow2(x, what):
  x = float(x)
  if not (x > 0.0 and math.isfinite(x) and math.frexp(x)[0] == 0.5):
    raise ValueError('loss scale: %s must be a power of two, got %r' % (what, x))
  if not (2.0 ** -126 <= x <= 2.0 ** 126):
    raise ValueError('loss scale: %s = %r is outside the fp32 range of exact reciprocals' % (what, x))
  return x


class LossScaleRule:
  """init / growth_interval / min / max of one network's scale.
  spec: 'dynamic' (2^16, grows every 2000 finite steps, between 1 and 2^24) | a power-of-two float (static: no growth, floor equal to
  the scale, so every non-finite step is a bad step) | dict(init=, growth_interval=, min=, max=) | a LossScaleRule."""

  def __init__(self, spec):
    if isinstance(spec, LossScaleRule):
      spec = dict(init=spec.init, growth_interval=spec.growth_interval, min=spec.min, max=spec.max)
    if isinstance(spec, str):
      if spec != 'dynamic':
        raise ValueError("loss_scale: 'dynamic', a power-of-two float or a dict, got %r" % (spec,))
      spec = DYNAMIC
    elif isinstance(spec, bool) or spec is None:
      raise ValueError("loss_scale: 'dynamic', a power-of-two float or a dict, got %r" % (spec,))
    elif isinstance(spec, (int, float)):
      s = _pow2(spec, 'the static scale')
      spec = dict(init=s, growth_interval=0, min=s, max=s)
    elif isinstance(spec, dict):
      unknown = set(spec) - set(DYNAMIC)
      if unknown:
        raise ValueError('loss_scale: unknown keys %s (init, growth_interval, min, max)' % sorted(unknown))
      spec = dict(DYNAMIC, **spec)
    else:
      raise ValueError("loss_scale: 'dynamic', a power-of-two float or a dict, got %r" % (spec,))
    self.init = _pow2(spec['init'], 'init')
    self.min = _pow2(spec['min'], 'min')
    self.max = _pow2(spec['max'], 'max')
    self.growth_interval = int(spec['growth_interval'])
    if self.growth_interval < 0 or self.growth_interval != spec['growth_interval']:
      raise ValueError('loss_scale: growth_interval is a non-negative integer (0: never grow)')
    if not (self.min <= self.init <= self.max):
      raise ValueError('loss_scale: min <= init <= max, got %r <= %r <= %r' % (self.min, self.init, self.max))

  def initial_state(self):
    return dict(scale=self.init, good_steps=0, overflow_skips=0, last_was_overflow_skip=0)

  def step(self, state, finite, meeting_error=False):
    """The device's rule on a host copy of the state: -> (new state, applied, bad).  applied: the optimizer moved the weights;
    bad: a non-finite step at the floor scale, or at any scale while an in-launch meeting's error word is raised (meeting_error:
    the scale then stays) -- counted in the optimizer's step word 3, a refused step as without scaling."""
    S, good, skips = float(state['scale']), int(state['good_steps']), int(state['overflow_skips'])
    last, bad = 0, False
    if finite:
      good = min(good + 1, 0x7fffffff)
      if self.growth_interval > 0 and good >= self.growth_interval and S < self.max:
        S, good = S * 2.0, 0
    else:
      good = 0
      if S > self.min and not meeting_error:
        S, skips, last = S * 0.5, skips + 1, 1
      else:
        bad = True
    return dict(scale=S, good_steps=good, overflow_skips=skips, last_was_overflow_skip=last), bool(finite), bad


def state_words(state):
  """The 8 device words of a state, as (S, 1/S) floats and six ints."""
  S = float(state['scale'])
  return (S, 1.0 / S), (int(state['good_steps']), int(state['overflow_skips']), int(state.get('last_was_overflow_skip', 0)), 0, 0, 0)
