"""Learning-rate schedules of the trainer, host side only (no torch, no device).

The reference trains with Adam(lr=1e-4) per network and torch.optim.lr_scheduler.ExponentialLR(gamma=0.99), stepped once per
epoch for both optimizers (TR:262-287,311-313,499-500).  A schedule here maps the CURRENT learning rate of one optimizer to the
next one -- torch's chained form, `lr = lr * gamma` in Python double, not the closed form lr0 * gamma**k (the two differ in the
last bits after a few epochs).  What the device receives is float32(lr): MixStageTrainStep(lr_schedule=...) writes it into the
word the optimizer's prep kernel reads (include/mixstage.h: ms_adam_step_segmented_lr), so a captured step follows the schedule.

Protocol of a schedule object, either of
  step(lr) -> lr    the next learning rate from the current one (chained; what ExponentialLR and ConstantLR implement)
  lr(epoch) -> lr   the learning rate of epoch `epoch` as an absolute value (asked for epoch 1, 2, ...; epoch 0 runs at the lr the
                    trainer was constructed with)
and optionally state() / set_state(state) like the lambda schedulers of gan.py (a schedule without them is taken as stateless).
as_lr_schedule() turns None / a float gamma / an object into such a schedule."""


class ExponentialLR:
  """Mirror of torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma): every step() multiplies the current lr by gamma."""

  def __init__(self, gamma=0.99):
    gamma = float(gamma)
    if not (gamma > 0.0) or gamma != gamma or gamma == float('inf'):
      raise ValueError('ExponentialLR: gamma is a positive finite number, got %r' % (gamma,))
    self.gamma = gamma
    self.epoch = 0

  def step(self, lr):
    self.epoch += 1
    return float(lr) * self.gamma

  def state(self):
    return (self.epoch,)

  def set_state(self, state):
    self.epoch, = state
    self.epoch = int(self.epoch)

  def __repr__(self):
    return 'ExponentialLR(gamma=%r)' % (self.gamma,)


class ConstantLR:
  """The learning rate stays where it is (epochs are still counted)."""

  def __init__(self):
    self.epoch = 0

  def step(self, lr):
    self.epoch += 1
    return float(lr)

  def state(self):
    return (self.epoch,)

  def set_state(self, state):
    self.epoch, = state
    self.epoch = int(self.epoch)

  def __repr__(self):
    return 'ConstantLR()'


class _ByEpoch:
  """Adapter: a caller's object with lr(epoch) -> float behind the chained protocol."""

  def __init__(self, obj):
    self.obj = obj
    self.epoch = 0

  def step(self, lr):
    self.epoch += 1
    return float(self.obj.lr(self.epoch))

  def state(self):
    inner = self.obj.state() if hasattr(self.obj, 'state') else ()
    return (self.epoch, inner)

  def set_state(self, state):
    self.epoch, inner = state
    self.epoch = int(self.epoch)
    if hasattr(self.obj, 'set_state'):
      self.obj.set_state(inner)

  def __repr__(self):
    return 'by_epoch(%r)' % (self.obj,)


def as_lr_schedule(spec):
  """None -> None; a number -> ExponentialLR(gamma=number); an object with step(lr) -> itself; one with lr(epoch) -> adapted."""
  if spec is None:
    return None
  if isinstance(spec, bool):
    raise TypeError('lr_schedule: None, a float gamma or a schedule object, got %r' % (spec,))
  if isinstance(spec, (int, float)):
    return ExponentialLR(float(spec))
  if callable(getattr(spec, 'step', None)):
    return spec
  if callable(getattr(spec, 'lr', None)):
    return _ByEpoch(spec)
  raise TypeError('lr_schedule: None, a float gamma or an object with step(lr) -> lr or lr(epoch) -> lr, got %r' % (spec,))


def check_lr(lr, who='lr'):
  """A learning rate a step can be taken with: a positive finite number whose float32 value is positive and finite too (the device
  refuses anything else as a bad step)."""
  import struct
  lr = float(lr)
  try:
    f32 = struct.unpack('f', struct.pack('f', lr))[0]
  except OverflowError:
    f32 = float('inf')
  if not (lr > 0.0 and f32 > 0.0 and f32 != float('inf')):
    raise ValueError('%s: a positive finite float32 value, got %r' % (who, lr))
  return lr
