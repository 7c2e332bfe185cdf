"""CPU: the host side of the learning-rate schedule -- the mirror of torch's ExponentialLR bit for bit in Python double, the
state() / set_state() round trip, the schedule protocol, and the two new C-ABI symbols behind the unchanged ABI version."""
import copy

import pytest
import torch


def _torch_exponential(lr0, gamma, epochs):
  """[lr after epoch 1, ..., lr after epoch `epochs`] of torch.optim.lr_scheduler.ExponentialLR on a dummy optimizer."""
  import warnings
  p = torch.nn.Parameter(torch.zeros(1))
  opt = torch.optim.Adam([p], lr=lr0)
  sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=gamma)
  out = []
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')                   # (scheduler.step() before optimizer.step(): no optimizer step is wanted here)
    for _ in range(epochs):
      sched.step()
      out.append(opt.param_groups[0]['lr'])
  return out


@pytest.mark.parametrize('lr0,gamma,epochs', [(1e-4, 0.99, 300), (3e-4, 0.5, 40)])
def test_exponential_mirror_equals_torch_bit_for_bit(lr0, gamma, epochs):
  from mix_stage_amd.lr_schedule import ExponentialLR
  ref = _torch_exponential(lr0, gamma, epochs)
  sched, lr, got = ExponentialLR(gamma), lr0, []
  for _ in range(epochs):
    lr = sched.step(lr)
    got.append(lr)
  assert all(isinstance(x, float) for x in got)
  assert got == ref, [(i, a, b) for i, (a, b) in enumerate(zip(got, ref)) if a != b][:3]
  assert sched.epoch == epochs
  if gamma == 0.99:
    # the figures of the reference's run: 0.366 of the initial step size after 100 epochs, 0.049 after 300
    assert abs(got[99] / lr0 - 0.366) < 5e-4 and abs(got[299] / lr0 - 0.049) < 5e-4
    # the chained form is NOT the closed form in the last bits -- which is why the mirror chains
    assert any(a != lr0 * gamma ** (i + 1) for i, a in enumerate(got))


def test_state_round_trip_and_constant():
  from mix_stage_amd.lr_schedule import ConstantLR, ExponentialLR
  a = ExponentialLR(0.9)
  lr = 1e-3
  for _ in range(7):
    lr = a.step(lr)
  b = ExponentialLR(0.9)
  b.set_state(copy.deepcopy(a.state()))
  assert b.state() == a.state() == (7,) and b.epoch == 7
  assert [b.step(lr), b.step(lr)] == [a.step(lr), a.step(lr)] and a.state() == b.state() == (9,)
  c = ConstantLR()
  assert c.step(1e-4) == 1e-4 and c.step(1e-4) == 1e-4 and c.state() == (2,)
  d = ConstantLR()
  d.set_state(c.state())
  assert d.state() == (2,)
  for bad in (0.0, -0.5, float('nan'), float('inf')):
    with pytest.raises(ValueError):
      ExponentialLR(bad)


def test_protocol_accepts_gamma_objects_and_lr_of_epoch():
  from mix_stage_amd import lr_schedule as LS
  import mix_stage_amd as A
  assert A.ExponentialLR is LS.ExponentialLR and A.ConstantLR is LS.ConstantLR and A.as_lr_schedule is LS.as_lr_schedule
  assert LS.as_lr_schedule(None) is None
  s = LS.as_lr_schedule(0.5)
  assert isinstance(s, LS.ExponentialLR) and s.gamma == 0.5 and s.step(1.0) == 0.5
  own = LS.ExponentialLR(0.25)
  assert LS.as_lr_schedule(own) is own

  class Halving:                                      # a caller's schedule: step(lr) -> lr, no state
    def step(self, lr):
      return lr / 2

  h = Halving()
  assert LS.as_lr_schedule(h) is h

  class Table:                                        # a caller's schedule: lr(epoch) -> lr
    def lr(self, epoch):
      return [1e-3, 5e-4, 1e-4][min(epoch, 2)]

  t = LS.as_lr_schedule(Table())
  assert [t.step(123.0), t.step(123.0), t.step(123.0)] == [5e-4, 1e-4, 1e-4]
  u = LS.as_lr_schedule(Table())
  u.set_state(t.state())
  assert u.state() == t.state() == (3, ())
  for bad in (True, 'exp', object()):
    with pytest.raises(TypeError):
      LS.as_lr_schedule(bad)
  for bad in (0.0, -1e-4, float('nan'), float('inf'), 1e-60, 1e60):         # (1e-60 is 0, 1e60 is inf in float32: the device would refuse them)
    with pytest.raises(ValueError):
      LS.check_lr(bad)
  assert LS.check_lr(1e-4) == 1e-4


def test_new_symbols_load_and_the_abi_version_stays():
  import ctypes
  from mix_stage_amd import _lib
  L = _lib.lib()
  assert L.ms_abi_version() == 4
  for name, twin in (('ms_adam_step_segmented_lr', 'ms_adam_step_segmented'),
                     ('ms_adam_step_segmented_scaled_lr', 'ms_adam_step_segmented_scaled')):
    fn = getattr(L, name)
    assert fn.restype is ctypes.c_int
    res, args = _lib.SIGNATURES[name]
    tres, targs = _lib.SIGNATURES[twin]
    # argument for argument the twin, except `float lr` (argument 7) -> a pointer
    assert res is tres and len(args) == len(targs)
    assert [i for i, (a, b) in enumerate(zip(args, targs)) if a is not b] == [7]
    assert targs[7] is ctypes.c_float and args[7] is ctypes.c_void_p
