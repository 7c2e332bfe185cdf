"""GPU: two independent clip-resident DATA GRADIENTS in ONE launch (ms_clip_hold around ms_conv_block_bwd_ex; csrc/clip32.hip:
clip32_pair_kernel) -- the PoseStyleEncoder's data gradients inside the UNet's half-empty data-gradient launches.  A merged launch
runs the same bodies on the same arguments, so every comparison here is bit for bit against the two launches one by one."""
import ctypes

import pytest
import torch

from oracle import mixstage_oracle as O
from test_gpu_clip_corun import (PAIR_MARK, _equal_dicts, _g_forward, _gan, _labels, _ptr, _stream,
                                 trainer_globals_restored)  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _L():
  from mix_stage_amd import _lib
  return _lib


class BwdBlock:
  """The backward call of one 1-D conv block (MS_BARE: dy is the gradient of the conv output) through the C-ABI, with buffers of
  its own: data gradient on the clip-resident kernel, weight gradient queued (ms_wgrad_flush).  fused: the launch carries the
  BatchNorm + LeakyReLU backward of the block that produced x (EP_DGRAD_BN, with its meeting); accum: ms_bwd_options.dx_accum."""

  def __init__(self, B, cin, cout, T, k, s, up2=False, fused=False, accum=False, seed=0):
    L = _L()
    lib = L.lib()
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    To = (T + 2 - k) // s + 1
    self.up2, self.fused = up2, fused
    self.d = L.ConvDesc(B, cin, 1, T, cout, 1, 1, k, 1, s, 0, 1, 1, To, L.MS_BARE, L.MS_IN_UP2ADD if up2 else L.MS_IN_PLAIN, 0.2, 1e-5, 0.1, 0)
    self.x = rnd(B, cin, T // 2 if up2 else T)
    self.x2 = rnd(B, cin, T) if up2 else None
    self.w = rnd(cout, cin, k) * (1.0 / (cin * k) ** 0.5)
    self.dy = rnd(B, cout, To)
    self.dx = torch.zeros_like(self.x)
    self.dx2 = torch.zeros_like(self.x2) if up2 else None
    self.dw = torch.zeros_like(self.w)
    self.acc = rnd(B, cin, T) if accum else None
    sp = ctypes.c_int(1)
    n = lib.ms_wgrad_partials_elems(ctypes.byref(self.d), ctypes.byref(sp))
    self.part = torch.zeros(n, device=DEV) if n else None
    self.ws = torch.zeros(max(256, lib.ms_conv_block_bwd_workspace(ctypes.byref(self.d))), dtype=torch.uint8, device=DEV)
    self.sync = None
    if fused:
      # the producer of x: y_raw, its batch statistics (save = mean, invstd, scale, shift), y = lrelu(scale * y_raw + shift)
      assert lib.ms_dgrad_fuses_prev_bn(ctypes.byref(self.d)) == 1
      self.p_raw = self.x.clone()
      mean, var = self.p_raw.mean((0, 2)), self.p_raw.var((0, 2), unbiased=False)
      self.p_gamma = 1 + 0.1 * rnd(cin)
      invstd = (var + 1e-5).rsqrt()
      sc = self.p_gamma * invstd
      sh = 0.1 * rnd(cin) - mean * sc
      self.p_save = torch.cat([mean, invstd, sc, sh]).contiguous()
      self.p_y = torch.nn.functional.leaky_relu(self.p_raw * sc[None, :, None] + sh[None, :, None], 0.2).contiguous()
      self.p_dgamma, self.p_dbeta, self.p_dbias = (torch.zeros(cin, device=DEV) for _ in range(3))
      self.sync = torch.zeros(1024, dtype=torch.int32, device=DEV)

  def grid(self):
    return _L().lib().ms_clip_dgrad_grid(ctypes.byref(self.d))

  def run(self):
    L = _L()
    opt = L.BwdOptions()
    opt.wgrad_partials = self.part.data_ptr() if self.part is not None else None
    opt.defer_wgrad_launch = 1
    if self.acc is not None:
      opt.dx_accum = self.acc.data_ptr()
    if self.fused:
      opt.prev_y, opt.prev_y_raw, opt.prev_save, opt.prev_gamma = (t.data_ptr() for t in (self.p_y, self.p_raw, self.p_save, self.p_gamma))
      opt.prev_dgamma, opt.prev_dbeta, opt.prev_dbias = self.p_dgamma.data_ptr(), self.p_dbeta.data_ptr(), self.p_dbias.data_ptr()
      opt.prev_slope, opt.bn_sync, opt.bn_sync_words = 0.2, self.sync.data_ptr(), self.sync.numel()
    L.check(L.lib().ms_conv_block_bwd_ex(ctypes.byref(self.d), _ptr(self.x), _ptr(self.x2), _ptr(self.w), None, None, None, None, None, None,
                                         _ptr(self.dy), None, _ptr(self.dx), _ptr(self.dx2), _ptr(self.dw), None, None, None,
                                         _ptr(self.ws), self.ws.numel(), _stream(), ctypes.byref(opt)), 'ms_conv_block_bwd_ex')

  def state(self):
    """(after ms_wgrad_flush) the data gradient, the EP_DGRAD_BN outputs, what the weight-gradient queue wrote, the sync words"""
    out = {'dx': self.dx, 'dw': self.dw}
    if self.up2:
      out['dx2'] = self.dx2
    if self.part is not None:
      out['wgrad partials'] = self.part
    if self.fused:
      out.update({'prev dgamma': self.p_dgamma, 'prev dbeta': self.p_dbeta, 'prev dbias': self.p_dbias, 'sync words': self.sync})
    return {k: v.clone() for k, v in out.items()}


def _flush_wgrad():
  L = _L()
  L.check(L.lib().ms_wgrad_flush(_stream()), 'ms_wgrad_flush')


def _held_then(guest, host):
  """guest held, host launched, flush: what a guest block's backward and the next block's do between them."""
  L = _L()
  try:
    L.check(L.lib().ms_clip_hold(_stream()), 'ms_clip_hold')
    guest.run()
    host.run()
    L.check(L.lib().ms_clip_hold_flush(_stream()), 'ms_clip_hold_flush')
    _flush_wgrad()
  except BaseException:
    L.lib().ms_clip_hold_discard(_stream())
    L.lib().ms_wgrad_discard()
    raise


def _alone(guest, host):
  guest.run()
  host.run()
  _flush_wgrad()


def _same(a, b, what):
  assert sorted(a) == sorted(b), what
  for k in a:
    assert torch.equal(a[k], b[k]), '%s: %s differs' % (what, k)
  assert not torch.isnan(a['dx']).any(), '%s: NaN data gradient (an in-launch meeting gave up)' % what


# the path's instances.  Hosts: a UNet1D up block's and down block's data gradient (256 -> 256); guests: the PoseStyleEncoder's k4 s2
# blocks by the channel groups per wave of their data gradient's reduction (= output channels): 8 -> the run-time form, 64 -> 2,
# 128 -> 4, 256 -> 8
HOSTS = {'up8': dict(cin=256, cout=256, k=3, s=1, up2=True), 'down8': dict(cin=256, cout=256, k=4, s=2),
         'down8_acc': dict(cin=256, cout=256, k=4, s=2, accum=True)}
GUESTS = {'dg0_256to8': dict(cin=256, cout=8, k=4, s=2, fused=True), 'dg8_256to256': dict(cin=256, cout=256, k=4, s=2, fused=True),
          'dg8_128to256': dict(cin=128, cout=256, k=4, s=2, fused=True), 'dg4_64to128': dict(cin=64, cout=128, k=4, s=2, fused=True),
          'dg2_64to64': dict(cin=64, cout=64, k=4, s=2, fused=True)}
PAIRS = [('up8', 'dg0_256to8'), ('up8', 'dg8_256to256')] + [(h, g) for h in ('down8', 'down8_acc') for g in ('dg8_128to256', 'dg4_64to128', 'dg2_64to64')]


@pytest.mark.parametrize('T', [16, 8])
@pytest.mark.parametrize('host,guest', PAIRS)
def test_pair_equals_the_two_launches_bitwise(host, guest, T):
  """B = 8.  The host (T = 16) has two pixel workgroups per channel tile, sixteen workgroups in all; the guest at T = 16 has two as
  well and meets inside the launch (its producer's BatchNorm backward), at T = 8 one and does not.  Two rounds: the meeting
  counters are monotonic, a merged launch must advance the guest's as a launch of its own does; the queued weight gradients add."""
  make = lambda: (BwdBlock(8, T=16, seed=1, **HOSTS[host]), BwdBlock(8, T=T, seed=2, **GUESTS[guest]))
  (h1, g1), (h2, g2) = make(), make()
  assert h1.grid() == 16 and g1.grid() == (T // 8) * ((GUESTS[guest]['cin'] + 31) // 32)
  assert _L().lib().ms_clip_dgrad_pair_ok(ctypes.byref(h1.d), ctypes.byref(g1.d)) == 1
  states_alone, states_pair = [], []

  def alone():
    for _ in range(2):
      _alone(g1, h1)
      states_alone.append((h1.state(), g1.state()))

  def paired():
    for _ in range(2):
      _held_then(g2, h2)
      states_pair.append((h2.state(), g2.state()))
  la, lp = _labels(alone), _labels(paired)
  assert sum(la.values()) == 4 and not any(PAIR_MARK in k for k in la), la
  assert sum(lp.values()) == 2 and all(PAIR_MARK in k and 'dgrad' in k for k in lp), lp
  for r, ((ha, ga), (hp, gp)) in enumerate(zip(states_alone, states_pair)):
    _same(ha, hp, 'round %d host' % r)
    _same(ga, gp, 'round %d guest' % r)
  assert int(g2.sync[0]) == 0                                      # (no meeting gave up)
  assert (int(g2.sync[32:].sum()) > 0) == (T == 16)                # (... and at T = 16 the guest did meet)


def _no_merge_case(name):
  if name == 'no_room':               # a full-resolution UNet data gradient of 32 clips is 256 workgroups: no room on 256 compute units
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 32
    while 8 * (B * 64 // 64) + 2 * (B * 16 // 64) <= cus:
      B *= 2
    return BwdBlock(B, T=64, seed=1, **HOSTS['down8']), BwdBlock(B, T=16, seed=2, **GUESTS['dg2_64to64'])
  if name == 'host_grid_not_8':       # 96 input channels: 3 channel tiles x 2 pixel workgroups
    return BwdBlock(8, 96, 256, 16, 4, 2, seed=1), BwdBlock(8, T=16, seed=2, **GUESTS['dg2_64to64'])
  if name == 'no_instance':           # the up path never meets the encoder's first blocks: no instance for that pair
    return BwdBlock(8, T=16, seed=1, **HOSTS['up8']), BwdBlock(8, T=16, seed=2, **GUESTS['dg4_64to128'])
  if name == 'guest_not_dg2':         # a k3 s1 guest (the transposed form) has no instance as a guest
    return BwdBlock(8, T=16, seed=1, **HOSTS['down8']), BwdBlock(8, 64, 64, 16, 3, 1, fused=True, seed=2)
  if name == 'guest_not_clip':        # a k5 block's data gradient runs the other kernels: launched at once, the hold is disarmed
    return BwdBlock(8, T=16, seed=1, **HOSTS['down8']), BwdBlock(8, 64, 64, 16, 5, 1, seed=2)
  assert name in ('knob_bwd_off', 'knob_off')
  return BwdBlock(8, T=16, seed=1, **HOSTS['down8']), BwdBlock(8, T=16, seed=2, **GUESTS['dg2_64to64'])


@pytest.mark.parametrize('name', ['no_room', 'host_grid_not_8', 'no_instance', 'guest_not_dg2', 'guest_not_clip', 'knob_bwd_off', 'knob_off'])
def test_no_merge_same_bits_and_two_plain_launches(name):
  lib = _L().lib()
  (h1, g1), (h2, g2) = _no_merge_case(name), _no_merge_case(name)
  knob = {'knob_bwd_off': lib.ms_debug_set_clip_corun_bwd, 'knob_off': lib.ms_debug_set_clip_corun}.get(name)
  old = knob(0) if knob else None
  try:
    la = _labels(lambda: _alone(g1, h1))
    lp = _labels(lambda: _held_then(g2, h2))
  finally:
    if knob:
      knob(old)
  assert not any(PAIR_MARK in k for k in lp), lp
  assert lp == la, (lp, la)
  if name == 'guest_not_clip':
    assert g1.grid() == 0 and sum(lp.values()) == 1, lp           # (only the host is on the clip path)
  else:
    assert g1.grid() > 0 and h1.grid() > 0 and sum(lp.values()) == 2, lp
    if not knob:
      assert lib.ms_clip_dgrad_pair_ok(ctypes.byref(h1.d), ctypes.byref(g1.d)) == 0
  _same(h1.state(), h2.state(), name + ' host')
  _same(g1.state(), g2.state(), name + ' guest')


def test_a_forward_block_and_a_data_gradient_never_share_a_launch():
  """A held data gradient in front of a forward block that could host a forward guest: launched first, on its own."""
  from test_gpu_clip_corun import HOSTS as FWD_HOSTS, Block
  g1, g2 = (BwdBlock(8, T=16, seed=2, **GUESTS['dg2_64to64']) for _ in range(2))
  f1, f2 = (Block(4, T=32, mode=2, seed=1, **FWD_HOSTS['down8']) for _ in range(2))
  L = _L()

  def held():
    L.check(L.lib().ms_clip_hold(_stream()), 'ms_clip_hold')
    g2.run()
    f2.run()
    L.check(L.lib().ms_clip_hold_flush(_stream()), 'ms_clip_hold_flush')
    _flush_wgrad()
  la = _labels(lambda: (g1.run(), f1.run(), _flush_wgrad()))
  lp = _labels(held)
  assert lp == la and sum(lp.values()) == 2 and not any(PAIR_MARK in k for k in lp), (lp, la)
  _same(g1.state(), g2.state(), 'guest')
  for u, v in zip(f1.state(), f2.state()):
    assert torch.equal(u, v)


def test_flush_discard_and_second_hold():
  L = _L()
  lib = L.lib()
  # hold, explicit flush, then a launch of the library that is no conv block and reads the held block's output
  from mix_stage_amd import ops
  g1, g2 = (BwdBlock(8, T=16, seed=2, **GUESTS['dg2_64to64']) for _ in range(2))
  g1.run()
  want = ops.to_time_major(g1.dx)
  L.check(lib.ms_clip_hold(_stream()), 'ms_clip_hold')
  g2.run()
  L.check(lib.ms_clip_hold_flush(_stream()), 'ms_clip_hold_flush')
  got = ops.to_time_major(g2.dx)
  _flush_wgrad()
  _same(g1.state(), g2.state(), 'flush')
  assert torch.equal(want, got)
  # hold, then discard: the data gradient is not launched (the call's weight gradient is queued as always)
  g3 = BwdBlock(8, T=16, seed=2, **GUESTS['dg2_64to64'])
  before = g3.state()

  def held_and_dropped():
    L.check(lib.ms_clip_hold(_stream()), 'ms_clip_hold')
    g3.run()
    lib.ms_clip_hold_discard(_stream())
    L.check(lib.ms_clip_hold_flush(_stream()), 'ms_clip_hold_flush')       # (nothing left to launch)
    lib.ms_wgrad_discard()
  assert _labels(held_and_dropped) == {}
  torch.cuda.synchronize()
  _same(before, g3.state(), 'discard')
  # a second hold while a data gradient is pending is an error, and leaves the pending one alone
  L.check(lib.ms_clip_hold(_stream()), 'ms_clip_hold')
  g3.run()
  assert lib.ms_clip_hold(_stream()) != 0
  assert b'pending' in lib.ms_last_error()
  L.check(lib.ms_clip_hold_flush(_stream()), 'ms_clip_hold_flush')
  _flush_wgrad()
  torch.cuda.synchronize()
  _same(g1.state(), g3.state(), 'flush after the refused hold')


# ---------------------------------------------------------------------------------------------------------------------------
# model level
def _bwd_merged(labels):
  return sum(c for k, c in labels.items() if PAIR_MARK in k and 'dgrad' in k)


def _same_bits(a, b, what):
  """Bit patterns, not values: a NaN or infinity (fp16 without loss scaling) has to be the same NaN on both sides."""
  assert sorted(a) == sorted(b), what
  for k in a:
    u, v = a[k].reshape(-1).contiguous().view(torch.uint8), b[k].reshape(-1).contiguous().view(torch.uint8)
    assert a[k].shape == b[k].shape and torch.equal(u, v), '%s: %s differs' % (what, k)


def _g_backward_runs(batch, M, S, hook=None, prepare=None, pose_grad=False):
  """The generator forward and backward with the backward co-run on and off -> ({on: results}, {on: merged data gradients},
  {on: data gradients held back}).  hook(model) -> a handle to remove; prepare(model) -> a callable that undoes it; pose_grad: the
  pose input y requires a gradient, reported as 'grad/y'."""
  from mix_stage_amd import ops
  res, merged, offered = {}, {}, {}

  def run(model, on):
    if not pose_grad:
      res[on] = _g_forward(model, batch, True, backward=True)
      return
    audio, pose, labels, style = batch
    y = pose.to(DEV).requires_grad_()
    res[on] = _g_forward(model, (audio, y, labels, style), True, backward=True)
    assert y.grad is not None
    res[on]['grad/y'] = y.grad.detach().clone()
  for on in (True, False):
    model = _gan(M, S)
    h = hook(model) if hook else None
    undo = prepare(model) if prepare else None
    old = ops.enable_corun_bwd(on)
    try:
      before = ops._corun['bwd_offered']
      labels = _labels(lambda: run(model, on))
      assert not ops._corun['bwd_keep'] and not ops._corun['keep']     # (what a held launch touches is let go once it is on the stream)
      offered[on] = ops._corun['bwd_offered'] - before
      merged[on] = _bwd_merged(labels)
    finally:
      ops.enable_corun_bwd(old)
      if undo is not None:
        undo()
      if h is not None:
        h.remove()
  return res, merged, offered


def test_generator_backward_with_and_without_the_corun():
  """B = 4, T = 64, M = S = 2: losses, pose, BatchNorm buffers and every parameter gradient are the same bits with the style
  encoder's data gradients riding in the UNet's data-gradient launches and without."""
  batch = O.synthetic_batch(4, M=2, S=2, seed=11)
  res, merged, offered = _g_backward_runs(batch, 2, 2)
  assert offered[True] > 0 and merged[True] > 0 and offered[False] == 0 and merged[False] == 0, (offered, merged)
  _equal_dicts(res[True], res[False], 'backward co-run')


def test_pose_gradient_with_and_without_the_corun():
  """y requires a gradient (input saliency, a gradient check of G): the encoder's first block has a data gradient too, and its
  reader is the transpose in front of the chain, not a conv block -- that block must not hold its launch back.  dL/dy and
  everything else are the same bits with the switch on and off, and the other data gradients still merge."""
  batch = O.synthetic_batch(4, M=2, S=2, seed=14)
  res, merged, offered = _g_backward_runs(batch, 2, 2, pose_grad=True)
  assert offered[True] > 0 and merged[True] > 0 and offered[False] == 0 and merged[False] == 0, (offered, merged)
  assert float(res[False]['grad/y'].abs().sum()) > 0
  _equal_dicts(res[True], res[False], 'pose gradient')


def _mode(name):
  """prepare(model) of an arithmetic mode other than fp32 -> undo()"""
  def prepare(model):
    import mix_stage_amd as A
    if name == 'bf16x6':
      lib = _L().lib()
      old = lib.ms_set_precision(1)
      return lambda: lib.ms_set_precision(old)
    A.set_compute_dtype(model, name)
    return None
  return prepare


@pytest.mark.parametrize('mode', ['bf16', 'fp16', 'bf16x6'])
def test_other_arithmetic_modes_make_the_backward_corun_stand_aside(mode):
  """The 16-bit modes and bf16x6: no forward co-run, so nobody's guest; every data gradient is a launch of its own and the
  results are the same bits with the switch on and off."""
  batch = O.synthetic_batch(4, M=2, S=2, seed=15)
  res, merged, offered = _g_backward_runs(batch, 2, 2, prepare=_mode(mode))
  assert offered == {True: 0, False: 0} and merged == {True: 0, False: 0}, (offered, merged)
  _same_bits(res[True], res[False], mode)


def test_switches_between_forward_and_backward(monkeypatch):
  """An fp32 co-run forward marks the encoder's blocks as guests; what decides in the backward pass is the state THEN.  With
  bn_sync='global' reported active after the forward (or the co-run switched off) no data gradient is held back, and the results
  are those of the untouched pass.  The terms of the decision one by one, on a guest-able block: fp32 on, bf16x6 / bn_sync /
  either switch / a float64 gradient off."""
  from mix_stage_amd import ops
  M = S = 2
  audio, pose, labels, style = [t.to(DEV) for t in O.synthetic_batch(4, M=M, S=S, seed=16)]

  def run(between):
    model = _gan(M, S)
    G = model.G
    G.train(True)
    model.zero_grad()
    torch.manual_seed(7)
    pose_out, losses = G([audio, labels], pose, **O.model_kwargs(style))
    total = sum(losses[1:], losses[0])
    before = ops._corun['bwd_offered']
    with monkeypatch.context() as mp:
      between(mp)
      lab = _labels(total.backward)
    assert not ops._corun['bwd_keep']
    grads = {n: p.grad.detach().clone() for n, p in G.named_parameters() if p.grad is not None}
    return grads, ops._corun['bwd_offered'] - before, _bwd_merged(lab)
  plain, offered, merged = run(lambda mp: None)
  assert offered > 0 and merged > 0
  for what, between in (('bn_sync', lambda mp: mp.setattr(ops, 'bn_sync_active', lambda: True)),
                        ('corun off', lambda mp: mp.setitem(ops._corun, 'on', False))):
    got, offered, merged = run(between)
    assert offered == 0 and merged == 0, (what, offered, merged)
    _equal_dicts(plain, got, what)
  # the terms of ops._bwd_guest_ok
  L = _L()
  lib = L.lib()
  d = L.ConvDesc(8, 64, 1, 16, 64, 1, 1, 4, 1, 2, 0, 1, 1, 8, 2, L.MS_IN_PLAIN, 0.2, 1e-5, 0.1, 0)
  dy = torch.zeros(8, 64, 8, device=DEV)
  assert ops._bwd_guest_ok(d, dy)
  old = lib.ms_set_precision(1)
  try:
    assert not ops._bwd_guest_ok(d, dy)
  finally:
    lib.ms_set_precision(old)
  with monkeypatch.context() as mp:
    mp.setattr(ops, 'bn_sync_active', lambda: True)
    assert not ops._bwd_guest_ok(d, dy)
  for key in ('on', 'bwd_on'):
    with monkeypatch.context() as mp:
      mp.setitem(ops._corun, key, False)
      assert not ops._bwd_guest_ok(d, dy)
  assert not ops._bwd_guest_ok(d, dy.double()) and ops._bwd_guest_ok(d, dy)
  k5 = L.ConvDesc(8, 64, 1, 16, 64, 1, 1, 5, 1, 1, 0, 1, 1, 14, 2, L.MS_IN_PLAIN, 0.2, 1e-5, 0.1, 0)
  assert not ops._bwd_guest_ok(k5, torch.zeros(8, 64, 14, device=DEV))


def test_global_bn_two_ranks_make_the_backward_corun_stand_aside():
  """bn_sync='global' needs ranks: two of them (gloo, both on this device) run the generator forward and backward with the switch on
  and off (tests/helpers/dp_corun_bwd_worker.py).  No forward co-run, no data gradient held back, no merged label, and each rank's
  gradients, buffers and losses are the same bits either way."""
  import os
  import sys
  from test_gpu_dp import ROOT, _run_ranks
  env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
  cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
         '--master-port', '29561', os.path.join(ROOT, 'tests', 'helpers', 'dp_corun_bwd_worker.py')]
  out, res = _run_ranks(cmd, env)
  assert out.returncode == 0 and len(res) == 2, (out.stdout[-2000:], out.stderr[-4000:])
  for r in res:
    assert r['bn_sync_active'] is True
    assert r['offered'] == {'on': 0, 'off': 0} and r['merged'] == {'on': 0, 'off': 0} and r['fwd_offered'] == {'on': 0, 'off': 0}, r
    assert r['n_tensors'] > 100 and r['digest']['on'] == r['digest']['off'], (r['rank'], r['digest'])


@pytest.mark.parametrize('where', ['encoder', 'unet'])
def test_hooked_block_makes_the_backward_corun_stand_aside(where):
  """A hooked block of either module: the forward co-run stands aside, the encoder's blocks are nobody's guests, and the backward
  pass launches every data gradient on its own: the same bits with the switch on and off.  (Against the unhooked model only the
  UNet case is bit for bit: a hooked encoder block also keeps its BatchNorm backward out of its consumer's data gradient --
  layers._chain_ok -- which is another, equally exact, arithmetic.)"""
  batch = O.synthetic_batch(4, M=2, S=2, seed=12)
  seen = []
  pick = (lambda m: m.G.pose_style_encoder.conv[2]) if where == 'encoder' else (lambda m: m.G.unet.conv1[2])
  hook = lambda model: pick(model).register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
  hooked, merged, offered = _g_backward_runs(batch, 2, 2, hook=hook)
  assert len(seen) >= 2 and offered == {True: 0, False: 0} and merged == {True: 0, False: 0}, (seen, offered, merged)
  _equal_dicts(hooked[True], hooked[False], 'hooked ' + where + ', switch on and off')
  if where == 'unet':
    plain, _, _ = _g_backward_runs(batch, 2, 2)
    _equal_dicts(plain[True], hooked[True], 'hooked unet against the unhooked model')


def test_three_train_steps_graphs_equal_eager_with_the_backward_corun(trainer_globals_restored):  # noqa: F811
  from mix_stage_amd import ops
  from mix_stage_amd.train_step import MixStageTrainStep
  M = S = 2
  batches = [O.synthetic_batch(4, M=M, S=S, seed=60 + i) for i in range(3)]
  kinds = ['G', 'D', 'G']
  results = {}
  assert ops._corun['bwd_on'] and ops._corun['on']
  for use_graphs in (False, True):
    torch.manual_seed(99)
    model = _gan(M, S)
    ts = MixStageTrainStep(model, use_graphs=use_graphs)
    before = ops._corun['bwd_offered']
    got = []
    for rep in range(2 if use_graphs else 1):        # (with graphs the second pass is pure replay)
      if rep == 1:
        model.load_state_dict(O.deterministic_state(model.state_dict()))
        for o in (ts.optim_G, ts.optim_D):
          o.reset_state()
        got = []
      for (audio, pose, labels, style), k in zip(batches, kinds):
        ts.step(audio.to(DEV), labels.to(DEV), pose.to(DEV), style.to(DEV), kind=k)
        got.append([float(l) for l in ts.losses])
    assert ops._corun['bwd_offered'] > before and not ops._corun['bwd_keep']
    results[use_graphs] = (got, {k: v.clone() for k, v in model.state_dict().items()})
  assert results[True][0] == results[False][0]
  for k, v in results[False][1].items():
    assert torch.equal(v, results[True][1][k]), k


def _planned_bwd_pairs(G, B, T):
  """The pairs the backward pass finds, from ms_clip_grid / ms_clip_pair_ok (which UNet block carried which encoder block in the
  forward pass: the driver's rule) and ms_clip_dgrad_grid / ms_clip_dgrad_pair_ok: autograd runs the nodes latest-created first, so
  the data gradient of encoder block g + 1 -- carried by UNet block h + 1 -- comes directly in front of block h's, which carried g."""
  L = _L()
  lib = L.lib()
  cus = torch.cuda.get_device_properties(0).multi_processor_count

  def desc(cin, cout, W, k, s, up2=False):
    To = (W + 2 - k) // s + 1
    return L.ConvDesc(B, cin, 1, W, cout, 1, 1, k, 1, s, 0, 1, 1, To, 2, L.MS_IN_UP2ADD if up2 else L.MS_IN_PLAIN, 0.2, 1e-5, 0.1, 0), To
  guests, W = [], T
  for m in G.pose_style_encoder.conv:
    c = m.conv
    d, W = desc(c.in_channels, c.out_channels, W, c.kernel_size[0], c.stride[0])
    guests.append(d)
  hosts, W = [], T
  for m in G.unet.conv1:
    d, W = desc(256, 256, W, 4, 2)
    hosts.append(d)
  for m in G.unet.conv2:
    W *= 2
    hosts.append(desc(256, 256, W, 3, 1, up2=True)[0])
  ref = ctypes.byref
  carried, gi = {}, 0
  for hi, h in enumerate(hosts):
    if gi < len(guests):
      nh, ng = lib.ms_clip_grid(ref(h)), lib.ms_clip_grid(ref(guests[gi]))
      if nh and ng and nh + ng <= cus and lib.ms_clip_pair_ok(ref(h), ref(guests[gi])):
        carried[hi] = gi
        gi += 1
  pairs = 0
  for hi, g in carried.items():
    if carried.get(hi + 1) == g + 1:
      nh, ng = lib.ms_clip_dgrad_grid(ref(hosts[hi])), lib.ms_clip_dgrad_grid(ref(guests[g + 1]))
      if nh and ng and nh + ng <= cus and lib.ms_clip_dgrad_pair_ok(ref(hosts[hi]), ref(guests[g + 1])):
        pairs += 1
  return pairs


def test_the_backward_corun_is_not_vacuous():
  """At the headline batch the plan has at least four merged data gradients, and the launch labels of a real backward pass show
  at least as many."""
  M = S = 8
  model = _gan(M, S)
  batch = O.synthetic_batch(32, M=M, S=S, seed=13)
  planned = _planned_bwd_pairs(model.G, 32, 64)
  labels = _labels(lambda: _g_forward(model, batch, True, backward=True))
  merged = _bwd_merged(labels)
  assert planned >= 4, planned
  assert merged >= planned, (merged, planned, sorted(labels))
  if torch.cuda.get_device_properties(0).multi_processor_count == 256:
    assert planned == 6 and merged == 6, (merged, planned, sorted(labels))
