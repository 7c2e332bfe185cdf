"""GPU: two independent clip-resident forward blocks in ONE launch (ms_clip_hold; csrc/clip32.hip: clip32_pair_kernel) -- the
PoseStyleEncoder's blocks inside the UNet's half-empty launches.  A merged launch runs the same bodies on the same arguments, so
every comparison here is bit for bit against the two blocks launched one by one."""
import ctypes

import pytest
import torch

from oracle import mixstage_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAIR_MARK = '>+<'       # a merged launch's label: clip32_kernel<host>+<guest>|host description + guest description


def _L():
  from mix_stage_amd import _lib
  return _lib


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Block:
  """One 1-D conv block through the C-ABI with buffers of its own (scratch and meeting counters included)."""

  def __init__(self, B, cin, cout, T, k, s, mode, up2=False, seed=0, sync=True):
    L = _L()
    g = torch.Generator().manual_seed(seed)
    self.up2 = up2
    To = (T + 2 - k) // s + 1
    self.d = L.ConvDesc(B, cin, 1, T, cout, 1, 1, k, 1, s, 0, 1, 1, To, mode, L.MS_IN_UP2ADD if up2 else L.MS_IN_PLAIN, 0.2, 1e-5, 0.1, 0)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    self.x = rnd(B, cin, T // 2 if up2 else T)
    self.x2 = rnd(B, cin, T) if up2 else None
    self.w = rnd(cout, cin, k) * (1.0 / (cin * k) ** 0.5)
    self.bias, self.gamma, self.beta = rnd(cout) * 0.1, 1 + 0.1 * rnd(cout), 0.1 * rnd(cout)
    self.rm, self.rv = 0.1 * rnd(cout), 1 + 0.1 * rnd(cout).abs()
    self.y = torch.zeros(B, cout, To, device=DEV)
    self.y_raw = torch.zeros_like(self.y)            # (BN_TRAIN writes it only where the backward cannot invert y: zeros elsewhere)
    self.save = torch.zeros(4 * cout, device=DEV)
    self.ws = torch.zeros(max(256, L.lib().ms_conv_block_fwd_workspace(ctypes.byref(self.d))), dtype=torch.uint8, device=DEV)
    self.sync = torch.zeros(1024, dtype=torch.int32, device=DEV) if sync else None

  def grid(self):
    return _L().lib().ms_clip_grid(ctypes.byref(self.d))

  def run(self):
    L = _L()
    opt = L.FwdOptions(None, _ptr(self.sync), self.sync.numel() if self.sync is not None else 0)
    L.check(L.lib().ms_conv_block_fwd_ex(ctypes.byref(self.d), _ptr(self.x), _ptr(self.x2), _ptr(self.w), _ptr(self.bias), _ptr(self.gamma),
                                         _ptr(self.beta), _ptr(self.rm), _ptr(self.rv), _ptr(self.y_raw), _ptr(self.y), _ptr(self.save),
                                         _ptr(self.ws), self.ws.numel(), _stream(), ctypes.byref(opt)), 'ms_conv_block_fwd_ex')

  def state(self):
    out = [self.y, self.y_raw, self.save, self.rm, self.rv]
    return [t.clone() for t in out] + ([self.sync.clone()] if self.sync is not None else [])


def _held_then(guest, host):
  """guest held, host launched, flush: what the co-run driver does around one host block."""
  L = _L()
  L.check(L.lib().ms_clip_hold(_stream()), 'ms_clip_hold')
  try:
    guest.run()
    host.run()
    L.check(L.lib().ms_clip_hold_flush(_stream()), 'ms_clip_hold_flush')
  except BaseException:
    L.lib().ms_clip_hold_discard(_stream())
    raise


def _labels(fn):
  from mix_stage_amd import ops
  ops.timing_enable(True)
  try:
    fn()
    torch.cuda.synchronize()
    rows = ops.timing_report()
  finally:
    ops.timing_enable(False)
  return {r['label']: r['count'] for r in rows if r['label'].startswith('clip32_kernel<')}


def _same(a, b, what):
  names = ('y', 'y_raw', 'save', 'running_mean', 'running_var', 'sync words')
  for n, u, v in zip(names, a, b):
    assert torch.equal(u, v), '%s: %s differs' % (what, n)
  assert not torch.isnan(a[0]).any(), '%s: NaN output (an in-launch meeting gave up)' % what


# the path's instances: hosts = a UNet1D down / up block (256 -> 256), guests = the PoseStyleEncoder's blocks by channel groups per wave
HOSTS = {'down8': dict(cin=256, cout=256, k=4, s=2, up2=False), 'up8': dict(cin=256, cout=256, k=3, s=1, up2=True)}
GUESTS = {'k3_104to64': dict(cin=104, cout=64, k=3, s=1), 'down_64to128': dict(cin=64, cout=128, k=4, s=2),
          'down_128to256': dict(cin=128, cout=256, k=4, s=2), 'down_256to256': dict(cin=256, cout=256, k=4, s=2)}
MODES = {'train': 2, 'eval': 3}


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('guest', sorted(GUESTS))
@pytest.mark.parametrize('host', sorted(HOSTS))
def test_pair_equals_the_two_launches_bitwise(host, guest, mode):
  """B = 4, T = 32: both blocks have two pixel workgroups per channel tile, so each BN_TRAIN block really meets inside the launch.
  Three rounds: the meeting counters are monotonic, a merged launch must advance each block's as a launch of its own does."""
  make = lambda: (Block(4, T=32, mode=MODES[mode], seed=1, **HOSTS[host]), Block(4, T=32, mode=MODES[mode], seed=2, **GUESTS[guest]))
  (h1, g1), (h2, g2) = make(), make()
  assert h1.grid() == 16 and g1.grid() >= 4 and g1.grid() == 2 * ((GUESTS[guest]['cout'] + 31) // 32)
  assert _L().lib().ms_clip_pair_ok(ctypes.byref(h1.d), ctypes.byref(g1.d)) == 1

  def alone():
    for _ in range(3):
      g1.run(); h1.run()
      states_alone.append((h1.state(), g1.state()))

  def paired():
    for _ in range(3):
      _held_then(g2, h2)
      states_pair.append((h2.state(), g2.state()))
  states_alone, states_pair = [], []
  la, lp = _labels(alone), _labels(paired)
  assert sum(la.values()) == 6 and not any(PAIR_MARK in k for k in la), la
  assert sum(lp.values()) == 3 and all(PAIR_MARK in k for k in lp), lp
  for r, ((ha, ga), (hp, gp)) in enumerate(zip(states_alone, states_pair)):
    _same(ha, hp, 'round %d host' % r)
    _same(ga, gp, 'round %d guest' % r)
  if mode == 'train':
    assert int(h2.sync[0]) == 0 and int(g2.sync[0]) == 0                       # (no meeting gave up)
    assert int(h2.sync[32:].sum()) > 0 and int(g2.sync[32:].sum()) > 0         # (... and both blocks did meet)


def _no_merge_case(name):
  T = 32
  if name == 'over_cus':              # a full-resolution UNet block of 32 clips is 256 workgroups: no room on 256 compute units
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 32
    while 8 * (B * 32 // 32) + 2 * (B * 32 // 64) <= cus:
      B *= 2
    return Block(B, T=64, mode=2, seed=1, **HOSTS['down8']), Block(B, T=32, mode=2, seed=2, **GUESTS['k3_104to64'])
  if name == 'host_grid_not_8':       # 96 output channels: 3 channel tiles x 2 pixel workgroups
    return Block(4, 256, 96, T, 4, 2, 2, seed=1), Block(4, T=T, mode=2, seed=2, **GUESTS['k3_104to64'])
  if name == 'no_instance':           # a k3 s1 plain-input host (the UNet's pre-downsampling blocks) has no pair instance
    return Block(4, 256, 256, T, 3, 1, 2, seed=1), Block(4, T=T, mode=2, seed=2, **GUESTS['k3_104to64'])
  if name == 'guest_not_clip':        # a k5 block runs the other kernels: launched at once, the hold is disarmed
    return Block(4, T=T, mode=2, seed=1, **HOSTS['down8']), Block(4, 64, 64, T, 5, 1, 2, seed=2)
  assert name == 'knob_off'
  return Block(4, T=T, mode=2, seed=1, **HOSTS['down8']), Block(4, T=T, mode=2, seed=2, **GUESTS['k3_104to64'])


@pytest.mark.parametrize('name', ['over_cus', 'host_grid_not_8', 'no_instance', 'guest_not_clip', 'knob_off'])
def test_no_merge_same_bits_and_two_plain_launches(name):
  L = _L()
  (h1, g1), (h2, g2) = _no_merge_case(name), _no_merge_case(name)
  old = L.lib().ms_debug_set_clip_corun(0) if name == 'knob_off' else None
  try:
    la = _labels(lambda: (g1.run(), h1.run()))
    lp = _labels(lambda: _held_then(g2, h2))
  finally:
    if old is not None:
      L.lib().ms_debug_set_clip_corun(old)
  assert not any(PAIR_MARK in k for k in lp), lp
  assert lp == la, (lp, la)
  if name == 'guest_not_clip':
    assert g1.grid() == 0 and sum(lp.values()) == 1, lp           # (only the host is on the clip path)
  else:
    assert g1.grid() > 0 and h1.grid() > 0 and sum(lp.values()) == 2, lp
    if name != 'knob_off':
      assert L.lib().ms_clip_pair_ok(ctypes.byref(h1.d), ctypes.byref(g1.d)) == 0
  _same(h1.state(), h2.state(), name + ' host')
  _same(g1.state(), g2.state(), name + ' guest')


def test_flush_discard_and_second_hold():
  L = _L()
  lib = L.lib()
  # hold, explicit flush, then a launch of the library that is no conv block and reads the held block's output
  from mix_stage_amd import ops
  g1, g2 = (Block(4, T=32, mode=2, seed=2, **GUESTS['k3_104to64']) for _ in range(2))
  g1.run()
  want = ops.to_time_major(g1.y)
  L.check(lib.ms_clip_hold(_stream()), 'ms_clip_hold')
  g2.run()
  L.check(lib.ms_clip_hold_flush(_stream()), 'ms_clip_hold_flush')
  got = ops.to_time_major(g2.y)
  _same(g1.state(), g2.state(), 'flush')
  assert torch.equal(want, got)
  # hold, then discard: nothing is launched
  g3 = Block(4, T=32, mode=2, seed=2, **GUESTS['k3_104to64'])
  before = g3.state()

  def held_and_dropped():
    L.check(lib.ms_clip_hold(_stream()), 'ms_clip_hold')
    g3.run()
    lib.ms_clip_hold_discard(_stream())
    L.check(lib.ms_clip_hold_flush(_stream()), 'ms_clip_hold_flush')       # (nothing left to launch)
  assert _labels(held_and_dropped) == {}
  torch.cuda.synchronize()
  _same(before, g3.state(), 'discard')
  # a second hold while a block is pending is an error, and leaves the pending block alone
  L.check(lib.ms_clip_hold(_stream()), 'ms_clip_hold')
  g3.run()
  assert lib.ms_clip_hold(_stream()) != 0
  assert b'pending' in lib.ms_last_error()
  L.check(lib.ms_clip_hold_flush(_stream()), 'ms_clip_hold_flush')
  torch.cuda.synchronize()
  _same(g1.state(), g3.state(), 'flush after the refused hold')


# ---------------------------------------------------------------------------------------------------------------------------
# model level
def _gan(M, S):
  from test_gpu_model import build_hip_gan
  return build_hip_gan(M, S)


def _g_forward(model, batch, train, backward):
  audio, pose, labels, style = [t.to(DEV) for t in batch]
  G = model.G
  G.train(train)
  model.zero_grad()
  torch.manual_seed(7)                 # (the host-side draw of JL:127)
  with torch.set_grad_enabled(backward):
    pose_out, losses = G([audio, labels], pose, **O.model_kwargs(style))
    if backward:
      total = 0
      for l in losses:
        total = total + l
      total.backward()
  out = {'pose': pose_out.detach().clone(), 'labels_cap_soft': G.labels_cap_soft.detach().clone()}
  for i, l in enumerate(losses):
    out['loss%d' % i] = l.detach().clone()
  for n, b in G.state_dict().items():
    if 'running_' in n or 'num_batches' in n:
      out['buf/' + n] = b.detach().clone()
  if backward:
    for n, p in G.named_parameters():
      if p.grad is not None:
        out['grad/' + n] = p.grad.detach().clone()
  return out


def _equal_dicts(a, b, what):
  assert sorted(a) == sorted(b), what
  for k in a:
    assert torch.equal(a[k], b[k]), '%s: %s differs' % (what, k)


@pytest.mark.parametrize('train,backward', [(True, True), (True, False), (False, False)], ids=['train', 'train_no_grad', 'eval'])
def test_generator_forward_with_and_without_the_corun(train, backward):
  """The small golden configuration (B = 4, T = 64, M = S = 8): pose, internal losses, labels_cap_soft, BatchNorm buffers and, in
  train mode, every parameter gradient are the same bits with the style encoder riding in the UNet's launches and without.
  train_no_grad is the generator's pass of a D-step: nothing but the driver keeps a held block's y_raw / save / input allocated."""
  from mix_stage_amd import ops
  M = S = 8
  batch = O.synthetic_batch(4, M=M, S=S, seed=11)
  res = {}
  for on in (True, False):
    model = _gan(M, S)
    old = ops.enable_corun(on)
    try:
      before = ops._corun['merges_offered']
      res[on] = _g_forward(model, batch, train, backward=backward)
      assert not ops._corun['keep']          # (what a held block's launch touches is let go once it is on the stream)
      offered = ops._corun['merges_offered'] - before
    finally:
      ops.enable_corun(old)
    assert (offered > 0) == on
  _equal_dicts(res[True], res[False], 'train' if train else 'eval')


def test_hooked_block_makes_the_corun_stand_aside():
  from mix_stage_amd import ops
  M = S = 8
  batch = O.synthetic_batch(4, M=M, S=S, seed=12)
  plain = _g_forward(_gan(M, S), batch, True, backward=True)
  model = _gan(M, S)
  seen = []
  h = model.G.unet.conv1[2].register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
  try:
    before = ops._corun['merges_offered']
    hooked = _g_forward(model, batch, True, backward=True)
    assert ops._corun['merges_offered'] == before and len(seen) == 1
  finally:
    h.remove()
  _equal_dicts(plain, hooked, 'hooked')


@pytest.fixture
def trainer_globals_restored():
  """MixStageTrainStep switches the trainer's process-wide modes on (prepared weights, deferred weight gradients): off again for the
  tests that run after this file."""
  from mix_stage_amd import ops
  yield
  ops.enable_prepared_weights(False)
  ops.enable_deferred_wgrad(False)


def test_three_train_steps_graphs_equal_eager_with_the_corun(trainer_globals_restored):
  from mix_stage_amd.train_step import MixStageTrainStep
  M = S = 8
  batches = [O.synthetic_batch(4, M=M, S=S, seed=60 + i) for i in range(3)]
  kinds = ['G', 'D', 'G']
  results = {}
  for use_graphs in (False, True):
    torch.manual_seed(99)
    model = _gan(M, S)
    ts = MixStageTrainStep(model, use_graphs=use_graphs)
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
    results[use_graphs] = (got, {k: v.clone() for k, v in model.state_dict().items()})
  assert results[True][0] == results[False][0]
  for k, v in results[False][1].items():
    assert torch.equal(v, results[True][1][k]), k


def _planned_pairs(G, B, T, train):
  """The pairs the driver's rule finds, from ms_clip_grid: the UNet's down and up blocks in order, each taking the style encoder's
  next block when both run the clip-resident kernel, the host's grid is a multiple of 8 and the two fit the device together."""
  L = _L()
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  mode = 2 if train else 3

  def grid(cin, cout, W, k, s, up2=False):
    To = (W + 2 - k) // s + 1
    d = L.ConvDesc(B, cin, 1, W, cout, 1, 1, k, 1, s, 0, 1, 1, To, mode, L.MS_IN_UP2ADD if up2 else L.MS_IN_PLAIN, 0.2, 1e-5, 0.1, 0)
    return L.lib().ms_clip_grid(ctypes.byref(d)), To
  guests, W = [], T
  for m in G.pose_style_encoder.conv:
    c = m.conv
    n, W2 = grid(c.in_channels, c.out_channels, W, c.kernel_size[0], c.stride[0])
    guests.append(n)
    W = W2
  hosts, W = [], T
  for m in G.unet.conv1:
    n, W = grid(256, 256, W, 4, 2)
    hosts.append(n)
  for m in G.unet.conv2:
    W *= 2
    hosts.append(grid(256, 256, W, 3, 1, up2=True)[0])
  pairs, gi = 0, 0
  for n in hosts:
    if gi < len(guests) and n and guests[gi] and n % 8 == 0 and n + guests[gi] <= cus:
      pairs += 1
      gi += 1
  return pairs, len(guests)


@pytest.mark.parametrize('B', [32, 4])
def test_the_corun_is_not_vacuous(B):
  """With timing on, the generator forward reports a merged launch for all seven style-encoder blocks at the headline batch on a
  256-CU device, and at B = 4 at least as many as the rule finds room for."""
  M = S = 8
  model = _gan(M, S)
  batch = O.synthetic_batch(B, M=M, S=S, seed=13)
  planned, n_guests = _planned_pairs(model.G, B, 64, True)
  labels = _labels(lambda: _g_forward(model, batch, True, backward=False))
  merged = sum(c for k, c in labels.items() if PAIR_MARK in k)
  assert n_guests == 7 and planned > 0
  assert merged >= planned, (merged, planned, sorted(labels))
  if B == 32 and torch.cuda.get_device_properties(0).multi_processor_count == 256:
    assert planned == 7 and merged == 7, (merged, planned, sorted(labels))
