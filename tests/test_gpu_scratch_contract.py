"""GPU: the C-ABI's scratch contract -- the caller hands every call exactly the bytes its size function names, with unspecified
contents -- checked for every scratch-taking entry point on exactly-sized, poisoned, guarded buffers (helpers/guarded_scratch.py).

Everywhere else in the suite a block's scratch comes from ops.workspace(): at least 4 MiB, 1.5 x the request, shared by all blocks of
the stream and never cleared.  A launch that touches bytes past its claimed size, or that reads a slab it did not write, computes
the right answer there.  Here each case runs three times -- on that roomy scratch, and on exact scratch poisoned with 0xFF (NaN in
every float format, -1 as a counter) and with 0x55 (finite, absurd) -- and asserts
  - both guards of every buffer intact (an overrun lands in memory the test owns and is named by its offsets),
  - the same launch labels in the three runs,
  - every result bit for bit equal in the three runs (the kernels reduce in a fixed order; no entry is exempt),
  - the case's own fp64 bars in all three runs,
  - that the case is not vacuous: the exact workspace was written, or the entry is on UNUSED with the reason.
a. all entries of helpers/dispatch_table.py; b. the chained decoder (train, 16-bit, eval forms), ms_bn_bwd_sums, a co-run pair, a
block with its weight gradient on a side stream, blocks in trainer mode (prepared weights, deferred weight gradients);
c. the scratch arguments of the loss / optimizer entry points; d. a workspace one byte short is refused before anything is touched.

The per-entry high-water mark (highest byte written / claimed bytes, from the 0x55 run) is printed; with MS_SCRATCH_HIGHWATER_OUT
set to a path the table is written there as JSON (profiles/scratch_highwater.json is that file)."""
import ctypes
import json
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

from helpers.dispatch_table import TABLE
from helpers.ew_table import BY_ID as EW
from helpers.guarded_scratch import POISONS, exact_scratch, guarded, guard_damage, touched
from test_gpu_dispatch_parity import MODES, _deterministic, _nd_kernel, check_labels, rel_err, run_entry

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BY_ID = {e['id']: e for e in TABLE}

# Calls whose size function claims scratch that the path they take never writes: (id, 'fwd' | 'bwd') -> why.  (Checked both ways: a
# call listed here that does write its workspace fails as well.)
_FRONT = ("a forward without BatchNorm statistics, split-K slab or bf16x6 planes: the claim is FwdPlan's 256-byte front, which is sized "
          "for every kernel family, plus the 256-byte tail; the gather / patch kernel of this path writes neither")
UNUSED = {(i, 'fwd'): _FRONT for i in ('act_1025', 'act_2049', 'act_4097', 'act_bare_4097', 'logits_g8', 'c4_logits_g25')}

HIGHWATER = {}


@pytest.fixture(autouse=True)
def _stop_on_a_faulted_device():
  """A device fault (an overrun past the guards would be one) ends the session here: nothing more is launched on that device."""
  try:
    torch.cuda.synchronize()
  except RuntimeError as err:
    pytest.exit('the device reported a fault before this case: %s' % err, returncode=3)
  yield


@pytest.fixture(autouse=True)
def _trainer_modes_off():
  """Every case starts with the process-wide trainer modes off (prepared weights, deferred weight gradients): a MixStageTrainStep
  of an earlier test file leaves them on, and a table entry would then take the trainer's launches (transpose_weight_multi)
  instead of the ones it exists for.  The cases that want them switch them on themselves; what was on before is on again after."""
  from mix_stage_amd import ops
  was = (ops._prepared['on'], ops._deferred['on'])
  if was[0]:
    ops.enable_prepared_weights(False)
  if was[1]:
    ops.enable_deferred_wgrad(False)
  yield
  if ops._prepared['on'] != was[0]:
    ops.enable_prepared_weights(was[0])
  if ops._deferred['on'] != was[1]:
    ops.enable_deferred_wgrad(was[1])


def _flat(obj, prefix=''):
  """[(name, tensor or None)] of a nested dict / list / tuple of tensors."""
  if isinstance(obj, dict):
    return [r for k in sorted(obj) for r in _flat(obj[k], '%s%s.' % (prefix, k))]
  if isinstance(obj, (list, tuple)):
    return [r for i, v in enumerate(obj) for r in _flat(v, '%s%d.' % (prefix, i))]
  return [(prefix.rstrip('.'), obj)]


def _assert_same_bits(runs, names, what):
  """Every tensor of runs[1:] equals that of runs[0] bit for bit."""
  first = _flat(runs[0])
  for run, name in zip(runs[1:], names[1:]):
    got = _flat(run)
    assert [n for n, _ in got] == [n for n, _ in first], (what, name)
    diff = []
    for (n, a), (_, b) in zip(first, got):
      if a is None or b is None or not torch.is_tensor(a):
        same = (a is None and b is None) or (not torch.is_tensor(a) and a == b)
      else:
        same = a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
      if not same:
        nan = torch.is_tensor(b) and b.is_floating_point() and not bool(torch.isfinite(b).all())
        diff.append(n + (' (non-finite)' if nan else ''))
    assert not diff, '%s: %s differs from %s in %s' % (what, name, names[0], diff)


def _three(monkeypatch, fn):
  """fn() on roomy scratch and under both poisons -> ([results], [Scratch records of the two exact runs])."""
  out, recs = [fn()], []
  for poison in POISONS:
    with exact_scratch(monkeypatch, poison) as rec:
      out.append(fn())
      torch.cuda.synchronize()
    recs.append(rec)
  return out, recs


RUN_NAMES = ['roomy scratch'] + ['exact scratch, poison 0x%02X' % p for p in POISONS]


def _written(recs, owner='workspace'):
  return any(f > 0 for rec in recs for _, f in rec.highwater(owner))


# ------------------------------------------------------------------------------------------------ a. + e. the dispatch table
@pytest.mark.parametrize('e', TABLE, ids=[e['id'] for e in TABLE])
def test_conv_block_on_exact_poisoned_scratch(e, monkeypatch):
  keeps, labels, errs = [], [], []

  def once():
    keep = {}
    l, r = run_entry(e, keep)
    keeps.append(keep); labels.append(l); errs.append(r)
  _, recs = _three(monkeypatch, once)
  for l in labels:
    check_labels(e, l)
  assert set(labels[1]) == set(labels[0]) and set(labels[2]) == set(labels[0]), \
      '%s: launches differ: %s' % (e['id'], [sorted(set(l)) for l in labels])
  _assert_same_bits(keeps, RUN_NAMES, e['id'])
  for name, r in zip(RUN_NAMES, errs):
    bad = {kk: v for kk, v in r.items() if not v[0] <= v[1]}
    assert not bad, '%s on %s: errors (value, bar): %s' % (e['id'], name, bad)
  if e['mode'] == 'BN_TRAIN':
    assert all(torch.is_tensor(k['save']) for k in keeps), 'the save vector dropped out of the comparison'
  assert all(torch.is_tensor(k['y']) for k in keeps)
  hws = [rec.highwater() for rec in recs]
  hw = hws[1]
  HIGHWATER[e['id']] = [[n, round(f, 4)] for n, f in hw]
  print('SCRATCH %-28s %s' % (e['id'], ' '.join('%d B: %.3f' % (n, f) for n, f in hw)))
  assert len(hw) == (1 if e['mode'] == 'BN_EVAL' else 2) and [n for n, _ in hws[0]] == [n for n, _ in hw], (hws, 'one workspace per call')
  # not vacuous, call by call: the forward's and the backward's exact workspace was written under at least one poison
  for i, call in enumerate(('fwd', 'bwd')[:len(hw)]):
    written = hws[0][i][1] > 0 or hws[1][i][1] > 0
    if (e['id'], call) in UNUSED:
      assert not written, '%s %s writes its workspace; take it off UNUSED' % (e['id'], call)
    else:
      assert written, '%s %s: no byte of the %d claimed workspace bytes changed' % (e['id'], call, hw[i][0])


def test_highwater_table_of_a_complete_run():
  """After a run of the whole table (this test follows its cases; a selection of the table checks nothing here): every entry has a
  row per call, and the file, when asked for, is written: one line per entry."""
  if not all(e['id'] in HIGHWATER for e in TABLE):
    return
  assert sorted(HIGHWATER) == sorted(e['id'] for e in TABLE)
  assert all(len(HIGHWATER[e['id']]) == (1 if e['mode'] == 'BN_EVAL' else 2) for e in TABLE)
  assert all(BY_ID[i]['mode'] not in ('BN_TRAIN',) or rows[0][1] > 0 for i, rows in HIGHWATER.items()), 'a BN_TRAIN forward keeps statistics in scratch'
  path = os.environ.get('MS_SCRATCH_HIGHWATER_OUT')
  if path:
    what = ('per conv-block dispatch entry: [claimed workspace bytes, highest byte written / claimed] of the forward, then the backward '
            'call (tests/test_gpu_scratch_contract.py, poison 0x55); information, not a bar')
    with open(path, 'w') as f:
      f.write('{"what": %s,\n "entries": {\n' % json.dumps(what))
      f.write(',\n'.join('  %s: %s' % (json.dumps(i), json.dumps(HIGHWATER[i])) for i in sorted(HIGHWATER)))
      f.write('\n}}\n')


# ------------------------------------------------------------------------------------------------ b. chains
def _chain_float64(blocks, logits, x, score, M, P, round_to):
  from test_gpu_chain import _segment_float64
  return _segment_float64(blocks, logits, x, score, M, P, round_to).detach(), torch.softmax(score.double().cpu().transpose(1, 2), -1)


CHAIN_CASES = [(8, 4, 104, 10), (5, 3, 16, 16)]          # B, M, P, cin0 - 256
_cid = lambda c: 'b%d_m%d_p%d_cin%d' % (c[0], c[1], c[2], 256 + c[3])


@pytest.mark.parametrize('case', CHAIN_CASES, ids=_cid)
def test_train_chain_fp32_on_exact_poisoned_scratch(case, monkeypatch):
  """ms_decoder_chain_fwd (train) and the blocks' backward pass behind it; forward against float64 as test_chain_against_float64."""
  from test_gpu_chain import _build, _close, _inputs, _run
  B, M, P, extra = case
  blocks, logits = _build(M, P, extra, seed=3)
  x, score = _inputs(B, M, 256 + extra, seed=3)
  dout = torch.randn(B, 64, P, generator=torch.Generator().manual_seed(5)).to(DEV)
  runs, recs = _three(monkeypatch, lambda: _run(blocks, logits, x, score, P, True, dout=dout))
  _assert_same_bits(runs, RUN_NAMES, 'train chain ' + _cid(case))
  assert _written(recs, 'chain_prepared') and _written(recs)
  print('SCRATCH chain32 %s workspace %s' % (_cid(case), recs[1].highwater()))
  ref, soft = _chain_float64(blocks, logits, x, score, M, P, torch.float32)
  for r in runs:
    assert float((r['out'].detach().cpu().double() - ref).abs().mean()) <= 2e-6
    _close(r['out'].cpu().double(), ref, 2e-5, 'mixture vs float64')
    _close(r['soft'].cpu().double(), soft, 1e-6, 'softmax vs float64')


@pytest.mark.parametrize('case', CHAIN_CASES, ids=_cid)
def test_chain16_bf16_on_exact_poisoned_scratch(case, monkeypatch):
  """The 16-bit chain; against float64 on the rounded operands with the bars of test_chain16_against_blocks_and_float64."""
  from test_gpu_chain import _build, _close, _inputs, _run16
  B, M, P, extra = case
  blocks, logits = _build(M, P, extra, seed=21)
  x, score = _inputs(B, M, 256 + extra, seed=21)
  dout = torch.randn(B, 64, P, generator=torch.Generator().manual_seed(6)).to(DEV)
  runs, recs = _three(monkeypatch, lambda: _run16(blocks, logits, x, score, P, True, 'bf16', dout=dout))
  _assert_same_bits(runs, RUN_NAMES, 'chain16 ' + _cid(case))
  assert _written(recs, 'chain_prepared') and _written(recs)
  print('SCRATCH chain16 %s workspace %s' % (_cid(case), recs[1].highwater()))
  b = _run16(blocks, logits, x, score, P, False, 'bf16', dout=dout)
  ref, _ = _chain_float64(blocks, logits, x, score, M, P, torch.bfloat16)
  eb, scale = float((b['out'].cpu().double() - ref).abs().mean()), float(ref.abs().mean())
  for r in runs:
    ea = float((r['out'].cpu().double() - ref).abs().mean())
    assert torch.isfinite(r['out']).all()
    assert ea <= 1.5 * eb + 1e-4 * scale and ea <= 3e-2 * scale, (ea, eb, scale)
    _close(r['soft'], b['soft'], 1e-6, 'softmax')


EVAL_CASES = [(2, 3, 100, 16, 16), (1, 8, 640, 104, 10)]       # B, M, T, P, cin0 - 256


@pytest.mark.parametrize('dt_name', [None, 'bf16'], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', EVAL_CASES, ids=lambda c: 'b%d_m%d_t%d_p%d' % c[:4])
def test_eval_chain_on_exact_poisoned_scratch(case, dt_name, monkeypatch):
  """ms_decoder_chain_eval_fwd; (2, 3, 100) spreads the groups of a tile over workgroups, whose partial sums live in the workspace.
  Against float64 with the bars of test_gpu_chain_eval."""
  from test_gpu_chain import _build, _close, _inputs
  from test_gpu_chain_eval import _eval, _segment_eval_float64
  B, M, T, P, extra = case
  blocks, logits = _build(M, P, extra, seed=41)
  x, score = _inputs(B, M, 256 + extra, seed=41, T=T)
  runs, recs = _three(monkeypatch, lambda: [t.clone() for t in _eval(blocks, logits, x, score, P, True, dt_name)])
  _assert_same_bits(runs, RUN_NAMES, 'eval chain %s %s' % (case, dt_name))
  print('SCRATCH chain_eval %s %s workspace %s' % (case, dt_name, recs[1].highwater()))
  assert _written(recs, 'chain_prepared')
  if (B, M, T) == (2, 3, 100):
    assert _written(recs), 'the spread plan left its workspace untouched'
  ref, soft_ref = _segment_eval_float64(blocks, logits, x, score, M, P, torch.bfloat16 if dt_name else None)
  if dt_name:
    out_b, soft_b = _eval(blocks, logits, x, score, P, False, dt_name)
    eb, scale = float((out_b.cpu().double() - ref).abs().mean()), float(ref.abs().mean())
  for out, soft in runs:
    assert torch.isfinite(out).all()
    if dt_name:
      ea = float((out.cpu().double() - ref).abs().mean())
      assert ea <= 1.5 * eb + 1e-4 * scale and ea <= 3e-2 * scale, (ea, eb, scale)
      _close(soft, soft_b, 1e-6, 'softmax')
    else:
      assert float((out.cpu().double() - ref).abs().mean()) <= 2e-6
      _close(out.cpu().double(), ref, 2e-5, 'mixture vs float64')
      _close(soft.cpu().double(), soft_ref, 1e-6, 'softmax vs float64')


# ------------------------------------------------------------------------------------------------ b. stand-alone users
def _p(t):
  return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
  from mix_stage_amd import _lib as L
  return L.lib()


@pytest.mark.parametrize('shape', [(2047, 1, 1), (3, 64, 683)], ids=lambda s: 'b%d_c%d_hw%d' % s)
def test_bn_bwd_sums_on_exact_poisoned_scratch(shape):
  """ms_bn_bwd_sums with exactly ms_bn_bwd_workspace(B, C) bytes: sums[C][2] = (sum dz, sum dz * xhat) against float64 with the
  derived bar of test_gpu_ew_parity (4 x the error of the float32 CPU evaluation, floored at 2 * 2^-24)."""
  from test_gpu_ew_parity import FLOOR, _two_metrics
  L = _lib()
  B, C, HW = shape
  gen = torch.Generator().manual_seed(B + C)
  x = torch.randn(B, C, HW, generator=gen) * (torch.rand(1, C, 1, generator=gen) + 0.5) + torch.randn(1, C, 1, generator=gen)
  dy = torch.randn(B, C, HW, generator=gen)
  gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
  slope = 0.2

  # save = mean | invstd | scale | shift, as the forward leaves it (float32 roundings of the float64 statistics)
  mean = x.double().mean((0, 2))
  invstd = 1.0 / ((x.double() - mean.reshape(1, C, 1)).pow(2).mean((0, 2)) + 1e-5).sqrt()
  save_c = torch.cat([mean, invstd, gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd]).float()
  save = save_c.to(DEV)
  xd, dyd = x.to(DEV), dy.to(DEV)
  nbytes = L.ms_bn_bwd_workspace(B, C)
  assert nbytes > 0
  outs, views = [], []
  for ws in [torch.empty(max(4 << 20, 2 * nbytes), dtype=torch.uint8, device=DEV)] + [guarded(nbytes, DEV, p) for p in POISONS]:
    sums = torch.full((C, 2), float('nan'), device=DEV)
    assert L.ms_bn_bwd_sums(_p(dyd), _p(xd), _p(save), _p(sums), B, C, HW, slope, _p(ws), nbytes if hasattr(ws, '_guard') else ws.numel(),
                            _stream()) == 0
    torch.cuda.synchronize()
    outs.append(sums)
    views.append(ws)
  for v in views[1:]:
    assert guard_damage(v) is None, guard_damage(v)
  assert any(touched(v) is not None for v in views[1:])
  _assert_same_bits(outs, RUN_NAMES, 'ms_bn_bwd_sums %s' % (shape,))
  # the function the kernel evaluates, on the float32 statistics it is handed: xhat = (x - mean) * invstd, the activation's sign
  # that of z = scale * x + shift (taken in float64: no |z| of these inputs is within the float32 rounding of that expression,
  # two roundings of 2^-24 relative to |scale * x| + |shift|, of 0)
  col = lambda i, dtype: save_c[i * C:(i + 1) * C].to(dtype).reshape(1, C, 1)
  sx = x.double() * col(2, torch.float64)
  z64 = sx + col(3, torch.float64)
  assert bool((z64.abs() > 2 * 2.0 ** -24 * (sx.abs() + col(3, torch.float64).abs())).all())
  pos = z64 > 0

  def sums_ref(dtype):
    xh = (x.to(dtype) - col(0, dtype)) * col(1, dtype)
    dz = dy.to(dtype) * torch.where(pos, torch.ones((), dtype=dtype), torch.tensor(slope, dtype=dtype))
    return torch.stack([dz.sum((0, 2)), (dz * xh).sum((0, 2))], 1)
  r64, r32 = sums_ref(torch.float64), sums_ref(torch.float32)
  for k, nm in enumerate(('sum dz', 'sum dz*xhat')):
    got, yard = _two_metrics(outs[0][:, k], r64[:, k]), _two_metrics(r32[:, k], r64[:, k])
    print('SCRATCH bn_bwd_sums %s %s: device %.3e / %.3e, float32 CPU %.3e / %.3e' % (shape, nm, got[0], got[1], yard[0], yard[1]))
    assert got[0] <= 4 * max(yard[0], FLOOR) and got[1] <= 4 * max(yard[1], FLOOR), (nm, got, yard)


def test_corun_pair_on_exact_poisoned_scratch():
  """One merged launch of test_gpu_clip_corun (host down8, guest k3_104to64, BN_TRAIN): host AND held guest on exactly-sized
  poisoned workspaces; as in that file the results are the bits of the two blocks launched one by one."""
  from test_gpu_clip_corun import GUESTS, HOSTS, PAIR_MARK, Block, _held_then, _labels, _same
  L = _lib()

  def make():
    return Block(4, T=32, mode=2, seed=1, **HOSTS['down8']), Block(4, T=32, mode=2, seed=2, **GUESTS['k3_104to64'])
  h0, g0 = make()
  g0.run(); h0.run()
  torch.cuda.synchronize()
  alone = (h0.state(), g0.state())
  for poison in (None,) + POISONS:
    h, g = make()
    for blk in (h, g):
      n = L.ms_conv_block_fwd_workspace(ctypes.byref(blk.d))
      blk.ws = torch.empty(4 << 20, dtype=torch.uint8, device=DEV) if poison is None else guarded(n, DEV, poison)
    labels = _labels(lambda: _held_then(g, h))
    assert sum(labels.values()) == 1 and all(PAIR_MARK in k for k in labels), labels
    what = 'roomy' if poison is None else 'poison 0x%02X' % poison
    _same(alone[0], h.state(), what + ' host')
    _same(alone[1], g.state(), what + ' guest')
    if poison is not None:
      for blk in (h, g):
        assert guard_damage(blk.ws) is None, guard_damage(blk.ws)
        assert touched(blk.ws) is not None


# ------------------------------------------------------------------------------------------------ b. blocks under a flat optimizer
@pytest.fixture
def trainer_globals_restored():
  from mix_stage_amd import ops
  yield
  ops.set_backward_overlap(None)
  ops.enable_prepared_weights(False)
  ops.enable_deferred_wgrad(False)


def _flat_block_runs(monkeypatch, geometry, how, dt_name=None):
  """One BN_TRAIN ConvNormRelu whose parameters live in a FlatAdam buffer (gradients written straight into the flat buffer),
  forward + backward three times.  how = 'overlap': weight gradient on a side stream with a side workspace
  (ops.set_backward_overlap); 'trainer': prepared weights + deferred weight gradients (what MixStageTrainStep switches on)."""
  import mix_stage_amd as A
  from mix_stage_amd import ops, ops16
  from mix_stage_amd.train_step import FlatAdam
  B, cin, cout, groups, k, s, p, T = geometry
  blk = _deterministic(A.ConvNormRelu(cin, cout, type='1d', leaky=True, kernel_size=k, stride=s, padding=p, groups=groups), 'blk.').to(DEV)
  blk.train()
  if dt_name:
    A.set_compute_dtype(blk, dt_name)
  opt = FlatAdam(list(blk.parameters()))
  gen = torch.Generator().manual_seed(17)
  x = torch.randn(B, cin * groups, T, generator=gen).to(DEV)
  To = (T + 2 * p - k) // s + 1
  gy = torch.randn(B, cout * groups, To, generator=gen).to(DEV)
  rm0, rv0 = blk.norm.running_mean.clone(), blk.norm.running_var.clone()
  side = torch.cuda.Stream()
  if how == 'trainer':
    ops.enable_prepared_weights(True)
    ops.enable_deferred_wgrad(True)

  def once():
    with torch.no_grad():
      blk.norm.running_mean.copy_(rm0); blk.norm.running_var.copy_(rv0)
    opt.zero_grad()
    xin = x.clone().requires_grad_()
    if how == 'overlap':
      ops.set_backward_overlap(side)
    try:
      h = ops16.to_cb8(xin, ops16.NAME_DT[dt_name]) if dt_name else xin
      y = blk(h)
      y32 = ops16.from_cb8(y, cout * groups) if dt_name else y
      y32.backward(gy)
      ops.join_backward_overlap()
    finally:
      ops.set_backward_overlap(None)
    torch.cuda.synchronize()
    return dict(y=y32.detach().clone(), dx=xin.grad.clone(), flat_g=opt.flat_g.clone(), rm=blk.norm.running_mean.clone(),
                rv=blk.norm.running_var.clone())
  runs, recs = _three(monkeypatch, once)
  grads = [g.clone() for g in opt._grad_views]            # (of the last run; equal to the others' by flat_g)
  return blk, x, gy, runs, recs, grads


def _block_float64_bars(blk, x, gy, run, grads, groups, stride, padding):
  """conv1d + batch-statistics BatchNorm + LeakyReLU(0.2) in float64, the slope mask taken from the device output; the bars of
  test_gpu_dispatch_parity (forward 2e-5, gradients 1e-4 of the tensor's max-abs)."""
  w, b, ga, be = [t.detach().double().clone().requires_grad_() for t in (blk.conv.weight, blk.conv.bias, blk.norm.weight, blk.norm.bias)]
  x64 = x.double().requires_grad_()
  raw = F.conv1d(x64, w, b, stride=stride, padding=padding, groups=groups)
  mean, var = raw.mean((0, 2), keepdim=True), raw.var((0, 2), unbiased=False, keepdim=True)
  z = (raw - mean) / torch.sqrt(var + 1e-5) * ga.view(1, -1, 1) + be.view(1, -1, 1)
  y_ref = torch.where(run['y'] > 0, z, 0.2 * z)
  y_ref.backward(gy.double())
  gw, _, gg, gb = grads
  errs = {'fwd': (rel_err(run['y'], y_ref), 2e-5), 'dx': (rel_err(run['dx'], x64.grad), 1e-4), 'dw': (rel_err(gw, w.grad), 1e-4),
          'dgamma': (rel_err(gg, ga.grad), 1e-4), 'dbeta': (rel_err(gb, be.grad), 1e-4)}
  bad = {kk: v for kk, v in errs.items() if not v[0] <= v[1]}
  assert not bad, 'errors (value, bar): %s' % bad


def _block16_float64_bars(blk, x, gy, run, grads, geometry, dt_name):
  """The 16-bit block against float64 on its 16-bit-rounded operands, slope mask from the device output: the reference and the bars of
  test_gpu_kernels16._case as helpers/wgrad_queue_checks.py restates them for a block that lives in a module (forward 1.2e-2,
  gradients 2e-2 in l2 and twice that in max-abs, running statistics 1e-4 / 2e-3)."""
  import mix_stage_amd as A
  from helpers import wgrad_queue_checks as C
  from helpers.wgrad_queue_table import Bk
  B, cin, cout, groups, k, s, p, T = geometry
  b = Bk(1, B, cin, cout, groups, k, s, p, (T,), prec=dt_name)
  fresh = _deterministic(A.ConvNormRelu(cin, cout, type='1d', leaky=True, kernel_size=k, stride=s, padding=p, groups=groups), 'blk.')
  params = dict(w=blk.conv.weight, bias=blk.conv.bias, gamma=blk.norm.weight, beta=blk.norm.bias)
  macs = B * groups * cout * cin * k * run['y'].shape[-1]
  ref = C.reference(b, params, [dict(xs=[x], gy=gy, y=run['y'])], fresh.norm.running_mean, fresh.norm.running_var, dev=DEV if macs > 5e8 else 'cpu')
  gw, gbias, gg, gb = grads
  got = dict(y=[run['y']], dx0=[run['dx']], dx1=[None], dw=gw, dbias=gbias, dgamma=gg, dbeta=gb, rm=run['rm'], rv=run['rv'])
  errs = C.bars(b, got, ref)
  assert 'dw l2' in errs and 'fwd[0]' in errs and 'running_var' in errs
  assert not C.failed(errs), 'errors (value, bar): %s' % C.failed(errs)


def test_block_with_backward_overlap_on_exact_poisoned_scratch(monkeypatch, trainer_globals_restored):
  """unet_pre's geometry at B = 32 with ops.set_backward_overlap: the weight gradient runs on the side stream with the side
  workspace (ms_conv_block_bwd_overlap), both workspaces exactly sized."""
  geometry = (32, 256, 256, 1, 3, 1, 1, 64)
  blk, x, gy, runs, recs, grads = _flat_block_runs(monkeypatch, geometry, 'overlap')
  assert all(any(o == 'side_workspace' for o, _ in rec.views) for rec in recs), 'the side-stream form did not run'
  print('SCRATCH overlap workspace %s side %s' % (recs[1].highwater(), recs[1].highwater('side_workspace')))
  _assert_same_bits(runs, RUN_NAMES, 'backward overlap')
  assert _written(recs, 'side_workspace'), 'the weight gradient on the side stream left its workspace unwritten'
  assert _written(recs)
  _block_float64_bars(blk, x, gy, runs[2], grads, 1, 1, 1)


@pytest.mark.parametrize('name,geometry,dt_name', [('unet_down64', (32, 256, 256, 1, 4, 2, 1, 64), None), ('dec1', (32, 256, 256, 8, 3, 1, 1, 64), None),
                                                   ('h16_dec1', (32, 256, 256, 8, 3, 1, 1, 64), 'bf16'), ('h16_unet_down64', (32, 256, 256, 1, 4, 2, 1, 64), 'bf16')],
                         ids=['unet_down64', 'dec1', 'h16_dec1', 'h16_unet_down64'])
def test_trainer_mode_block_on_exact_poisoned_scratch(name, geometry, dt_name, monkeypatch, trainer_globals_restored):
  """Prepared weights (ms_dgrad_weights_elems / ms_fwd_weights_bytes / ms_weights16_bytes) and deferred weight gradients
  (ms_wgrad_partials_elems, ms_wgrad_flush) on exactly-sized poisoned buffers of the caller, as MixStageTrainStep runs a block."""
  blk, x, gy, runs, recs, grads = _flat_block_runs(monkeypatch, geometry, 'trainer', dt_name)
  owners = sorted(set(o for rec in recs for o, _ in rec.views))
  print('SCRATCH trainer %s owners %s workspace %s' % (name, owners, recs[1].highwater()))
  assert any(o in ('prepared', 'prepared16', 'wgrad_partials') for o in owners), owners
  for o in owners:
    if o != 'workspace':
      assert _written(recs, o), '%s buffers of %s were never written' % (o, name)
  _assert_same_bits(runs, RUN_NAMES, 'trainer-mode ' + name)
  if not dt_name:
    _block_float64_bars(blk, x, gy, runs[2], grads, geometry[3], geometry[5], geometry[6])
  else:
    _block16_float64_bars(blk, x, gy, runs[2], grads, geometry, dt_name)


# ------------------------------------------------------------------------------------------------ c. loss / optimizer scratch
@pytest.mark.parametrize('n', [2049, 2101249])
@pytest.mark.parametrize('squared', [0, 1], ids=['l1', 'l2'])
def test_lp_mean_partials_exactly_sized(n, squared):
  """ms_l1_mean_fwd / ms_l2_mean_fwd with ms_reduce_partials_count(n) poisoned floats; loss within 1e-6 of float64 (the bar of
  test_gpu_ew_parity's lp_mean cases), with `b` and with `target`."""
  L = _lib()
  fn = L.ms_l2_mean_fwd if squared else L.ms_l1_mean_fwd
  gen = torch.Generator().manual_seed(n % 1000 + squared)
  a, b, target = torch.randn(n, generator=gen) * 2 + 0.5, torch.randn(n, generator=gen), 0.75
  ad, bd = a.to(DEV), b.to(DEV)
  count = L.ms_reduce_partials_count(n)
  for other, od in ((b.double(), bd), (float(torch.tensor(target)), None)):
    d = a.double() - other
    ref = float((d * d).mean() if squared else d.abs().mean())
    got = []
    for poison in POISONS:
      part = guarded(4 * count, DEV, poison)
      loss = torch.full((), float('nan'), device=DEV)
      assert fn(_p(ad), _p(od), target, _p(loss), _p(part), n, _stream()) == 0
      torch.cuda.synchronize()
      assert guard_damage(part) is None, guard_damage(part)
      assert touched(part) is not None or count == 0
      got.append(loss)
    assert torch.equal(got[0], got[1]) and bool(torch.isfinite(got[0])), got
    assert abs(float(got[0]) - ref) <= 1e-6 * abs(ref), (float(got[0]), ref)


def test_cross_entropy_row_scratch_exactly_sized():
  """ms_cross_entropy_fwd at the table's bct_c25_r8192 shape with a row_scratch of one float per row (the kernels of this version
  keep their per-row terms in registers and leave it alone; whether it is written is not part of the contract): guards intact, the loss meets the derived bar of that case."""
  from test_gpu_ew_parity import FLOOR
  L = _lib()
  e = EW['ce_bct_c25_r8192']
  (Bn, T), C = e['p']['shape'], e['p']['C']
  gen = torch.Generator().manual_seed(zlib.crc32(e['id'].encode()) % 100000)
  sc = torch.randn(Bn, C, T, generator=gen) * 3 + torch.randn(1, C, 1, generator=gen) * 2
  tg = torch.randint(0, C, (Bn, T), generator=gen)
  sd, td = sc.to(DEV), tg.to(DEV)
  ref = lambda dt: float(F.cross_entropy(sc.to(dt).transpose(2, 1).reshape(-1, C), tg.reshape(-1)))
  r64, r32 = ref(torch.float64), ref(torch.float32)
  got = []
  for poison in POISONS:
    rows = guarded(4 * Bn * T, DEV, poison)
    loss = torch.full((), float('nan'), device=DEV)
    assert L.ms_cross_entropy_fwd(_p(sd), _p(td), _p(loss), _p(rows), Bn, T, C, C * T, T, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert guard_damage(rows) is None, guard_damage(rows)
    got.append(loss)
  assert torch.equal(got[0], got[1])
  assert abs(float(got[0]) - r64) / abs(r64) <= 4 * max(abs(r32 - r64) / abs(r64), FLOOR), (float(got[0]), r64, r32)


def test_segmented_adam_seg_scratch_exactly_sized():
  """ms_adam_step_segmented on the table's adam_seg_n64000_chunks case (1000 segments; never-updated and future segments) with a
  seg_scratch of exactly 2 * n_seg poisoned floats: p, m, v after three steps meet the case's derived bars."""
  from test_gpu_ew_parity import FLOOR, _adam_reference, _adam_segments, _two_metrics, f32
  from mix_stage_amd import ops
  e = EW['adam_seg_n64000_chunks']
  n = e['p']['n']
  gen = torch.Generator().manual_seed(zlib.crc32(e['id'].encode()) % 100000)
  hp = lr, b1, b2, eps = (f32(1e-3), f32(0.9), f32(0.999), f32(1e-8))
  p0 = torch.randn(n, generator=gen) * 0.1
  m0, v0 = torch.randn(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 1e-4
  seg, sfirst = _adam_segments(e['p']['seg'], n, gen)
  first = sfirst.long()[seg.long()].repeat_interleave(64)
  grads, norms, max_norms = [], [], []
  for kind in e['p']['norms']:
    g = torch.randn(n, generator=gen) * 0.02 * torch.exp(torch.randn(n, generator=gen))
    true = f32(g.double().norm().item())
    grads.append(g); norms.append(true); max_norms.append(f32(true * (0.25 if kind == 'clip' else 1.5)))
  got = []
  for poison in POISONS:
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    scratch = guarded(4 * 2 * sfirst.numel(), DEV, poison)
    for g, nrm, mx in zip(grads, norms, max_norms):
      scratch.fill_(poison)                                  # (nothing is carried from step to step either)
      ops.adam_step_segmented(p, g.to(DEV), m, v, torch.tensor([nrm], device=DEV), mx, lr, b1, b2, eps, state, seg.to(DEV), sfirst.to(DEV),
                              scratch.view(torch.float32))
    torch.cuda.synchronize()
    assert guard_damage(scratch) is None, guard_damage(scratch)
    assert touched(scratch) is not None
    got.append((p, m, v))
  _assert_same_bits([list(got[0]), list(got[1])], RUN_NAMES[1:], 'segmented Adam')
  ref = _adam_reference(torch.float64, p0, m0, v0, grads, norms, max_norms, first, hp)
  y32 = _adam_reference(torch.float32, p0, m0, v0, grads, norms, max_norms, first, hp)
  for nm, a, r, y in zip('pmv', got[0], ref, y32):
    (mx, el), (ymx, yel) = _two_metrics(a, r), _two_metrics(y, r)
    assert mx <= 4 * max(ymx, FLOOR) and el <= 4 * max(yel, FLOOR), (nm, mx, el, ymx, yel)


# ------------------------------------------------------------------------------------------------ d. refusal
REFUSED = ['unet_pre', 'ae2', 'dec1', 'h16_dec1', 'd_logits']          # clip | patch / tile 2-D | grouped | bf16 | BARE


@pytest.mark.parametrize('eid', REFUSED)
def test_workspace_one_byte_short_is_refused_untouched(eid):
  """ms_conv_block_fwd_ex / ms_conv_block_bwd_ex with workspace_bytes = claimed - 1: an error that names the workspace, outputs
  (pre-filled with NaN) still NaN, in-out statistics unchanged, workspace and guards unchanged, no launch in the timing report."""
  from mix_stage_amd import _lib as LM, ops, ops16
  L = LM.lib()
  e = BY_ID[eid]
  assert e['in_mode'] == 'plain' and not e['pair'] and e['prec'] in ('fp32', 'bf16')
  nd, g = e['nd'], e['groups']
  k, s, p = _nd_kernel(e)
  sp = e['sp']
  H, W = sp if nd == 2 else (1, sp[0])
  is16 = e['prec'] == 'bf16'
  flags = (LM.MS_BF16 | (LM.MS_DT_OUT_F32 if e['out_f32'] else 0)) if is16 else 0
  d = ops.ConvGeom(nd, g, k, s, p).desc(e['B'], e['cin'], H, W, e['cout'], MODES[e['mode']], LM.MS_IN_PLAIN, flags)
  B, cin_tot, ctot = e['B'], e['cin'] * g, e['cout'] * g
  osp = (d.OH, d.OW) if nd == 2 else (d.OW,)
  gen = torch.Generator().manual_seed(1)
  rnd = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
  nan = lambda t: torch.full_like(t, float('nan'))
  kt = tuple(k) if isinstance(k, tuple) else (k,)
  x32, w = rnd(B, cin_tot, *sp), rnd(ctot, e['cin'], *kt)
  x = ops16.to_cb8(x32, LM.MS_BF16) if is16 else x32
  act = (lambda: torch.empty((B, (ctot + 7) // 8) + osp + (8,), dtype=torch.bfloat16, device=DEV)) if is16 else \
        (lambda: torch.empty((B, ctot) + osp, device=DEV))
  bn = e['mode'] in ('BN_TRAIN', 'BN_EVAL')
  bias = rnd(ctot)
  gamma, beta, rm, rv = (rnd(ctot), rnd(ctot), rnd(ctot), rnd(ctot).abs() + 0.5) if bn else (None,) * 4
  stats0 = [t.clone() for t in (rm, rv)] if bn else []
  sync = torch.zeros(1024, dtype=torch.int32, device=DEV)

  def refused(call, nbytes, outputs, what):
    ws = guarded(nbytes, DEV, 0x55)
    ops.timing_enable(True)
    try:
      ops.timing_report()
      rc = call(ws, nbytes - 1)
      torch.cuda.synchronize()
      rows = ops.timing_report()
    finally:
      ops.timing_enable(False)
    assert rc != 0, what
    assert b'workspace' in L.ms_last_error(), L.ms_last_error()
    assert not rows, '%s launched %s' % (what, rows)
    assert guard_damage(ws) is None and touched(ws) is None, what
    for nm, t in outputs.items():
      assert bool(torch.isnan(t.float()).all()), '%s wrote %s' % (what, nm)
    assert all(torch.equal(a, b) for a, b in zip(stats0, (rm, rv))) and not bool(sync.any()), what

  # forward
  y, y_raw, save = nan(act()), nan(act()), torch.full((4 * ctot,), float('nan'), device=DEV)
  if is16 and e['out_f32']:
    y = torch.full((B, ctot) + osp, float('nan'), device=DEV)
  opt = LM.FwdOptions(None, sync.data_ptr(), sync.numel())
  n_fwd = L.ms_conv_block_fwd_workspace(ctypes.byref(d))
  assert n_fwd > 0
  refused(lambda ws, nb: L.ms_conv_block_fwd_ex(ctypes.byref(d), _p(x), None, _p(w), _p(bias), _p(gamma), _p(beta), _p(rm), _p(rv), _p(y_raw),
                                                _p(y), _p(save), _p(ws), nb, _stream(), ctypes.byref(opt)),
          n_fwd, dict(y=y, y_raw=y_raw, save=save), eid + ' forward')
  # backward (its inputs y, y_raw, save now finite)
  yb, yrb = torch.randn_like(y.float()).to(y.dtype), torch.randn_like(y_raw.float()).to(y_raw.dtype)
  saveb = torch.rand(4 * ctot, device=DEV) + 0.5
  dy = torch.randn_like(yb.float()).to(yb.dtype)
  outs = dict(dyr=nan(act()), dx=nan(x), dw=nan(w), dbias=nan(bias))
  if bn:
    outs.update(dgamma=nan(bias), dbeta=nan(bias))
  bopt = LM.BwdOptions()
  n_bwd = L.ms_conv_block_bwd_workspace(ctypes.byref(d))
  assert n_bwd > 0
  refused(lambda ws, nb: L.ms_conv_block_bwd_ex(ctypes.byref(d), _p(x), None, _p(w), _p(gamma), None, None, _p(yrb), _p(yb), _p(saveb), _p(dy),
                                                _p(outs['dyr']), _p(outs['dx']), None, _p(outs['dw']), _p(outs['dbias']), _p(outs.get('dgamma')),
                                                _p(outs.get('dbeta')), _p(ws), nb, _stream(), ctypes.byref(bopt)),
          n_bwd, outs, eid + ' backward')
