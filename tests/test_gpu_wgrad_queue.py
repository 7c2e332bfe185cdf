"""GPU: the queued weight gradients of trainer mode (ops.enable_deferred_wgrad: every block's weight gradient waits in a queue,
ONE ms_wgrad_flush at the end of the backward pass launches the queue as a few multi-job kernels, ms_wgrad_reduce_multi adds the
pixel-split slabs into the gradient slots) against fp64, case by case of tests/helpers/wgrad_queue_table.py.

A batch is N independent blocks (ConvNormRelu, or a bare conv) whose parameters live in ONE FlatAdam, each with its own input and
upstream gradient; after zero_grad() one torch.autograd.backward over all outputs queues every block into the same flush.  Every
batch case asserts
  a. labels      the multi-job launches and the slab reductions of the pass are exactly the claimed ones (jobsN and wgsN from the
                 table's mirrors), no unqueued weight-gradient launch appears, the blocks that launch at once show their own label;
  b. fp64        every block's y, dx, dw, dgamma / dbeta or dbias and running statistics meet the bars of
                 test_gpu_dispatch_parity (fp32) / test_gpu_kernels16._case (16-bit) -- helpers/wgrad_queue_checks.py;
  c. placement   bit for bit the results of the same block queued ALONE (same planner hint): its place in a job table, the sort
                 and the rollover cannot change a job's arithmetic;
  d. queueing    bit for bit the results of the unqueued launches with the planner hint pinned on (ms_set_wgrad_batched(1, 0)) and
                 deferral off -- the premise of test_prepared_dgrad_weights_and_deferred_wgrad_reductions_change_nothing.
                 16-bit: plan_wgrad16 does not read the hint; queued jobs of up to 3 slots run on the 5-slot instance, which
                 differs from the 3-slot one only in the staging DMAs a wave issues per tile (csrc/wgrad16.hip:240-247, the
                 `i * 256 + wave * 64 < xv` skip) -- the MFMA order is the same, so bit equality is held there too.
Then: a module used twice in one pass, a pre-filled gradient buffer (queued writes ADD), a queue discarded after a failed backward
pass, and ms_wgrad_reduce_multi called directly on values whose every summation order is exact."""
import contextlib
import ctypes
import zlib

import pytest
import torch

from helpers import wgrad_queue_checks as C
from helpers import wgrad_queue_table as T
from test_gpu_dispatch_parity import _deterministic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEASURED = {}                 # id -> {family: worst dw error / bar}: printed per case (the commit message quotes them)


@pytest.fixture(autouse=True)
def _stop_on_a_faulted_device():
  try:
    torch.cuda.synchronize()
  except RuntimeError as err:
    pytest.exit('the device reported a fault before this case: %s' % err, returncode=3)
  yield


@pytest.fixture(autouse=True)
def _trainer_modes_off():
  """Process-wide modes off before each case (a MixStageTrainStep of an earlier file leaves them on), what was on before on again after;
  the planner hint and the backward overlap likewise."""
  from mix_stage_amd import ops
  was = (ops._prepared['on'], ops._deferred['on'])
  hint = ops.lib().ms_set_wgrad_batched(0, 0)
  ops.enable_prepared_weights(False)
  ops.enable_deferred_wgrad(False)
  ops.set_backward_overlap(None)
  yield
  ops.set_backward_overlap(None)
  ops.reset_deferred_wgrad()
  ops.enable_prepared_weights(was[0])
  ops.enable_deferred_wgrad(was[1])
  if not was[1]:
    ops.lib().ms_set_wgrad_batched(hint, 0)


def _queued(on):
  """Trainer mode as MixStageTrainStep switches it on; off = the unqueued launches under the SAME planner hint."""
  from mix_stage_amd import ops
  ops.enable_prepared_weights(on)
  ops.enable_deferred_wgrad(on)
  ops.lib().ms_set_wgrad_batched(1, 0)


@contextlib.contextmanager
def _timed(labels):
  from mix_stage_amd import ops
  ops.timing_enable(True)
  try:
    yield
    torch.cuda.synchronize()
    for r in ops.timing_report():
      labels[r['label']] = labels.get(r['label'], 0) + r['count']
  finally:
    ops.timing_enable(False)


def _ref_device(b):
  """As test_gpu_dispatch_parity: float64 on the CPU, on the device for 2-D blocks and above ~0.5 GMAC."""
  g = T.geometry(b)
  macs = b['B'] * b['groups'] * b['cout'] * b['cin'] * g['KH'] * g['KW'] * g['OH'] * g['OW']
  return DEV if (b['nd'] == 2 or macs > 5e8) else 'cpu'


class Batch:
  def __init__(self, blocks, name, uses=1):
    import mix_stage_amd as A
    from mix_stage_amd.train_step import FlatAdam
    self.blocks, self.uses = blocks, uses
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)
    self.mods, self.xs, self.gys = [], [], []
    for i, b in enumerate(blocks):
      g, geo = b['groups'], T.geometry(b)
      k, s, p = C._nd_kernel(b)
      if b['mode'] == 'BN_TRAIN':
        mod = _deterministic(A.ConvNormRelu(b['cin'], b['cout'], type='%dd' % b['nd'], leaky=True, kernel_size=k, stride=s, padding=p, groups=g),
                             'blk%d.' % i).to(DEV)
        mod.train()
      else:
        assert b['mode'] == 'BARE' and b['in_mode'] == 'plain'
        cls = torch.nn.Conv1d if b['nd'] == 1 else torch.nn.Conv2d
        mod = _deterministic(cls(b['cin'] * g, b['cout'] * g, k, s, padding=p, groups=g), 'c%d.' % i).to(DEV)
      if b['prec'] != 'fp32':
        A.set_compute_dtype(mod, b['prec'])
      self.mods.append(mod)
      cin_tot = b['cin'] * (1 if b['in_mode'] == 'bcast' else g)
      osp = (geo['OH'], geo['OW']) if b['nd'] == 2 else (geo['OW'],)
      xs, gys = [], []
      for u in range(uses):
        scale, shift = (1.0, 0.0) if u == 0 else (1.6, 0.3)                       # the two uses differ in their statistics
        if b['in_mode'] == 'up2':
          x = [torch.randn(b['B'], cin_tot, b['sp'][0] // 2, generator=gen), torch.randn(b['B'], cin_tot, *b['sp'], generator=gen)]
        else:
          x = [torch.randn(b['B'], cin_tot, *b['sp'], generator=gen)]
        xs.append([(t * scale + shift).to(DEV) for t in x])
        gys.append(torch.randn(b['B'], b['cout'] * g, *osp, generator=gen).to(DEV))
      self.xs.append(xs)
      self.gys.append(gys)
    self.opt = FlatAdam([q for m in self.mods for q in m.parameters()])
    self.stats0 = [(m.norm.running_mean.clone(), m.norm.running_var.clone()) if hasattr(m, 'norm') else None for m in self.mods]

  def params(self, i):
    m = self.mods[i]
    if hasattr(m, 'norm'):
      return dict(w=m.conv.weight, bias=m.conv.bias, gamma=m.norm.weight, beta=m.norm.bias)
    return dict(w=m.weight, bias=m.bias, gamma=None, beta=None)

  def forward(self, i, xin):
    from mix_stage_amd.layers import bare_conv
    b, m = self.blocks[i], self.mods[i]
    if b['mode'] == 'BARE':
      return bare_conv(m, xin[0], out_f32=b['out_f32'])
    if b['in_mode'] == 'up2':
      return m.forward_upsample_add(xin[0], xin[1])
    if b['in_mode'] == 'bcast':
      return m.forward_broadcast(xin[0])
    return m(xin[0])

  def run(self, only=None, prefill=None):
    """Forward of every block (and use), ONE backward pass -> [per block: dict(y=[..], dx0=[..], dx1=[..], dw, dbias, dgamma, dbeta, rm, rv)]
    (None for the blocks left out by `only`)."""
    idx = list(range(len(self.blocks))) if only is None else list(only)
    with torch.no_grad():
      for m, st in zip(self.mods, self.stats0):
        if st is not None:
          m.norm.running_mean.copy_(st[0]); m.norm.running_var.copy_(st[1])
    self.opt.zero_grad()
    if prefill is not None:
      self.opt.flat_g.copy_(prefill)                      # (the slots stay fresh)
    leaves, ys, gys = {}, [], []
    for i in idx:
      for u in range(self.uses):
        xin = [t.clone().requires_grad_() for t in self.xs[i][u]]
        leaves[i, u] = xin
        ys.append(self.forward(i, xin))
        gys.append(self.gys[i][u])
    torch.autograd.backward(ys, gys)
    torch.cuda.synchronize()
    out = [None] * len(self.blocks)
    for n, i in enumerate(idx):
      slot = lambda q: None if q is None else q._ms_grad_slot.clone()
      pr = self.params(i)
      st = self.stats0[i]
      out[i] = dict(y=[ys[n * self.uses + u].detach().clone() for u in range(self.uses)],
                    dx0=[leaves[i, u][0].grad.clone() for u in range(self.uses)],
                    dx1=[leaves[i, u][1].grad.clone() if len(leaves[i, u]) > 1 else None for u in range(self.uses)],
                    dw=slot(pr['w']), dbias=slot(pr['bias']), dgamma=slot(pr['gamma']), dbeta=slot(pr['beta']),
                    rm=self.mods[i].norm.running_mean.clone() if st is not None else None,
                    rv=self.mods[i].norm.running_var.clone() if st is not None else None)
    return out

  def reference(self, i, got):
    b = self.blocks[i]
    uses = [dict(xs=self.xs[i][u], gy=self.gys[i][u], y=got['y'][u]) for u in range(self.uses)]
    st = self.stats0[i] or (None, None)
    return C.reference(b, self.params(i), uses, st[0], st[1], dev=_ref_device(b))


def _fp64_bars(e, bt, got):
  """b. of the module docstring for every block of the batch; records the worst dw error per family."""
  worst = MEASURED.setdefault(e['id'], {})
  for i, (b, c) in enumerate(zip(e['blocks'], e['claims']['blocks'])):
    errs = C.bars(b, got[i], bt.reference(i, got[i]))
    bad = C.failed(errs)
    assert not bad, '%s block %d (%s): errors (value, bar): %s | all: %s' % (e['id'], i, c, bad, {k: '%.2e' % v[0] for k, v in errs.items()})
    fam = c['family'] + ('' if c['splits'] > 1 else ' splits1')
    worst[fam] = max(worst.get(fam, (0.0, 0.0)), (errs['dw'][0], errs['dw'][1]))
  print('WGRAD-QUEUE %s worst dw error / bar per family: %s' % (e['id'], {k: '%.2e / %.0e' % v for k, v in sorted(worst.items())}))


BATCH = [e for e in T.TABLE if not e['twice'] and e['id'] != 'prefilled_slot']


@pytest.mark.parametrize('e', BATCH, ids=[e['id'] for e in BATCH])
def test_queued_batch_matches_fp64_and_the_unqueued_bits(e):
  bt = Batch(e['blocks'], e['id'])
  _queued(True)
  labels = {}
  with _timed(labels):
    got = bt.run()
  print('WGRAD-QUEUE %s launches: %s' % (e['id'], sorted(l for l in labels if 'wgrad' in l)))
  C.check_labels(e, labels)                                                               # a.
  _fp64_bars(e, bt, got)                                                                  # b.
  for i in range(len(e['blocks'])):                                                       # c.
    alone = bt.run(only=[i])[i]
    diff = C.differing(got[i], alone)
    assert not diff, '%s block %d (%s): queued with the batch and queued alone differ in %s' % (e['id'], i, e['claims']['blocks'][i], diff)
  _queued(False)                                                                          # d.
  labels_u = {}
  with _timed(labels_u):
    plain = bt.run()
  assert not any(' multi k' in l or ' multi shape' in l or ' multi taps' in l or l.startswith('wgrad_reduce_multi') for l in labels_u), sorted(labels_u)
  for i in range(len(e['blocks'])):
    diff = C.differing(got[i], plain[i])
    assert not diff, '%s block %d (%s): queued and unqueued launches differ in %s' % (e['id'], i, e['claims']['blocks'][i], diff)


TWICE = [e for e in T.TABLE if e['twice']]


@pytest.mark.parametrize('e', TWICE, ids=[e['id'] for e in TWICE])
def test_module_used_twice_in_one_backward_pass(e):
  """The second use of a parameter in a step goes to a temporary (ops.LATE) that a later round of ms_wgrad_reduce_multi adds into the
  slot: dw, dgamma, dbeta (and the ~0 conv bias gradient) are the fp64 sum of both uses at the bars, and bit for bit the unqueued
  result (first gradient written into the slot, second added by autograd) under the pinned hint."""
  bt = Batch(e['blocks'], e['id'], uses=2)
  _queued(True)
  labels = {}
  with _timed(labels):
    got = bt.run()
  print('WGRAD-QUEUE %s launches: %s' % (e['id'], sorted(l for l in labels if 'wgrad' in l)))
  C.check_labels(e, labels)
  _fp64_bars(e, bt, got)
  _queued(False)
  plain = bt.run()
  for i in range(len(e['blocks'])):
    diff = C.differing(got[i], plain[i])
    assert not diff, '%s block %d: queued and unqueued two-pass results differ in %s' % (e['id'], i, diff)


def test_prefilled_slot_queued_writes_add():
  """The gradient buffer pre-filled with a dyadic pattern after zero_grad (slots fresh): every block's dw slot must be pattern + the
  gradient of the zeroed run, computed in torch fp32, bit for bit -- jobs that write dw themselves (accumulate = 1), jobs whose
  slabs ms_wgrad_reduce_multi adds, and the blocks that launch at once and leave slabs."""
  e = T.BY_ID['prefilled_slot']
  bt = Batch(e['blocks'], e['id'])
  _queued(True)
  zeroed = bt.run()
  pattern = torch.where(torch.arange(bt.opt.total, device=DEV) % 2 == 0, 0.5, -0.25).float()
  labels = {}
  with _timed(labels):
    filled = bt.run(prefill=pattern)
  C.check_labels(e, labels)
  for i, (q, c) in enumerate(zip(bt.mods, e['claims']['blocks'])):
    w = bt.params(i)['w']
    at = bt.opt.offsets[[id(p) for p in bt.opt.params].index(id(w))]
    want = pattern[at:at + w.numel()].view_as(w) + zeroed[i]['dw']
    assert bool((zeroed[i]['dw'] != 0).any())
    assert C.same_bits(filled[i]['dw'], want), 'block %d (%s): the slot is not pattern + dw (max diff %.3e)' % (
        i, c, (filled[i]['dw'] - want).abs().max().item())
    assert not C.differing(zeroed[i], filled[i], keys=('y', 'dx0', 'dx1')), i


class _Raise(torch.autograd.Function):
  @staticmethod
  def forward(ctx, x):
    return x.clone()

  @staticmethod
  def backward(ctx, g):
    raise ValueError('backward pass interrupted on purpose (a Python exception: nothing runs on the device)')


def test_discarded_queue_leaves_nothing_behind():
  """A backward pass that queues a job and then raises: ops.reset_deferred_wgrad() drops the job (ms_wgrad_discard); the next
  pass launches only its own jobs and meets every check, and the dropped job's dw slot is never written."""
  from mix_stage_amd import ops
  chain = Batch([T.Bk(1, 8, 96, 136, 1, 3, 1, 1, (32,)), T.Bk(1, 8, 136, 96, 1, 3, 1, 1, (32,))], 'discarded_chain')
  assert T.plan(chain.blocks[1])['family'] == 'wave' and T.plan(chain.blocks[1])['queued']
  e = T.BY_ID['mixed_families']
  fresh = Batch(e['blocks'], 'discarded_fresh')
  _queued(True)
  chain.opt.zero_grad()
  x = chain.xs[0][0][0].clone().requires_grad_()
  y = chain.forward(1, [_Raise.apply(chain.forward(0, [x]))])
  with pytest.raises(ValueError, match='interrupted on purpose'):
    y.backward(chain.gys[1][0])
  torch.cuda.synchronize()
  assert ops._deferred['launches'] == 1 and ops._deferred['queued'], 'block B did not queue its weight gradient before the exception'
  ops.reset_deferred_wgrad()
  assert not ops._deferred['jobs'] and not ops._deferred['keep'] and not ops._deferred['queued']
  labels = {}
  with _timed(labels):
    got = fresh.run()
  C.check_labels(e, labels)
  _fp64_bars(dict(e, id='discarded_queue'), fresh, got)
  w_b = chain.params(1)['w']
  assert not bool(w_b._ms_grad_slot.any()), 'the discarded job ran: block B\'s dw slot was written'
  assert bool(chain.params(1)['gamma']._ms_grad_slot.any()), 'block B\'s backward pass did not run before the exception'
  for i in range(len(e['blocks'])):
    diff = C.differing(got[i], fresh.run(only=[i])[i])
    assert not diff, (i, diff)
  _queued(False)
  plain = fresh.run()
  for i in range(len(e['blocks'])):
    diff = C.differing(got[i], plain[i])
    assert not diff, (i, diff)


# ------------------------------------------------------------------------------------------------ ms_wgrad_reduce_multi, directly
def _arr(ctype, vals):
  return (ctype * max(1, len(vals)))(*vals)


def _reduce_multi(parts, outs, elems, splits):
  from mix_stage_amd import ops
  n = len(outs)
  return ops.lib().ms_wgrad_reduce_multi(n, _arr(ctypes.c_void_p, [t.data_ptr() if t is not None else None for t in parts]),
                                         _arr(ctypes.c_void_p, [t.data_ptr() if t is not None else None for t in outs]),
                                         _arr(ctypes.c_int, elems), _arr(ctypes.c_int, splits),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _dyadic(gen, *shape):
  """Integers in [-1024, 1024] times 2^-6: sums of up to 65 + 1 of them stay below 2^17 * 2^-6 with 6 fraction bits -- 23 bits, so
  every order of summation is exact in fp32."""
  return torch.randint(-1024, 1025, shape, generator=gen).float() / 64


@pytest.mark.parametrize('name,jobs', T.REDUCE_CASES, ids=[c[0] for c in T.REDUCE_CASES])
def test_reduce_multi_is_exact_on_dyadic_values(name, jobs):
  """out[j] += sum over its slabs, for every form of reduce_splits_multi_kernel (wave, 16-byte, scalar; the grid-stride loop; an
  `out` off 16-byte alignment; 97 jobs = two launches; no job): equal to the float64 sum bit for bit, guard words around every
  `out` untouched."""
  gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)
  parts, outs, bufs, refs = [], [], [], []
  for n, s, off in jobs:
    part, out0 = _dyadic(gen, s, n), _dyadic(gen, n)
    buf = torch.full((off + n + 4,), 7.0)
    buf[off:off + n] = out0
    buf = buf.to(DEV)
    bufs.append(buf)
    outs.append(buf[off:off + n])
    parts.append(part.to(DEV))
    refs.append((out0.double() + part.double().sum(0)).float())
    assert bool((refs[-1].double() == out0.double() + part.double().sum(0)).all())
  labels = {}
  with _timed(labels):
    rc = _reduce_multi(parts, outs, [j[0] for j in jobs], [j[1] for j in jobs])
  assert rc == 0
  want = {'wgrad_reduce_multi jobs%d' % k: 1 for k in T.reduce_launches(len(jobs))}
  assert labels == want, (labels, want)
  for (n, s, off), buf, ref in zip(jobs, bufs, refs):
    got = buf.cpu()
    assert torch.equal(got[off:off + n], ref), (name, n, s, off, (got[off:off + n] - ref).abs().max().item())
    assert bool((got[:off] == 7.0).all()) and bool((got[off + n:] == 7.0).all()), 'words around `out` were written'


def test_reduce_multi_refuses_bad_jobs_untouched():
  from mix_stage_amd import ops
  gen = torch.Generator().manual_seed(3)
  part, out = _dyadic(gen, 4, 100).to(DEV), _dyadic(gen, 100).to(DEV)
  out0 = out.clone()
  L = ops.lib()
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  one = lambda v, t=ctypes.c_int: (t * 1)(v)
  pp, po = one(part.data_ptr(), ctypes.c_void_p), one(out.data_ptr(), ctypes.c_void_p)
  calls = {
      'null partials array': lambda: L.ms_wgrad_reduce_multi(1, None, po, one(100), one(4), stream),
      'null dw array': lambda: L.ms_wgrad_reduce_multi(1, pp, None, one(100), one(4), stream),
      'null elems array': lambda: L.ms_wgrad_reduce_multi(1, pp, po, None, one(4), stream),
      'null splits array': lambda: L.ms_wgrad_reduce_multi(1, pp, po, one(100), None, stream),
      'null partials': lambda: L.ms_wgrad_reduce_multi(1, one(None, ctypes.c_void_p), po, one(100), one(4), stream),
      'null dw': lambda: L.ms_wgrad_reduce_multi(1, pp, one(None, ctypes.c_void_p), one(100), one(4), stream),
      'elems 0': lambda: L.ms_wgrad_reduce_multi(1, pp, po, one(0), one(4), stream),
      'elems -1': lambda: L.ms_wgrad_reduce_multi(1, pp, po, one(-1), one(4), stream),
      'splits 0': lambda: L.ms_wgrad_reduce_multi(1, pp, po, one(100), one(0), stream),
      'n -1': lambda: L.ms_wgrad_reduce_multi(-1, pp, po, one(100), one(4), stream),
  }
  for what, call in calls.items():
    labels = {}
    with _timed(labels):
      rc = call()
    assert rc != 0, what
    assert b'ms_wgrad_reduce_multi' in L.ms_last_error(), (what, L.ms_last_error())
    assert not labels, (what, labels)
    assert torch.equal(out, out0), what


def test_reduce_multi_checks_every_job_before_the_first_launch():
  """97 jobs of which the last is bad: the first 96 fill a launch of their own, which must not have run when the call is refused."""
  from mix_stage_amd import ops
  gen = torch.Generator().manual_seed(4)
  parts = [_dyadic(gen, 2, 16).to(DEV) for _ in range(97)]
  outs = [_dyadic(gen, 16).to(DEV) for _ in range(97)]
  before = [o.clone() for o in outs]
  for what, elems, splits in (('elems 0', [16] * 96 + [0], [2] * 97), ('splits 0', [16] * 97, [2] * 96 + [0])):
    labels = {}
    with _timed(labels):
      rc = _reduce_multi(parts, outs, elems, splits)
    assert rc != 0 and b'bad job 96' in ops.lib().ms_last_error(), (what, ops.lib().ms_last_error())
    assert not labels, (what, labels)
    assert all(torch.equal(a, b) for a, b in zip(outs, before)), '%s: jobs ahead of the bad one were reduced' % what
