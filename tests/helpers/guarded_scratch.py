"""Exactly-sized, poisoned scratch between guards, for the tests of the C-ABI's scratch contract.

The library allocates nothing: the caller asks a size function (ms_*_workspace, ms_wgrad_partials_elems, ms_dgrad_weights_elems,
ms_weights16_bytes, ...) and hands over that many bytes, whose contents on entry are unspecified.  `guarded` builds such a buffer
for a test: a uint8 view of exactly `nbytes` bytes on a 256-byte boundary, inside ONE larger allocation that keeps at least
GUARD bytes of a fixed pattern on each side, its interior filled with a poison byte.  A launch that strays past the claimed size
lands in the guard -- memory this test owns -- and `check` reports it; a launch that reads scratch it did not write computes with
the poison (0xFF: NaN as fp32 / bf16 / fp16, -1 as a counter; 0x55: finite and absurd) and its results differ between the two.

`exact_scratch(monkeypatch, poison)` puts every scratch owner of mix_stage_amd.ops / ops16 on such buffers for the duration of a
case and checks all guards on exit."""
import contextlib

import torch

GUARD = 1 << 20                 # bytes of pattern on each side of the exact region (at least)
ALIGN = 256                     # the exact region starts on this boundary, as torch's own allocations do
POISONS = (0xFF, 0x55)

_patterns = {}


def _pattern(device):
  """GUARD + ALIGN bytes that repeat with period 251 (a prime: no power-of-two stride sees a constant)."""
  key = str(device)
  p = _patterns.get(key)
  if p is None:
    p = _patterns[key] = ((torch.arange(GUARD + ALIGN, device=device) * 7 + 13) % 251).to(torch.uint8)
  return p


def _sync(device):
  if device.type == 'cuda':
    torch.cuda.synchronize(device)


def guarded(nbytes, device, poison):
  """uint8 view of exactly `nbytes` bytes (0 is allowed) between two guards; `view._guard` carries what `check` needs."""
  nbytes = int(nbytes)
  device = torch.device(device)
  whole = torch.empty(GUARD + ALIGN + nbytes + GUARD, dtype=torch.uint8, device=device)
  start = GUARD + (-(whole.data_ptr() + GUARD)) % ALIGN
  pat = _pattern(device)
  whole[:start].copy_(pat[:start])
  tail = whole.numel() - start - nbytes
  whole[start + nbytes:].copy_(pat[:tail])
  view = whole[start:start + nbytes]
  view.fill_(poison)
  assert (whole.data_ptr() + start) % ALIGN == 0 and start >= GUARD and tail >= GUARD
  assert nbytes == 0 or view.data_ptr() == whole.data_ptr() + start      # (an empty view has no address worth checking)
  view._guard = dict(whole=whole, start=start, nbytes=nbytes, poison=poison)
  return view


def guarded_like(t, poison):
  """A guarded, poisoned tensor of t's element count and dtype (1-D)."""
  g = guarded(t.numel() * t.element_size(), t.device, poison)
  out = g.view(t.dtype)
  out._guard = g._guard
  return out


def is_guarded(t):
  return getattr(t, '_guard', None) is not None


def _first_last(mask):
  """(lowest, highest) index at which the 1-D bool `mask` is set, or None."""
  if mask.numel() == 0 or not bool(mask.any()):
    return None
  m = mask.to(torch.uint8)
  return int(m.argmax()), mask.numel() - 1 - int(m.flip(0).argmax())


def guard_damage(view):
  """None when both guards are untouched, else a text that names the changed range relative to the region's ends."""
  g = view._guard
  whole, start, n = g['whole'], g['start'], g['nbytes']
  pat = _pattern(whole.device)
  _sync(whole.device)
  msgs = []
  hi = _first_last(whole[start + n:] != pat[:whole.numel() - start - n])
  if hi is not None:
    msgs.append('bytes +%d .. +%d past the end of the %d claimed bytes changed' % (hi[0], hi[1], n))
  lo = _first_last(whole[:start] != pat[:start])
  if lo is not None:
    msgs.append('bytes -%d .. -%d in front of the region changed (%d .. %d before its end)'
                % (start - lo[0], start - lo[1], start - lo[0] + n, start - lo[1] + n))
  return '; '.join(msgs) or None


def check(view):
  bad = guard_damage(view)
  assert bad is None, 'scratch overrun: ' + bad


def touched(view):
  """(lowest, highest) byte offset of the exact region that no longer holds the poison, or None when nothing changed.
  (A byte a kernel wrote that happens to equal the poison counts as unchanged: the high-water mark is a lower bound.)"""
  g = view._guard
  _sync(g['whole'].device)
  interior = g['whole'][g['start']:g['start'] + g['nbytes']]
  return _first_last(interior != g['poison'])


class Scratch:
  """What exact_scratch handed out: `views` in call order as (owner, view), owner = 'workspace' | 'side_workspace' |
  'wgrad_partials' | 'prepared' | 'prepared16' | 'chain_prepared'."""

  def __init__(self, poison):
    self.poison, self.views = poison, []

  def new(self, owner, nbytes, device):
    v = guarded(nbytes, device, self.poison)
    self.views.append((owner, v))
    return v

  def new_like(self, owner, t):
    v = guarded_like(t, self.poison)
    self.views.append((owner, v))
    return v

  def check(self):
    bad = [(owner, v._guard['nbytes'], guard_damage(v)) for owner, v in self.views]
    bad = [b for b in bad if b[2]]
    assert not bad, 'scratch overrun (owner, claimed bytes, damage): %s' % bad

  def highwater(self, owner='workspace'):
    """[(claimed bytes, (highest changed offset + 1) / claimed bytes, or 0.0 when nothing changed)] per view of `owner`."""
    rows = []
    for o, v in self.views:
      if o == owner and v._guard['nbytes']:
        t = touched(v)
        rows.append((v._guard['nbytes'], 0.0 if t is None else (t[1] + 1) / v._guard['nbytes']))
    return rows


@contextlib.contextmanager
def exact_scratch(monkeypatch, poison):
  """Every scratch buffer that mix_stage_amd.ops / ops16 hand to the library is exactly as large as the size function says, fresh,
  poisoned and guarded while the block runs:
    ops.workspace, ops.side_workspace, ops16.workspace   a new view per call (kept alive: deferred launches and held blocks point
                                                         into them after the call returns)
    ops._wgrad_partials_for, ops._prepared_for, ops16._prepared16_for, ops._chain_prepared
                                                         the cached torch.empty buffer is replaced by a guarded one of the same
                                                         element count before the first launch that writes it
  Yields the Scratch record; on exit the caches are emptied of the guarded buffers and every guard is checked.  The meeting
  counters (block_sync, chain_sync) are zero-initialised state, not scratch, and stay as they are."""
  from mix_stage_amd import ops, ops16
  rec = Scratch(poison)
  real_prepare, real_prepare16 = ops._prepare_entries, ops16._prepare16
  orig_partials, orig_prepared, orig_prepared16, orig_chain = ops._wgrad_partials_for, ops._prepared_for, ops16._prepared16_for, ops._chain_prepared

  def workspace(nbytes, device):
    if ops.USE_IN_LAUNCH_SPLIT_REDUCTION:
      ops._ensure_counters(device)         # (as the real ops.workspace does: zeroed state, not scratch)
    return rec.new('workspace', nbytes, device)

  def side_workspace(nbytes, device):
    return rec.new('side_workspace', nbytes, device)

  def wgrad_partials_for(w, d):
    buf, nsplit = orig_partials(w, d)
    if buf is None or is_guarded(buf):
      return buf, nsplit
    key = (w.data_ptr(), id(d))
    old = ops._deferred['bufs'][key]
    g = rec.new_like('wgrad_partials', buf)
    ops._deferred['bufs'][key] = (g,) + tuple(old[1:])
    assert orig_partials(w, d)[0] is g                    # (the cache now hands out the guarded buffer)
    return g, nsplit

  def _held(module, name, real, call):
    """Run `call` with the prepare launch held back -> (its result, the entries it wanted to build)."""
    pending = []
    setattr(module, name, pending.extend)
    try:
      wt = call()
    finally:
      setattr(module, name, real)
    return wt, pending

  def _swap_and_build(owner, entries, real):
    for e in entries:
      if e.get('wt') is not None and not is_guarded(e['wt']):
        old = e['wt']
        e['wt'] = rec.new_like(owner, old)
        for k, v in list(ops._chain_scratch.items()):
          if v is old:
            ops._chain_scratch[k] = e['wt']
    if entries:
      real(entries)

  def prepared_for(w, d, kind='dgrad'):
    wt, pending = _held(ops, '_prepare_entries', real_prepare, lambda: orig_prepared(w, d, kind))
    if wt is None:
      return None
    e = ops._prepared['entries'][(w.data_ptr(), id(d), kind)]
    if not is_guarded(e['wt']) and not any(q is e for q in pending):
      pending.append(e)                  # (built before this case began, into a plain buffer: build it again into a guarded one)
    _swap_and_build('prepared', pending, real_prepare)
    assert is_guarded(e['wt']) and ops._prepared['entries'][(w.data_ptr(), id(d), kind)] is e    # what the launch is handed
    return e['wt']

  def prepared16_for(w, d, kind, bn=None):
    wt, pending = _held(ops16, '_prepare16', real_prepare16, lambda: orig_prepared16(w, d, kind, bn))
    if wt is None:
      return None
    e = ops._prepared['entries'][(w.data_ptr(), id(d), kind)]
    if not is_guarded(e['wt']) and not any(q is e for q in pending):
      pending.append(e)
    _swap_and_build('prepared16', pending, real_prepare16)
    assert is_guarded(e['wt']) and ops._prepared['entries'][(w.data_ptr(), id(d), kind)] is e
    return e['wt']

  def chain_prepared(d, ws):
    wt, pending = _held(ops, '_prepare_entries', real_prepare, lambda: orig_chain(d, ws))
    if not is_guarded(wt) and not any(e.get('wt') is wt for e in pending):
      key = (ws[0].data_ptr(), d.M, d.cin0, d.P, d.dtype, 'chain32')
      pending.append(ops._prepared['entries'][key])      # (trainer mode, built earlier into a plain buffer)
    _swap_and_build('chain_prepared', pending, real_prepare)
    out = pending[-1]['wt'] if pending else wt
    assert is_guarded(out)                                # what the launch is handed
    return out

  with monkeypatch.context() as mp:
    mp.setattr(ops, 'workspace', workspace)
    mp.setattr(ops, 'side_workspace', side_workspace)
    mp.setattr(ops16, 'workspace', workspace)
    mp.setattr(ops, '_wgrad_partials_for', wgrad_partials_for)
    mp.setattr(ops, '_prepared_for', prepared_for)
    mp.setattr(ops16, '_prepared16_for', prepared16_for)
    mp.setattr(ops, '_chain_prepared', chain_prepared)
    try:
      yield rec
    finally:
      torch.cuda.synchronize()
      # nothing of this case stays in the caches: later users build plain buffers again
      ops._deferred['bufs'] = {k: v for k, v in ops._deferred['bufs'].items() if not is_guarded(v[0])}
      for key, e in list(ops._prepared['entries'].items()):
        if e.get('wt') is not None and is_guarded(e['wt']):
          del ops._prepared['entries'][key]
          for sp, lst in ops._prepared['by_storage'].items():
            ops._prepared['by_storage'][sp] = [q for q in lst if q is not e]
      for k, v in list(ops._chain_scratch.items()):
        if is_guarded(v):
          del ops._chain_scratch[k]
  rec.check()
