"""GPU: the workspace contract of include/mixstage.h for the frozen-BatchNorm forms (MS_BN_EVAL with MS_DT_BN_FROZEN, and its backward):
forward and backward on exactly-sized, poisoned scratch between guard regions (tests/helpers/guarded_scratch.py) -- nothing outside
the claimed bytes is touched and the results do not depend on what the scratch held -- and a workspace one byte short is an error
before anything is written.  One fp32 1-D block (the clip-resident conv, one-launch backward), two fp32 2-D blocks (the two-pass
backward with its partials in the scratch, 16-byte and scalar rows) and one bf16 block."""
import ctypes

import pytest
import torch

from helpers.guarded_scratch import POISONS, exact_scratch, guarded, guard_damage, touched
from test_gpu_frozen_bn import CASES, DEV, _inputs, _mk, _run_hip

pytestmark = pytest.mark.gpu

PICK = ('f4_1_clip', 'r4a4_2d_s2', 'ra_2d_s2')


@pytest.mark.parametrize('case', [c for c in CASES if c[0] in PICK], ids=lambda c: c[0])
def test_frozen_block_on_exact_poisoned_scratch(case, monkeypatch):
  from mix_stage_amd import layers
  xs = _inputs(case, torch.Generator().manual_seed(3), case[8])
  results = []
  for poison in POISONS:
    blk = _mk(case, 3)
    layers.freeze_batchnorm(blk)
    with exact_scratch(monkeypatch, poison) as rec:
      y, leaves = _run_hip(blk, case, xs)
      gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
      y.backward(gy.to(DEV))
      torch.cuda.synchronize()
    assert len([o for o, _ in rec.views if o == 'workspace']) == 2          # one forward, one backward call
    out = [y.detach(), leaves[0].grad, blk.conv.weight.grad, blk.conv.bias.grad, blk.norm.weight.grad, blk.norm.bias.grad]
    assert all(torch.isfinite(t).all() for t in out)
    results.append(out)
  for a, b in zip(*results):
    assert torch.equal(a, b)


def test_frozen_bf16_block_on_exact_poisoned_scratch(monkeypatch):
  from mix_stage_amd import layers
  case = [c for c in CASES if c[0] == 'f4_1_clip'][0]
  xs = _inputs(case, torch.Generator().manual_seed(3), 4)
  results = []
  for poison in POISONS:
    blk = _mk(case, 3)
    layers.freeze_batchnorm(blk)
    layers.set_compute_dtype(blk, 'bf16')
    with exact_scratch(monkeypatch, poison) as rec:
      y, leaves = _run_hip(blk, case, xs)
      gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
      y.backward(gy.to(DEV))
      torch.cuda.synchronize()
    assert len([o for o, _ in rec.views if o == 'workspace']) == 2
    out = [y.detach(), leaves[0].grad, blk.conv.weight.grad, blk.conv.bias.grad, blk.norm.weight.grad, blk.norm.bias.grad]
    assert all(torch.isfinite(t).all() for t in out)
    results.append(out)
  for a, b in zip(*results):
    assert torch.equal(a, b)


@pytest.mark.parametrize('geo', [(2, 256, 1, 64, 256, 1, 1, 3, 1, 1, 0, 1, 1, 64), (5, 64, 62, 62, 64, 1, 4, 4, 2, 2, 1, 1, 31, 31)],
                         ids=['1d', '2d'])
def test_a_workspace_one_byte_short_is_refused_before_anything_is_written(geo):
  from mix_stage_amd import _lib
  L = _lib.lib()
  Bn, cin, H, W, cout = geo[:5]
  KH, KW, OH, OW = geo[6], geo[7], geo[12], geo[13]
  d = _lib.ConvDesc(*geo, _lib.MS_BN_EVAL, _lib.MS_IN_PLAIN, 0.2, 1e-5, 0.1, _lib.MS_DT_BN_FROZEN)
  t = lambda *s: torch.randn(*s, device=DEV)
  x = t(Bn, cin, H, W)
  w, v = t(cout, cin, KH, KW), t(cout).abs() + 0.5
  p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  n_out = Bn * cout * OH * OW
  outs = {k: guarded(4 * n, DEV, 0x55).view(torch.float32) for k, n in
          (('y', n_out), ('y_raw', n_out), ('save', 4 * cout), ('dyr', n_out), ('dx', x.numel()), ('dw', w.numel()), ('dv', cout))}
  before = {k: o.clone() for k, o in outs.items()}
  rm, rv = v.clone(), v.clone()
  for which, need in (('fwd', L.ms_conv_block_fwd_workspace(ctypes.byref(d))), ('bwd', L.ms_conv_block_bwd_workspace(ctypes.byref(d)))):
    ws = guarded(need, DEV, 0xFF)
    if which == 'fwd':
      rc = L.ms_conv_block_fwd(ctypes.byref(d), p(x), None, p(w), p(v), p(v), p(v), p(rm), p(rv), p(outs['y_raw']), p(outs['y']),
                               p(outs['save']), p(ws), need - 1, s)
    else:
      rc = L.ms_conv_block_bwd(ctypes.byref(d), p(x), None, p(w), p(v), None, None, p(outs['y_raw']), None, p(outs['save']), p(x.new_ones(n_out)),
                               p(outs['dyr']), p(outs['dx']), None, p(outs['dw']), p(outs['dv']), None, None, p(ws), need - 1, s)
    torch.cuda.synchronize()
    assert rc != 0 and 'workspace too small' in L.ms_last_error().decode(), which
    assert touched(ws) is None and guard_damage(ws) is None
    assert all(torch.equal(outs[k], before[k]) for k in outs), which
  assert torch.equal(rm, v) and torch.equal(rv, v)
