"""GPU: the workspace contract of include/mixstage.h for the dropout forms (ms_dropout_bn_fwd / ms_dropout_bn_bwd with
ms_dropout_bn_workspace): the block's forward and backward on exactly-sized, poisoned scratch between guard regions
(tests/helpers/guarded_scratch.py) -- nothing outside the claimed bytes is touched and the results do not depend on what the scratch
held -- and a workspace one byte short is an error before anything is written.  The one-launch forms claim no scratch at all; the
two-pass forms (more than 4096 values per channel) keep their chunk partials there: element dropout (1-D), channel dropout (2-D),
frozen statistics, and one bf16 block."""
import ctypes

import pytest
import torch

from helpers.guarded_scratch import POISONS, exact_scratch, guarded, guard_damage, touched
from test_gpu_dropout import CASES, DEV, SEED, _inputs, _mk, _run_hip

pytestmark = pytest.mark.gpu

PICK = ('n1024', 'n4098', '2d_4x4s2')


def _both_poisons(case, monkeypatch, frozen, dtype=None):
  import mix_stage_amd as A
  from mix_stage_amd import _lib, layers
  xs = _inputs(case, torch.Generator().manual_seed(3), case[8])
  results, sizes = [], None
  for poison in POISONS:
    A.manual_dropout_seed(SEED)
    blk = _mk(case, 3)
    if frozen:
      layers.freeze_batchnorm(blk)
    if dtype:
      layers.set_compute_dtype(blk, dtype)
    with exact_scratch(monkeypatch, poison) as rec:
      y, leaves = _run_hip(blk, case, xs)
      gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(4))
      y.backward(gy.to(DEV))
      torch.cuda.synchronize()
    sizes = [v._guard['nbytes'] for o, v in rec.views if o == 'workspace']
    out = [y.detach(), leaves[0].grad, blk.conv.weight.grad, blk.conv.bias.grad, blk.norm.weight.grad, blk.norm.bias.grad,
           blk.norm.running_mean.clone(), blk.norm.running_var.clone()]
    assert all(torch.isfinite(t).all() for t in out)
    results.append(out)
  for a, b in zip(*results):
    assert torch.equal(a, b)
  B, C, HW = y.shape[0], y.shape[1], y[0, 0].numel()
  need = _lib.lib().ms_dropout_bn_workspace(B, C, HW)
  # the bare conv's forward and backward ask for theirs; the dropout passes for exactly ms_dropout_bn_workspace, twice -- or not at all
  assert (need > 0) == (B * HW > 4096)
  assert sizes.count(need) >= 2 if need else len(sizes) == 2, (sizes, need)


@pytest.mark.parametrize('frozen', [False, True], ids=['batch', 'frozen'])
@pytest.mark.parametrize('case', [c for c in CASES if c[0] in PICK], ids=lambda c: c[0])
def test_dropout_block_on_exact_poisoned_scratch(case, frozen, monkeypatch):
  _both_poisons(case, monkeypatch, frozen)


def test_dropout_bf16_block_on_exact_poisoned_scratch(monkeypatch):
  _both_poisons([c for c in CASES if c[0] == 'n4098'][0], monkeypatch, False, 'bf16')


@pytest.mark.parametrize('frozen', [0, 1], ids=['batch', 'frozen'])
@pytest.mark.parametrize('channelwise', [0, 1], ids=['element', 'channel'])
def test_entry_points_on_exact_scratch_and_one_byte_short(frozen, channelwise):
  from mix_stage_amd import _lib, ops
  L = _lib.lib()
  B, C, HW = 3, 7, 1367                              # n = 4101 > 4096: the two-pass forms; rows that are no multiple of 4
  need = L.ms_dropout_bn_workspace(B, C, HW)
  assert need == 3 * C * 2 * 4                      # bwd_chunks(3, 7): one chunk per batch item
  gen = torch.Generator().manual_seed(2)
  y_raw, dy = torch.randn(B, C, HW, generator=gen).to(DEV), torch.randn(B, C, HW, generator=gen).to(DEV)
  gamma, beta = (0.5 + torch.rand(C, generator=gen)).to(DEV), torch.randn(C, generator=gen).to(DEV)
  state = ops.dropout_state_words(SEED, 3).to(DEV)
  P = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None
  s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  runs = []
  for poison in POISONS:
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    outs = {}
    for k, n in (('y', B * C * HW), ('save', 4 * C), ('dyr', B * C * HW), ('dg', C), ('db', C)):
      g = guarded(4 * n, DEV, 0x55)
      outs[k] = g.view(torch.float32)
      outs[k]._guard = g._guard
    before = {k: o.clone() for k, o in outs.items()}

    def fwd(ws, nbytes):
      return L.ms_dropout_bn_fwd(P(y_raw), P(gamma), P(beta), P(rm), P(rv), P(outs['y']), P(outs['save']), B, C, HW, 0.2, 1e-5, 0.1, frozen,
                                 channelwise, 0.25, 9, P(state), P(ws), nbytes, s)

    def bwd(ws, nbytes):
      return L.ms_dropout_bn_bwd(P(dy), P(y_raw), P(outs['save']), P(gamma), P(outs['dyr']), P(outs['dg']), P(outs['db']), B, C, HW, 0.2, 1e-5, frozen,
                                 channelwise, 0.25, 9, P(state), P(ws), nbytes, s)
    for fn in (fwd, bwd):
      ws = guarded(need, DEV, poison)
      assert fn(ws, need - 1) != 0 and 'workspace' in L.ms_last_error().decode()
      assert touched(ws) is None and guard_damage(ws) is None
      assert all(torch.equal(outs[k], before[k]) for k in outs) or fn is bwd
      assert fn(ws, need) == 0, L.ms_last_error().decode()
      torch.cuda.synchronize()
      assert guard_damage(ws) is None
    assert all(guard_damage(o) is None for o in outs.values())
    assert frozen or not torch.equal(rm, torch.zeros_like(rm))
    runs.append([o.clone() for o in outs.values()] + [rm, rv])
    assert all(torch.isfinite(t).all() for t in runs[-1])
  for a, b in zip(*runs):
    assert torch.equal(a, b)
