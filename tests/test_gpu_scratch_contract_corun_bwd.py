"""GPU: the scratch contract (tests/helpers/guarded_scratch.py) for a merged DATA-GRADIENT launch: the host and the held guest of
tests/test_gpu_clip_corun_bwd.py, each on an exactly-sized, poisoned workspace of its own."""
import ctypes

import pytest
import torch

from helpers.guarded_scratch import POISONS, guard_damage, guarded, touched

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_corun_bwd_pair_on_exact_poisoned_scratch():
  """Host: a UNet down block's data gradient with dx_accum; held guest: a style-encoder block's data gradient that carries its
  producer's BatchNorm backward (partials of the meeting and the prepared weights live in the workspace).  The results are the bits
  of the two launches one by one on roomy workspaces."""
  from mix_stage_amd import _lib as L
  from test_gpu_clip_corun import PAIR_MARK, _labels
  from test_gpu_clip_corun_bwd import GUESTS, HOSTS, BwdBlock, _alone, _held_then, _same

  def make():
    return BwdBlock(8, T=16, seed=1, **HOSTS['down8_acc']), BwdBlock(8, T=16, seed=2, **GUESTS['dg4_64to128'])
  h0, g0 = make()
  _alone(g0, h0)
  torch.cuda.synchronize()
  alone = (h0.state(), g0.state())
  for poison in (None,) + POISONS:
    h, g = make()
    for blk in (h, g):
      n = L.lib().ms_conv_block_bwd_workspace(ctypes.byref(blk.d))
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
