"""CPU: the wait-free eval form of the chained decoder (ms_decoder_chain_eval_*, include/mixstage.h) -- its host-side entry
points (pure arithmetic on the shape: no GPU) and the tile plan they return, restated in float64 torch and compared with the
untiled segment."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

T_LIST = [1, 5, 56, 60, 61, 64, 72, 200, 640, 1000]


def _desc(B, M, T, mode=None, dtype=0, C=256, P=104, cin0=266):
  from mix_stage_amd import _lib
  mode = _lib.MS_BN_EVAL if mode is None else mode
  return _lib.ChainDesc(B, M, T, cin0, C, P, 4, mode, dtype, 32, 0, 0.2, 1e-5, 0.1)


def _plan(d):
  from mix_stage_amd import _lib
  L = _lib.lib()
  n, gpw = ctypes.c_int32(), ctypes.c_int32()
  assert L.ms_decoder_chain_eval_plan(ctypes.byref(d), ctypes.byref(n), ctypes.byref(gpw), None, None, None, 0) == 0
  cap = n.value
  first, lo, hi = [(ctypes.c_int32 * cap)() for _ in range(3)]
  assert L.ms_decoder_chain_eval_plan(ctypes.byref(d), ctypes.byref(n), ctypes.byref(gpw), first, lo, hi, cap) == 0
  return n.value, gpw.value, list(first), list(lo), list(hi)


@pytest.mark.parametrize('B', [1, 1024])
@pytest.mark.parametrize('M', [1, 8, 25])
def test_plan_partitions_every_sequence(B, M):
  from mix_stage_amd import _lib
  L = _lib.lib()
  for T in T_LIST:
    d = _desc(B, M, T)
    assert L.ms_decoder_chain_eval_supported(ctypes.byref(d)) == 1
    n, gpw, first, lo, hi = _plan(d)
    assert n >= 1 and len(first) == n
    owner = [0] * T
    for k in range(n):
      assert 0 <= lo[k] < hi[k] <= T
      for f in range(lo[k], hi[k]):
        owner[f] += 1
      # owned frames lie inside the tile's 64 computed frames ...
      assert first[k] <= lo[k] and hi[k] <= first[k] + 64
      # ... and at least 4 frames from a tile edge that is not an end of the sequence
      if first[k] > 0:
        assert lo[k] >= first[k] + 4
      if first[k] + 64 < T:
        assert hi[k] <= first[k] + 64 - 4
    assert owner == [1] * T, (T, first, lo, hi)
    # the groups of a tile: ceil(M / gpw) workgroups of gpw groups (the last one the rest) cover 0..M-1 once
    assert 1 <= gpw <= M
    groups = [g for j in range((M + gpw - 1) // gpw) for g in range(j * gpw, min(M, (j + 1) * gpw))]
    assert groups == list(range(M))
    # few work units: the groups spread over workgroups; many: one workgroup carries them all and nothing is exchanged
    words, wsp = L.ms_decoder_chain_eval_sync_words(ctypes.byref(d)), L.ms_decoder_chain_eval_workspace(ctypes.byref(d))
    if gpw == M:
      assert words == 0 and wsp <= 256
    else:
      ngw = (M + gpw - 1) // gpw
      assert words >= B * n and wsp >= B * n * ngw * 104 * 64 * 4


def test_many_units_carry_several_groups_per_workgroup():
  """The c5 shape: one fp32 term per (clip, group) would be B*M*128*64*4 = 268 MB; the plan must need at most half of it."""
  from mix_stage_amd import _lib
  L = _lib.lib()
  d = _desc(1024, 8, 64, dtype=_lib.MS_F16)
  assert L.ms_decoder_chain_eval_supported(ctypes.byref(d)) == 1
  assert L.ms_decoder_chain_eval_workspace(ctypes.byref(d)) <= 134 * 1000 * 1000
  n, gpw, _, _, _ = _plan(d)
  assert n == 1 and gpw >= 2


def test_supported_is_a_shape_rule():
  from mix_stage_amd import _lib
  L = _lib.lib()
  ok = lambda d: L.ms_decoder_chain_eval_supported(ctypes.byref(d))
  assert ok(_desc(1, 8, 640)) == 1 and ok(_desc(4096, 32, 64)) == 1          # no compute-unit condition
  assert ok(_desc(1, 8, 640, mode=_lib.MS_BN_TRAIN)) == 0
  assert ok(_desc(1, 8, 640, C=128)) == 0
  assert ok(_desc(1, 33, 640)) == 0
  assert ok(_desc(1, 8, 640, P=129)) == 0
  assert ok(_desc(1, 8, 0)) == 0
  # train mode is refused with a message, not served
  n = ctypes.c_int32()
  assert L.ms_decoder_chain_eval_plan(ctypes.byref(_desc(1, 8, 640, mode=_lib.MS_BN_TRAIN)), ctypes.byref(n), None, None, None, None, 0) != 0
  assert b'MS_BN_EVAL' in L.ms_last_error()
  # the weight streams do not depend on B or T
  a, b = _desc(32, 8, 64), _desc(1, 8, 1000)
  assert L.ms_decoder_chain_prepared_bytes(ctypes.byref(a)) == L.ms_decoder_chain_prepared_bytes(ctypes.byref(b)) > 0


def _layers(M, cin0, seed=0):
  g = torch.Generator().manual_seed(seed)
  ws = [torch.randn(16 * M, cin0 if l == 0 else 16, 3, generator=g, dtype=torch.float64) * 0.2 for l in range(4)]
  bs = [torch.randn(16 * M, generator=g, dtype=torch.float64) for _ in range(4)]       # (bias + BatchNorm shift: nonzero beyond T)
  return ws, bs


def _stack(h, ws, bs, M, T_valid=None):
  for w, b in zip(ws, bs):
    h = F.leaky_relu(F.conv1d(h, w, b, padding=1, groups=M), 0.2)
    if T_valid is not None:
      h[..., T_valid:] = 0                 # frames outside the sequence are zero at the input of every layer
  return h


@pytest.mark.parametrize('T', T_LIST)
def test_tile_plan_reproduces_the_untiled_segment_in_float64(T):
  """Four k3 / pad 1 layers over the tiles ms_decoder_chain_eval_plan returns (64 computed frames from a zero halo, frames
  beyond T masked after every layer, owned frames copied out) against the same layers over the whole sequence."""
  M, cin0 = 2, 5
  ws, bs = _layers(M, cin0)
  x = torch.randn(2, cin0, T, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
  ref = _stack(torch.cat([x] * M, 1), ws, bs, M)
  n, _, first, lo, hi = _plan(_desc(2, M, T))
  out = torch.full_like(ref, float('nan'))
  for k in range(n):
    s = first[k]
    tile = torch.zeros(2, cin0, 64, dtype=torch.float64)
    nv = min(64, T - s)
    tile[..., :nv] = x[..., s:s + nv]
    y = _stack(torch.cat([tile] * M, 1), ws, bs, M, T_valid=nv)
    out[..., lo[k]:hi[k]] = y[..., lo[k] - s:hi[k] - s]
  assert torch.isfinite(out).all()
  assert float((out - ref).abs().max()) <= 1e-12
