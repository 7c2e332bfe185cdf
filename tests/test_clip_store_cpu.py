"""Device-resident clip store: the host-side arithmetic (window table, epoch order, sharding) and the constructor's refusals.  No GPU."""
import pytest
import torch

from mix_stage_amd.clip_store import DeviceClipStore, draw_positions, epoch_order, steps_per_epoch, window_table

LENGTHS = [0, 63, 64, 65, 127, 128, 200]


def _brute(lengths, T, hop):
  wi, ws = [], []
  for i, n in enumerate(lengths):
    start = 0
    while start + T <= n:
      wi.append(i)
      ws.append(start)
      start += hop
  return wi, ws


@pytest.mark.parametrize('T,hop', [(64, 1), (64, 5), (64, 64), (64, 100), (32, 3)])
def test_window_table_against_brute_force(T, hop):
  wi, ws = window_table(LENGTHS, T, hop)
  ref_i, ref_s = _brute(LENGTHS, T, hop)
  assert wi.dtype == torch.int64 and ws.dtype == torch.int64
  assert wi.tolist() == ref_i and ws.tolist() == ref_s
  assert len(ref_i) > 0 and set(ref_i) == {i for i, n in enumerate(LENGTHS) if n >= T}      # an interval shorter than T holds no window
  for i, s in zip(ref_i, ref_s):
    assert s + T <= LENGTHS[i]


def test_window_table_refuses_hop_below_one():
  with pytest.raises(ValueError):
    window_table(LENGTHS, 64, 0)


def test_epoch_order():
  W = 40
  a, b = epoch_order(W, 3, 0), epoch_order(W, 3, 0)
  assert a.dtype == torch.int32 and sorted(a.tolist()) == list(range(W))
  assert torch.equal(a, b)
  c = epoch_order(W, 3, 1)
  assert sorted(c.tolist()) == list(range(W)) and not torch.equal(a, c)
  assert torch.equal(a, torch.randperm(W, generator=torch.Generator().manual_seed(3)).to(torch.int32))
  assert torch.equal(epoch_order(W, 2, 1), a)                                # the generator's seed is seed + epoch


def test_sharding_two_ranks():
  W, B, world = 40, 3, 2
  steps = steps_per_epoch(W, B, world)
  assert steps == 6
  drawn = {0: [], 1: []}
  cursor = 0
  for _ in range(steps):
    for rank in range(world):
      drawn[rank].extend(draw_positions(cursor, B, rank, world))
    cursor += world * B
  assert len(drawn[0]) == len(drawn[1]) == 18
  assert not set(drawn[0]) & set(drawn[1])
  assert sorted(drawn[0] + drawn[1]) == list(range(36))                      # exactly the first 36 positions: the remainder is not drawn
  assert steps_per_epoch(7, 3) == 2 and steps_per_epoch(5, 3, 2) == 0


def _interval(n, P=104, F=128, style=0):
  return torch.zeros(n, P), torch.zeros(n, F), style


def test_constructor_refusals_before_any_device_use():
  # (device='cuda:0' throughout: every one of these raises on the shapes alone, on a machine without a GPU)
  with pytest.raises(ValueError, match='no window'):
    DeviceClipStore([_interval(63), _interval(10)], T=64, hop=5)
  with pytest.raises(ValueError, match='no window'):
    DeviceClipStore([], T=64, hop=5)
  for hop in (0, -3):
    with pytest.raises(ValueError, match='hop'):
      DeviceClipStore([_interval(100)], T=64, hop=hop)
  with pytest.raises(ValueError, match='P ='):
    DeviceClipStore([_interval(100), _interval(100, P=102)], T=64, hop=5)
  with pytest.raises(ValueError, match='F ='):
    DeviceClipStore([_interval(100), _interval(100, F=5)], T=64, hop=5)
  for style in (2 ** 31, -2 ** 31 - 1):
    with pytest.raises(ValueError, match='int32'):
      DeviceClipStore([_interval(100, style=style)], T=64, hop=5)
  with pytest.raises(ValueError):
    DeviceClipStore([(torch.zeros(100, 104), torch.zeros(99, 128), 0)], T=64, hop=5)     # pose and audio frames differ


def test_c_abi_is_declared_bound_and_built():
  """include/mixstage.h declares the two entry points, _lib.SIGNATURES binds them with as many arguments, the Makefile builds the file."""
  import os
  import re
  from mix_stage_amd._lib import SIGNATURES
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  header = open(os.path.join(root, 'include', 'mixstage.h')).read()
  for name in ('ms_clip_draw', 'ms_clip_advance'):
    m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
    assert m, name
    assert len(m.group(1).split(',')) == len(SIGNATURES[name][1]), name
  assert re.search(r'^SRCS\s*=.*\bclip_store\.hip\b', open(os.path.join(root, 'mix_stage_amd', 'csrc', 'Makefile')).read(), re.M)


def test_rank_and_world_are_fixed_at_construction():
  """Given explicitly, taken from a trainer's shard(), or 0 / 1 -- before the first new_epoch(), whose steps_left counts with world."""
  class Trainer:
    def shard(self):
      return (1, 2)
  one = [_interval(64 + 39)]                                  # hop 1: 40 windows
  plain = DeviceClipStore(one, T=64, hop=1, device='cpu', batch_size=3)
  bound = DeviceClipStore(one, T=64, hop=1, device='cpu', batch_size=3, trainer=Trainer())
  given = DeviceClipStore(one, T=64, hop=1, device='cpu', batch_size=3, rank=0, world=4, trainer=Trainer())
  assert (plain.rank, plain.world) == (0, 1) and (bound.rank, bound.world) == (1, 2) and (given.rank, given.world) == (0, 4)
  for store, steps in ((plain, 13), (bound, 6), (given, 3)):
    store.new_epoch()
    assert (store.W, store.steps_left) == (40, steps)
    assert store._order.numel() == 40 + store.max_batch * store.world and int(store._order[40:].max()) == -1
  for bad in (dict(rank=2, world=2), dict(rank=-1, world=1), dict(rank=0), dict(world=2)):
    with pytest.raises(ValueError):
      DeviceClipStore(one, T=64, hop=1, device='cpu', **bad)
