"""The guarded-scratch allocator of tests/helpers/guarded_scratch.py on host memory: geometry, what `check` sees and how it names it."""
import pytest
import torch

from helpers.guarded_scratch import ALIGN, GUARD, guard_damage, guarded, guarded_like, check, touched


@pytest.mark.parametrize('nbytes', [0, 1, 255, 256, 4097, (1 << 20) + 3])
@pytest.mark.parametrize('poison', [0xFF, 0x55])
def test_geometry_poison_and_clean_guards(nbytes, poison):
  v = guarded(nbytes, 'cpu', poison)
  g = v._guard
  assert v.dtype == torch.uint8 and v.numel() == nbytes and (g['whole'].data_ptr() + g['start']) % ALIGN == 0
  assert g['start'] >= GUARD and g['whole'].numel() - g['start'] - nbytes >= GUARD
  assert nbytes == 0 or v.data_ptr() == g['whole'].data_ptr() + g['start']
  assert bool((v == poison).all())
  assert guard_damage(v) is None and touched(v) is None
  check(v)


def test_poison_values_are_what_the_tests_rely_on():
  assert bool(torch.isnan(guarded(64, 'cpu', 0xFF).view(torch.float32)).all())
  assert bool(torch.isnan(guarded(64, 'cpu', 0xFF).view(torch.bfloat16).float()).all())
  assert bool(torch.isnan(guarded(64, 'cpu', 0xFF).view(torch.float16).float()).all())
  assert bool((guarded(64, 'cpu', 0xFF).view(torch.int32) == -1).all())
  f = guarded(64, 'cpu', 0x55).view(torch.float32)
  assert bool(torch.isfinite(f).all()) and float(f[0]) > 1e12


def test_overrun_and_underrun_are_named_by_their_offsets():
  v = guarded(1000, 'cpu', 0x55)
  whole, start = v._guard['whole'], v._guard['start']
  whole[start + 1000 + 3] ^= 0xFF          # 4th byte past the end
  whole[start + 1000 + 40] ^= 0xFF
  msg = guard_damage(v)
  assert 'bytes +3 .. +40 past the end of the 1000 claimed bytes' in msg
  with pytest.raises(AssertionError, match='scratch overrun'):
    check(v)
  v = guarded(1000, 'cpu', 0x55)
  v._guard['whole'][v._guard['start'] - 1] ^= 0xFF
  assert 'bytes -1 .. -1 in front of the region' in guard_damage(v)
  # the far ends of both guards are watched too
  v = guarded(8, 'cpu', 0x55)
  v._guard['whole'][0] ^= 0xFF
  v._guard['whole'][-1] ^= 0xFF
  msg = guard_damage(v)
  assert 'past the end' in msg and 'in front of' in msg


def test_touched_reports_the_written_range_and_typed_views_share_the_guard():
  w = torch.zeros(10)
  v = guarded_like(w, 0xFF)
  assert v.dtype == torch.float32 and v.numel() == 10 and v.data_ptr() % ALIGN == 0
  v[2] = 1.0
  v[7] = 2.0
  assert touched(v) == (8, 31)
  assert guard_damage(v) is None
