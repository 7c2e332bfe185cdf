"""CPU: the rounding model behind the fp16 bars (tests/helpers/round16_model.py) and the two conditions every case of
tests/helpers/fp16_block_table.py must meet with the seed the GPU test uses -- conditions on the cases, not on a kernel."""
import pytest
import torch

from helpers import round16_model as M
from helpers.fp16_block_table import TABLE, SCALED, BY_ID, TINY_DY, LOSS_SCALES, OVERFLOW
from helpers.conv16_plan_table import ENTRIES as PLAN_ENTRIES

TYPES = [torch.bfloat16, torch.float16]
FLIP_FRAC = 2e-3                # _case's flip_frac


def _probe_values(dt):
  """fp32 values across the type's range: normal, subnormal, ties, the overflow threshold, signed zeros, non-finite."""
  p, emin, emax = M.FORMATS[dt]
  g = torch.Generator().manual_seed(0)
  mant = 1.0 + torch.rand(4096, generator=g)
  expo = torch.randint(emin - p - 3, emax + 1, (4096,), generator=g).float()
  v = mant * torch.exp2(expo) * torch.where(torch.rand(4096, generator=g) < 0.5, -1.0, 1.0)
  tiny, big = 2.0 ** (emin - (p - 1)), 2.0 ** emax * (2.0 - 2.0 ** (1 - p))
  half_ulp_top = 2.0 ** (emax - p)
  edge = torch.tensor([0.0, -0.0, tiny, tiny / 2, tiny * 0.5000001, tiny * 1.5, tiny * 2.5, 2.0 ** emin, 2.0 ** emin * (1 - 2.0 ** -p),
                       big, big + half_ulp_top * 0.999, big + half_ulp_top, big * 1.01, -big - half_ulp_top, 1.0 + 2.0 ** -p,
                       1.0 + 3 * 2.0 ** -p, float('inf'), -float('inf'), float('nan')])
  ties = (torch.arange(1, 257).float() + 0.5) * 2.0 ** (1 - p)          # k + 1/2 units in the last place of [1, 2)
  n = min(256, 2 ** (p - 1) - 1)
  return torch.cat([v, edge, 1.0 + ties[:n], -(1.0 + ties[:n]), ties * tiny / 2.0 ** (1 - p)]).float()


@pytest.mark.parametrize('dt', TYPES, ids=['bf16', 'fp16'])
def test_round16_equals_the_cast(dt):
  v = _probe_values(dt)
  got, ref = M.round16(v.double(), dt), v.to(dt).double()
  assert torch.equal(torch.isnan(got), torch.isnan(ref))
  ok = ~torch.isnan(ref)
  assert torch.equal(got[ok], ref[ok]), (v[ok][got[ok] != ref[ok]][:8], got[ok][got[ok] != ref[ok]][:8], ref[ok][got[ok] != ref[ok]][:8])
  assert torch.equal(torch.signbit(got[ok]), torch.signbit(ref[ok]))
  # what the probe set must contain to mean anything
  p, emin, emax = M.FORMATS[dt]
  assert torch.isinf(ref[torch.isfinite(v)]).any()                                            # overflow to inf
  sub = ok & (ref != 0) & (ref.abs() < 2.0 ** emin)
  assert sub.sum() > 20 and ((ref == 0) & (v != 0)).any()                                     # subnormals, underflow to 0


@pytest.mark.parametrize('dt', TYPES, ids=['bf16', 'fp16'])
def test_power_of_two_scale_is_exact_on_normal_values(dt):
  p, emin, emax = M.FORMATS[dt]
  g = torch.Generator().manual_seed(1)
  v = ((1.0 + torch.rand(4096, generator=g)) * torch.exp2(torch.randint(emin + 1, emax - 17, (4096,), generator=g).float())).double()
  v = v * torch.where(torch.rand(4096, generator=g) < 0.5, -1.0, 1.0).double()
  for k in (1, 10, 16):
    S = 2.0 ** k
    assert torch.equal(M.round16_scaled(v, dt, S), M.round16(v, dt))             # S * v stays normal and finite
  # ... and is what rescues a subnormal value: 1e-7 loses bits unscaled, none (beyond one rounding) at 2^16
  if dt == torch.float16:
    t = torch.full((1,), 1e-7, dtype=torch.float64)
    assert abs(M.round16(t, dt).item() / 1e-7 - 1) > 0.1
    assert abs(M.round16_scaled(t, dt, 2.0 ** 16).item() / 1e-7 - 1) <= 2.0 ** -11


@pytest.mark.parametrize('c', TABLE, ids=[c['id'] for c in TABLE])
def test_case_separates_the_types_and_stays_off_the_kink(c):
  """Emulated bf16 error / emulated fp16 error in [5, 12] for fwd, dx l2 and dw l2: the case is dominated by the type's rounding,
  so 3 x the fp16 figure refuses a bf16-grade result.  (fp32 outputs have no forward rounding: no ratio there.)  Every case
  is modelled as its GPU run is set up -- the y / y_raw cases with the exact mask: a seed at which an activation mask taken from
  the rounded conv output flipped in fp16 would show in the figures below and in the GPU bars; in bf16 it lands far outside the
  ratio and the seed is refused here.
  Kink band share <= flip_frac / 2 for the seed the GPU test uses."""
  f, b = M.case_model(c, torch.float16), M.case_model(c, torch.bfloat16)
  checks = ['dx l2', 'dw l2'] + ([] if (c['out_f32'] and c['mode'] != 'BN_TRAIN') else ['fwd'])
  ratios = {k: b[k] / f[k] for k in checks}
  assert all(5.0 <= r <= 12.0 for r in ratios.values()), ratios
  assert f['kink share'] <= FLIP_FRAC / 2 and b['kink share'] >= f['kink share'], (f['kink share'], b['kink share'])
  # the model's fp16 figures are of the size of one fp16 rounding (u = 2^-11), never of bf16's
  assert all(2.0 ** -14 <= f[k] <= 2.0 ** -10 for k in checks), {k: f[k] for k in checks}


@pytest.mark.parametrize('c', PLAN_ENTRIES, ids=[c['id'] for c in PLAN_ENTRIES])
def test_plan_table_case_separates_the_types_and_stays_off_the_kink(c):
  """The plan-class shapes of tests/helpers/conv16_plan_table.py (tests/test_gpu_conv16_plans.py runs them in fp16 under
  bars='dtype'), held to the same conditions with the seeds that test uses."""
  test_case_separates_the_types_and_stays_off_the_kink(c)


@pytest.mark.parametrize('cid', SCALED)
def test_tiny_gradients_need_the_scale_and_get_it_back(cid):
  """dy elements of 1e-7: unscaled, fp16's subnormal spacing (6e-8) eats them; with S = 2^16 or 2^10 the emulated errors are
  those of the unit-size gradient again -- the reference alone meets the bars the GPU test sets."""
  c = BY_ID[cid]
  unit = M.case_model(c, torch.float16)
  lost = M.case_model(c, torch.float16, S=1.0, dy_scale=TINY_DY)
  assert lost['dx l2'] > 0.1 and lost['dw l2'] > 0.1, lost
  for S in LOSS_SCALES:
    m = M.case_model(c, torch.float16, S=S, dy_scale=TINY_DY)
    for k in unit:
      if k == 'kink share' or unit[k] == 0.0:
        continue
      # 2^16 lifts everything into the normal range; at 2^10 (1e-7 -> 1e-4) the small end of dy, dy_raw and dx is still subnormal:
      # somewhat more, yet within the bar of the unit-size gradient (3 x its figure), which is the bar the GPU test holds it to
      assert m[k] <= (1.25 if (S == 2.0 ** 16 and k.endswith(' l2')) else 3.0) * unit[k], (S, k, m[k], unit[k])


@pytest.mark.parametrize('c', OVERFLOW, ids=[c['id'] for c in OVERFLOW])
def test_overflow_blocks_stay_off_the_kink(c):
  """The LeakyReLU overflow block's reference takes its slopes from the device's signs, as the table cases do: same condition."""
  assert M.case_model(c, torch.float16, S=2.0 ** 10)['kink share'] <= FLIP_FRAC / 2
