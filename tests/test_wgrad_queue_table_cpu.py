"""CPU guard of tests/helpers/wgrad_queue_table.py (the queued weight gradients' case table): the constants its mirrors use are
the ones in the sources, every entry's claims are what the mirrors compute and reach the branch the entry exists for, and the
comparison helpers of tests/test_gpu_wgrad_queue.py reject a missing slab, swapped jobs, one ulp and a wrong job count."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from helpers import wgrad_queue_checks as C
from helpers import wgrad_queue_table as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mix_stage_amd', 'csrc')


def _src(name):
  with open(os.path.join(CSRC, name)) as f:
    return f.read()


def _int(name, pattern):
  m = re.search(pattern, _src(name))
  assert m, 'csrc/%s no longer has %r: update the mirror in tests/helpers/wgrad_queue_table.py' % (name, pattern)
  return int(m.group(1))


def test_mirror_constants_are_the_sources():
  assert _int('kernels.h', r'constexpr int WGP_MAX_JOBS = (\d+);') == T.WGP_MAX_JOBS
  assert _int('kernels.h', r'constexpr int WG_MAX_JOBS = (\d+);') == T.WG_MAX_JOBS
  assert _int('conv16.h', r'constexpr int WG16_MAX_JOBS = (\d+);') == T.WG16_MAX_JOBS
  assert _int('kernels.h', r'enum \{ REDUCE_BATCH_MAX = (\d+) \};') == T.REDUCE_BATCH_MAX
  assert _int('wgrad_patch.hip', r'\nint g_wgrad_steps_per_wg = (\d+);') == T.WGRAD_STEPS_PER_WG
  assert _int('wgrad_patch.hip', r'\nint g_wgrad_min_wgs = (\d+);') == T.WGRAD_MIN_WGS
  assert _int('wgrad_patch.hip', r'\nint g_wgrad_tiles_per_wg = (\d+);') == T.WGRAD_TILES_PER_WG
  assert _int('wgrad_patch.hip', r'\nint g_wgrad_patch_target_wgs = (\d+);') == T.WGRAD_PATCH_TARGET_WGS
  assert _int('wgrad_patch.hip', r'pl\.n_tiles < \(g_patch_min_wgs > 0 \? (\d+) : 1\)') == T.PATCH_MIN_TILES
  assert _int('conv_patch.hip', r'\nint g_patch_min_wgs = (\d+);') > 0
  assert _int('conv_igemm.hip', r'if \(tiles < (\d+)\) splits = \(int\)\(\(512 \+ tiles - 1\) / tiles\);') == T.GATHER_TILE_TARGET
  # (plan_wgrad16 and its constants live in conv16_plan.h; wgrad16.hip defines the knob from the header's default)
  assert '\nint g_wgrad16_target_wgs = WGRAD16_TARGET_WGS_DEFAULT;' in _src('wgrad16.hip')
  assert _int('conv16_plan.h', r'WGRAD16_TARGET_WGS_DEFAULT = (\d+);') == T.WG16_TARGET_WGS
  assert _int('conv16_plan.h', r'constexpr int WG16_NPX = (\d+);') == T.WG16_NPX
  assert _int('conv16_plan.h', r'splits = std::min\(splits, (\d+)\);') == T.WG16_SPLITS_MAX
  # the wave form of the slab reduction and the 512-block cap of the other two
  m = re.search(r'jb\.wave = \(jb\.splits >= (\d+) && jb\.n <= (\d+)\) \? 1 : 0;', _src('conv_igemm.hip'))
  assert m and (int(m.group(1)), int(m.group(2))) == (T.REDUCE_WAVE_SPLITS, T.REDUCE_WAVE_N)
  m = re.search(r'blocks \+= jb\.wave \? cdiv\(jb\.n, 4\) : std::max\(1, std::min\(cdiv\(jb\.n, (\d+)\), (\d+)\)\);', _src('conv_igemm.hip'))
  assert m and (int(m.group(1)), int(m.group(2))) == (T.REDUCE_PER_BLOCK, T.REDUCE_BLOCK_CAP)
  # the slot rule of queued 16-bit jobs, the pitch it rests on, and the wave_kind numbering
  assert 'inline int wg16_npxt_queued(int npx) { return npx <= 5 ? 5 : 0; }' in _src('wgrad16.hip')
  assert 'inline int wg16_npxt(int npx) { return npx <= 3 ? 3 : npx <= 5 ? 5 : 0; }' in _src('conv16_plan.h')
  assert 'inline int wg16_xpitch(int thpcx) { return ((thpcx + 11) & ~15) + 4; }' in _src('conv16_plan.h')
  assert 'a.wave_kind = mode ? 5 + mode : 2 * S + (wave == 2 ? 1 : 0);' in _src('wgrad_patch.hip')
  cases = re.findall(r'case (\d): wgrad_wave_body<(\d), (\d), (\d)(?:, (\d))?>', _src('wgrad_patch.hip'))
  assert cases == [('2', '1', '2', '2', ''), ('3', '1', '1', '4', ''), ('4', '2', '2', '2', ''), ('5', '2', '1', '4', ''),
                   ('6', '1', '2', '2', '1'), ('7', '1', '2', '2', '2')], cases
  # queued jobs without slabs accumulate, in all three families
  assert 'pw.a.accumulate = a.splits == 1 ? 1 : 0;' in _src('wgrad_patch.hip')
  assert 'w.a.accumulate = a.splits == 1 ? 1 : 0;' in _src('conv_igemm.hip')
  assert 'if (pl.splits == 1) pw.a.accumulate = 1;' in _src('wgrad16.hip')
  # the bars are the parity test's
  from test_gpu_dispatch_parity import KINK_MAX
  assert KINK_MAX == C.KINK_MAX


def test_planner_mirror_reproduces_the_dispatch_table_labels():
  """The unbatched planner's splits are printed by the unqueued launch (dispatch_table.py holds the labels of the production layers
  at B = 32): the mirror must give the same family, steps and splits for each of them."""
  from helpers.dispatch_table import TABLE as DISPATCH
  seen = 0
  for e in DISPATCH:
    if e['prec'] != 'fp32' or e['pair'] or e['mode'] == 'BN_EVAL' or e['knobs']:
      continue
    b = T.Bk(e['nd'], e['B'], e['cin'], e['cout'], e['groups'], e['k'], e['s'], e['p'], e['sp'], e['mode'], e['in_mode'])
    for rx in e['expect']:
      m = re.search(r'conv_wgrad_wave k(\d+)x(\d+) s(\d+) Cog(\d+) Kg(\d+) g(\d+) steps(\d+) splits(\d+)\$$', rx)
      if not m:
        continue
      pl = T.plan_fp32(b, batched=False)
      g = T.geometry(b)
      assert pl['family'] == 'wave', (e['id'], pl)
      rows, imgs = (b['B'], 1) if b['nd'] == 1 else (g['OH'], b['B'])
      assert (g['KH'], g['KW'], g['SW'], b['cout'], b['cin'] * g['KH'] * g['KW'], b['groups'], imgs * rows * T.cdiv(g['OW'], 16), pl['splits']) == \
          tuple(int(v) for v in m.groups()), (e['id'], pl, m.groups())
      seen += 1
  assert seen >= 40, seen


@pytest.mark.parametrize('e', T.TABLE, ids=[e['id'] for e in T.TABLE])
def test_claims_are_what_the_mirrors_compute_and_reach_their_branch(e):
  assert e['claims'] == T.compute_claims(e['blocks'], e['twice'])
  assert not T.check_want(e), (e['id'], T.check_want(e), e['claims'])
  assert e['why'] and e['expect']
  for c, b in zip(e['claims']['blocks'], e['blocks']):
    assert c['splits'] >= 1 and (c['wgs'] > 0) == c['queued'], c
    if c['family'] == 'wave':
      assert 2 <= c['kind'] <= 7
    if c['family'] == 'h16':
      # queued jobs of up to 5 slots share the 5-slot instance; unqueued ones of up to 3 take the 3-slot one
      assert c['npxt'] == (5 if c['npx'] <= 5 else 0) or b['in_mode'] == 'up2'
  # a job limit is never exceeded, and a rollover case really exceeds it
  limit = {'wave': T.WGP_MAX_JOBS, 'patch': T.WGP_MAX_JOBS, 'gather': T.WG_MAX_JOBS, 'h16': T.WG16_MAX_JOBS}
  assert all(l['jobs'] <= limit[l['queue'][0]] for l in e['claims']['launches'])
  if 'rollover' in e['id']:
    assert sorted(l['jobs'] for l in e['claims']['launches'])[-1] == limit[e['claims']['launches'][0]['queue'][0]]


def test_table_covers_what_it_says():
  by = T.BY_ID
  kinds = [c['kind'] for c in by['wave_all_kinds']['claims']['blocks']]
  assert sorted(set(kinds)) == [2, 3, 4, 5, 6, 7]
  assert [l['jobs'] for l in by['wave_all_kinds']['claims']['launches']] == [12]
  assert sorted(l['queue'][1] for l in by['gather_shapes']['claims']['launches']) == [0, 1, 2, 3]
  h16 = by['h16_all@bf16']['claims']['blocks']
  assert any(c['family'] == 'h16' and c['npx'] <= 3 and c['npxt'] == 5 and c['npxt_unqueued'] == 3 for c in h16), 'no block changes its slot instance when queued'
  assert any(c['family'] == 'h16' and 3 < c['npx'] <= 5 for c in h16) and sorted(set(l['queue'][2] for l in by['h16_all@bf16']['claims']['launches'])) == [1, 3, 4]
  assert {c['family'] for c in by['mixed_families']['claims']['blocks']} >= {'wave', 'patch', 'gather'}
  head = by['headline_mix']
  assert all(b['B'] == 32 for b in head['blocks'])
  # the batched planner's splits differ from the ones the dispatch table runs under
  assert [T.plan_fp32(b, True)['splits'] for b in head['blocks']] != [T.plan_fp32(b, False)['splits'] for b in head['blocks']]
  pre = by['prefilled_slot']['claims']['blocks']
  assert {c['family'] for c in pre} >= {'wave', 'patch', 'gather', 'h16', 'c1', 'c1_16'}
  # the reduction's forms: wave, 16-byte, scalar, the grid-stride loop, two launches
  forms = {T.reduce_form(n, s, off % 4 == 0)[0] for _, jobs in T.REDUCE_CASES for n, s, off in jobs}
  assert forms == {'wave', 'vec16', 'scalar'}
  assert T.reduce_form(65536, 32)[0] == 'wave' and T.reduce_form(65537, 32)[0] == 'scalar' and T.reduce_form(1000, 31)[0] == 'vec16'
  assert T.reduce_form(524292, 2) == ('vec16', T.REDUCE_BLOCK_CAP) and 524292 // 4 > T.REDUCE_BLOCK_CAP * 256
  assert T.reduce_launches(97) == [96, 1] and T.reduce_launches(0) == []


# ---- the comparison helpers have teeth ------------------------------------------------------------------------------------------------------
def _fake_run(b, seed):
  """A block's `device` results made from the float64 reference itself (rounded to float32): what a correct kernel would return."""
  gen = torch.Generator().manual_seed(seed)
  g = T.geometry(b)
  ctot, cin_tot = b['cout'] * b['groups'], b['cin'] * b['groups']
  params = dict(w=torch.randn(ctot, b['cin'], g['KW'], generator=gen) * (b['cin'] * g['KW']) ** -0.5, bias=torch.randn(ctot, generator=gen) * 0.1,
                gamma=0.5 + torch.rand(ctot, generator=gen), beta=torch.randn(ctot, generator=gen) * 0.1)
  rm0, rv0 = torch.randn(ctot, generator=gen) * 0.1, 0.5 + torch.rand(ctot, generator=gen)
  x = torch.randn(b['B'], cin_tot, g['W'], generator=gen)
  gy = torch.randn(b['B'], ctot, g['OW'], generator=gen)
  raw = F.conv1d(x, params['w'], params['bias'], stride=g['SW'], padding=g['PW'], groups=b['groups'])
  y = raw if b['mode'] == 'BARE' else F.leaky_relu(F.batch_norm(raw, None, None, params['gamma'], params['beta'], True), 0.2)
  use = dict(xs=[x], gy=gy, y=y)
  ref = C.reference(b, params, [use], rm0, rv0)
  f32 = lambda t: None if t is None else t.float()
  got = dict(y=[f32(t) for t in ref['y']], dx0=[f32(t) for t in ref['dx0']], dx1=[None], dw=f32(ref['dw']), dbias=f32(ref['dbias']),
             dgamma=f32(ref['dgamma']), dbeta=f32(ref['dbeta']), rm=f32(ref['rm']), rv=f32(ref['rv']))
  return params, use, ref, got


def test_fp64_bars_reject_a_missing_slab_and_swapped_jobs():
  bn = T.Bk(1, 4, 8, 16, 1, 3, 1, 1, (32,))
  bare = T.Bk(1, 4, 8, 16, 1, 3, 1, 1, (32,), mode='BARE')
  for b in (bn, bare):
    _, _, ref, got = _fake_run(b, 1)
    assert not C.failed(C.bars(b, got, ref)), C.bars(b, got, ref)
  # one slab left out: the weight gradient of a BARE block is the sum of its batch items' (its pixel splits are runs of them)
  params, use, ref, got = _fake_run(bare, 2)
  slabs = [torch.nn.grad.conv1d_weight(use['xs'][0][i:i + 1].double(), params['w'].shape, use['gy'][i:i + 1].double(), stride=1, padding=1)
           for i in range(bare['B'])]
  assert C.rel_err(sum(slabs), ref['dw']) < 1e-12
  for leave in range(bare['B']):
    bad = dict(got, dw=sum(s for i, s in enumerate(slabs) if i != leave).float())
    assert 'dw' in C.failed(C.bars(bare, bad, ref)), leave
  # two jobs' dw swapped (same layer, different data)
  _, _, ref_a, got_a = _fake_run(bn, 3)
  _, _, ref_b, got_b = _fake_run(bn, 4)
  assert 'dw' in C.failed(C.bars(bn, dict(got_a, dw=got_b['dw']), ref_a)) and 'dw' in C.failed(C.bars(bn, dict(got_b, dw=got_a['dw']), ref_b))
  # ... and the other per-channel gradients
  assert 'dgamma' in C.failed(C.bars(bn, dict(got_a, dgamma=got_b['dgamma']), ref_a))


def test_bit_equality_rejects_one_ulp():
  b = T.Bk(1, 4, 8, 16, 1, 3, 1, 1, (32,))
  _, _, ref, got = _fake_run(b, 5)
  assert C.differing(got, dict(got)) == []
  for name in ('dw', 'dgamma', 'dx0'):
    t = (got[name][0] if name == 'dx0' else got[name]).clone()
    flat = t.view(-1)
    flat[flat.numel() // 2] = torch.nextafter(flat[flat.numel() // 2], torch.tensor(float('inf')))
    moved = dict(got, **{name: [t] if name == 'dx0' else t})
    assert C.differing(got, moved) == [name + ('[0]' if name == 'dx0' else '')]
    assert not C.failed(C.bars(b, moved, ref)), 'one ulp is far inside the fp64 bars: only the bit comparison sees it'
  assert C.differing(got, dict(got, dw=got['dw'] + 0.0)) == []
  assert C.differing(got, dict(got, dw=-got['dw'] * 0.0 + got['dw'])) == []


def test_label_check_rejects_a_wrong_job_count_a_foreign_job_and_an_unqueued_launch():
  e = T.BY_ID['gather_rollover']
  good = {r'wgrad_multi_kernel<1>|conv_wgrad_gather multi shape1 jobs24 wgs%d' % e['claims']['launches'][0]['wgs']: 1,
          r'wgrad_multi_kernel<1>|conv_wgrad_gather multi shape1 jobs2 wgs%d' % e['claims']['launches'][1]['wgs']: 1, 'bn_bwd_fused<1> C64 N8': 26}
  C.check_labels(e, good)
  dropped = dict(good)
  dropped.pop(next(k for k in good if 'jobs2 ' in k))
  stale = dict(good, **{'wgrad_multi_kernel<1>|conv_wgrad_gather multi shape1 jobs3 wgs3': 1})
  twice = {k: (2 if 'jobs24' in k else n) for k, n in good.items()}
  unqueued = dict(good, **{'wgrad_kernel<1,1,1,3,0>|conv_wgrad k1x3 s1 Cog64 Kg192 g1 N8 splits1': 1})
  for bad in (dropped, stale, twice, unqueued):
    with pytest.raises(AssertionError):
      C.check_labels(e, bad)
