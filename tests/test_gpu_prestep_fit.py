"""GPU: fitting the pre-step on the device (mix_stage_amd/fit.py, csrc/prestep_fit.hip) against the NumPy float64 mirror of
tests/helpers/kmeans_ref.py.

Inputs: a few pose prototypes + a cumulative random walk + noise, cast to fp32 (kmeans_ref.make_pose).  A condition on the
reference alone makes every label comparable: the mirror's smallest relative gap (d2 - d1) / d2 between the best and the
second-best squared distance, over all rows and Lloyd iterations, must exceed 1e-9.  Device and mirror distances differ by at most
about W * 2^-52 ~ 5e-14 relative, so above that gap every label must be equal -- no row is excluded.  (The mirror on the CPU, the cases below: smallest gap over all Lloyd
iterations 2.1e-4 in CASES, 1.3e-5 in the restarts of the n_init test; every test asserts the condition before it compares.)

Bars, derived (fp64 sums of n terms on both sides, any order: each side is within (n - 1) * 2^-53 * sum|x| of the exact sum):
  labels equal;  |centre - ref| <= n_m * 2^-52 * max|f[:, w]| per column, n_m = the cluster's count (a cluster that ends empty
  keeps the centre of the iteration that last gave it rows: n_m is that iteration's count, and 0 -- the bits it was given --
  for a cluster that never had a row);  inertia to N * W * 2^-52 relative;  column mean to N * 2^-52 * max|x|, variance to
  N * 2^-52 * max|x|^2.
The speed block's sqrt(vx^2 + vy^2) may be contracted to one fma on the device (one rounding fewer than the mirror's): at most
1 ulp of a feature, which the centre bar's factor 2 over the practical sqrt(n) growth of a sum's error covers.
Measured worst ratios (value / bar): profiles/kmeans_fit.json."""
import functools

import numpy as np
import pytest
import torch

from helpers import guarded_scratch as GS
from helpers import kmeans_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -52
GAP_MIN = 1e-9
KEEP = R.keep_columns()
PK = len(KEEP)
FEAT_NAMES = {b: tuple(n for n, bit in (('pose', 1), ('velocity', 2), ('speed', 4)) if b & bit) for b in range(1, 8)}
WORST = {}                   # name of a bar -> the largest value / bar seen (what profiles/kmeans_fit.json records)

# id -> (seed, B, T, M, feats): every feats at (5,13) = 65 rows (two workgroups of 33 and 32 rows); T = 1; one row; M = 1 and
# M = 25; 512 rows (8 full slices), 63 rows (one short slice), 259 rows (5 slices of 52: rounds of 32 + 20)
CASES = dict([('feats%d' % f, (10 + f, 5, 13, 3, f)) for f in range(1, 8)] +
             [('t1', (21, 3, 1, 2, 1)), ('one_row', (22, 1, 1, 1, 1)), ('m1', (23, 5, 13, 1, 7)), ('m25', (24, 8, 64, 25, 3)),
              ('m8_512', (25, 8, 64, 8, 7)), ('speed_63', (26, 7, 9, 8, 4)), ('rows_259', (27, 7, 37, 4, 7))])


def _record(name, value, bar):
  value, bar = np.asarray(value, dtype=np.float64), np.asarray(bar, dtype=np.float64)
  ratio = float(np.max(np.where(bar > 0, value / np.where(bar > 0, bar, 1.0), np.where(value > 0, np.inf, 0.0))))
  WORST[name] = max(WORST.get(name, 0.0), ratio)
  print('%s: worst value / bar = %.3g' % (name, ratio))
  return ratio


@functools.lru_cache(maxsize=None)
def _reference(case):
  """(pose fp32 (B,T,P), feature rows, init, the mirror's fit) -- computed once per case, never modified."""
  seed, B, T, M, feats = CASES[case]
  pose = R.make_pose(seed, B, T)
  f = R.feature_rows(pose, KEEP, feats)
  init = R.draw_init(f, M, seed, T=T, skip_first_frame=not (feats & 1))
  ref = R.lloyd(f, init)
  for a in (pose, f, init, ref['centers'], ref['labels'], ref['counts']):
    a.setflags(write=False)
  return pose, f, init, ref


def _fitter(M, feats):
  from mix_stage_amd.fit import DeviceKMeansFit
  return DeviceKMeansFit(M, feats=FEAT_NAMES[feats], device=DEV)


def _compare(res, f, ref, init, tag):
  """Labels, centres, inertia, counts and the number of iterations of a device fit against the mirror's."""
  assert ref['min_gap'] > GAP_MIN, 'the reference has a near tie (gap %.3g): not a case for this test' % ref['min_gap']
  labels = torch.cat([l.reshape(-1) for l in res.labels]).cpu().numpy()
  np.testing.assert_array_equal(labels, ref['labels'])
  np.testing.assert_array_equal(res.counts.cpu().numpy(), ref['counts'])
  assert res.n_iter == ref['n_iter']
  c = res.centers.cpu().numpy()
  assert c.dtype == np.float64
  bar = ref['last_counts'][:, None] * U * np.abs(f).max(axis=0)[None, :]
  err = np.abs(c - ref['centers'])
  ratio = _record('centre', err, bar)
  assert ratio <= 1.0, '%s: centre error %.3g of its bar' % (tag, ratio)
  never = ref['last_counts'] == 0
  np.testing.assert_array_equal(c[never], np.asarray(init)[never])          # a cluster without rows keeps its centre, bit for bit
  N, W = f.shape
  ibar = N * W * U * abs(ref['inertia'])
  iratio = _record('inertia', abs(res.inertia - ref['inertia']), ibar)
  assert iratio <= 1.0 or res.inertia == ref['inertia'], '%s: inertia %.17g vs %.17g' % (tag, res.inertia, ref['inertia'])


@pytest.mark.parametrize('case', sorted(CASES))
def test_fit_equals_the_mirror(case):
  seed, B, T, M, feats = CASES[case]
  pose, f, init, ref = _reference(case)
  res = _fitter(M, feats).fit([torch.tensor(pose, device=DEV)], init)
  _compare(res, f, ref, init, case)


def test_labels_of_the_fit_are_the_labels_of_the_prestep_kernel():
  """One definition of the feature row and of the distance: at the fixed point, ms_kmeans_labels with the fitted centres gives the
  fit's labels -- bit-level agreement, no gap needed."""
  from mix_stage_amd.prestep import DevicePreStep
  seed, B, T, M, feats = CASES['m8_512']
  pose, f, init, ref = _reference('m8_512')
  x = torch.tensor(pose, device=DEV)
  res = _fitter(M, feats).fit([x], init)
  zeros, ones = np.zeros(104), np.ones(104)
  pre = DevicePreStep(res.centers, zeros, ones, zeros, ones, device=DEV, feats=FEAT_NAMES[feats])
  _, labels, _ = pre(x, torch.zeros(B, T, 104, device=DEV))
  assert torch.equal(labels, res.labels[0])


def test_three_unequal_chunks_against_one_chunk():
  seed, B, T, M, feats = CASES['m8_512']
  pose, f, init, ref = _reference('m8_512')
  x = torch.tensor(pose, device=DEV)
  chunks = [x[:2], x[2:7], x[7:]]
  km = _fitter(M, feats)
  res3 = km.fit(lambda: iter(chunks), init)
  assert [tuple(l.shape) for l in res3.labels] == [(2, T), (5, T), (1, T)]
  _compare(res3, f, ref, init, 'three chunks')
  res1 = km.fit([x], init)
  assert torch.equal(torch.cat(res3.labels), res1.labels[0]) and torch.equal(res3.counts, res1.counts)
  # the same chunking again: the same bits
  again = km.fit(chunks, init)
  assert torch.equal(again.centers, res3.centers) and again.inertia == res3.inertia


def test_a_far_centre_stays_empty_and_keeps_its_centre():
  seed, B, T, M, feats = CASES['feats7']
  pose, f, _, _ = _reference('feats7')
  init = np.concatenate([R.draw_init(f, 2, 5), np.full((1, f.shape[1]), 1.0e3)])
  ref = R.lloyd(f, init)
  assert ref['empties'] == 1 and ref['counts'][2] == 0
  res = _fitter(3, feats).fit([torch.tensor(pose, device=DEV)], init)
  _compare(res, f, ref, init, 'far centre')
  np.testing.assert_array_equal(res.centers[2].cpu().numpy(), init[2])


def test_n_init_3_picks_the_mirrors_winner():
  seed, B, T, M, feats = CASES['m8_512']
  pose, f, _, _ = _reference('m8_512')
  refs, inits = [], []
  for restart in range(3):
    index = np.sort(np.random.default_rng(40 + restart).choice(len(f), M, replace=False))
    inits.append(f[index])
    refs.append(R.lloyd(f, inits[-1]))
  inertias = sorted(r['inertia'] for r in refs)
  assert inertias[1] - inertias[0] > 1e-9 * inertias[0], 'two restarts of the reference tie: pick another seed'
  win = int(np.argmin([r['inertia'] for r in refs]))
  km = _fitter(M, feats)
  x = torch.tensor(pose, device=DEV)
  np.testing.assert_array_equal(km.feature_rows([x], index).cpu().numpy(), f[index])
  res = km.fit([x], 'rows', n_init=3, seed=40)
  _compare(res, f, refs[win], inits[win], 'n_init=3')
  with pytest.raises(ValueError):
    km.fit([x], inits[0], n_init=3)


def test_max_iter_and_tol_stop_where_the_mirror_stops():
  seed, B, T, M, feats = CASES['m8_512']
  pose, f, init, full = _reference('m8_512')
  assert full['n_iter'] >= 3
  x = torch.tensor(pose, device=DEV)
  for kw in (dict(max_iter=1), dict(max_iter=2), dict(tol=1e30)):
    ref = R.lloyd(f, init, **kw)
    _compare(_fitter(M, feats).fit([x], init, **kw), f, ref, init, str(kw))


def _stats_case(seed, rows, C):
  rng = np.random.default_rng(seed)
  return (rng.normal(0.0, 1.0, size=(rows, C)) * rng.uniform(0.1, 30.0, size=C) + rng.normal(0.0, 100.0, size=C)).astype(np.float32)


def _compare_stats(st, x, tag):
  N = x.shape[0]
  mean, var = R.column_stats(x)
  amax = float(np.abs(x.astype(np.float64)).max())
  assert st.count() == N
  m, v = st.mean().cpu().numpy(), st.var().cpu().numpy()
  assert m.dtype == np.float64 and v.dtype == np.float64
  assert _record('column_mean', np.abs(m - mean), np.full_like(mean, N * U * amax)) <= 1.0, tag
  assert _record('column_var', np.abs(v - var), np.full_like(var, N * U * amax * amax)) <= 1.0, tag


# rows x C: one short slice; one row; 3 slices of 257 (row lanes 256 // 104 = 2); C = 128 (2 lanes); C = 300 (two column blocks,
# the second with 5 lanes of 44); C = 1 (256 lanes)
@pytest.mark.parametrize('rows, C', [(65, 104), (1, 104), (769, 104), (1000, 128), (513, 300), (2049, 1)])
def test_column_stats_equal_the_two_pass_reference(rows, C):
  from mix_stage_amd.fit import DeviceColumnStats
  x = _stats_case(rows + C, rows, C)
  st = DeviceColumnStats(C, DEV).update(torch.from_numpy(x).to(DEV))
  _compare_stats(st, x, 'one chunk')
  if rows >= 3:
    st3 = DeviceColumnStats(C, DEV)
    for part in (x[:rows // 5], x[rows // 5:rows // 5 + 1], x[rows // 5 + 1:]):
      st3.update(torch.from_numpy(part).to(DEV))
    _compare_stats(st3, x, 'three unequal chunks')
  if rows == 1:
    assert torch.equal(st.var(), torch.zeros(C, dtype=torch.float64, device=DEV))


def test_column_stats_with_a_large_offset_keep_the_variance():
  """mean 1e4, spread 1e-2: sum x^2 - (sum x)^2 / N in fp64 would still pass, the fp32 data make the point instead -- the values
  are exact in fp64, the variance comes out to the bar."""
  from mix_stage_amd.fit import DeviceColumnStats
  rng = np.random.default_rng(9)
  x = (1.0e4 + rng.normal(0.0, 1.0e-2, size=(3, 700, 16))).astype(np.float32)
  st = DeviceColumnStats(16, DEV).update(torch.from_numpy(x).to(DEV))          # (..., C): leading indices are rows
  _compare_stats(st, x.reshape(-1, 16), 'offset')
  _, var = R.column_stats(x.reshape(-1, 16))
  assert np.all(np.abs(st.var().cpu().numpy() - var) <= 1e-9 * var)


def test_cpu_tensors_and_wrong_dtypes_raise():
  from mix_stage_amd.fit import DeviceColumnStats
  km = _fitter(3, 3)
  with pytest.raises(TypeError):
    km.fit([torch.zeros(2, 4, 104)], 'rows')
  with pytest.raises(TypeError):
    km.fit([torch.zeros(2, 4, 104, dtype=torch.float64, device=DEV)], 'rows')
  with pytest.raises(TypeError):
    DeviceColumnStats(4, DEV).update(torch.zeros(3, 4))
  with pytest.raises(ValueError):
    km.fit([torch.zeros(2, 4, 100, device=DEV)], 'rows')
  from mix_stage_amd._lib import MixStageLibError
  with pytest.raises(MixStageLibError, match='LDS'):
    _fitter(100, 7)


def _whole(case):
  """A fit and both statistics of a case -> every bit the feature produces, as CPU tensors."""
  from mix_stage_amd.fit import DeviceColumnStats
  seed, B, T, M, feats = CASES[case]
  pose, f, init, ref = _reference(case)
  x = torch.tensor(pose, device=DEV)
  res = _fitter(M, feats).fit([x[:3], x[3:]], init)
  st = DeviceColumnStats(104, DEV).update(x[:3]).update(x[3:])
  return [res.centers.cpu(), torch.tensor(res.inertia, dtype=torch.float64), res.counts.cpu(), torch.cat(res.labels).cpu(), st.state.cpu()]


def test_run_to_run_the_same_bits():
  a, b = _whole('m8_512'), _whole('m8_512')
  for u, v in zip(a, b):
    assert torch.equal(u, v)


@pytest.mark.parametrize('poison', GS.POISONS)
def test_exact_poisoned_scratch(poison, monkeypatch):
  """Every workspace exactly ms_*_workspace bytes, poisoned, between guards: guards intact, results unchanged."""
  from mix_stage_amd import fit as F
  from mix_stage_amd._lib import lib
  plain = _whole('m8_512')
  rec = GS.Scratch(poison)
  sizes = []

  def workspace(nbytes, device):
    sizes.append(int(nbytes))
    return rec.new('workspace', nbytes, device)
  monkeypatch.setattr(F, 'workspace', workspace)
  got = _whole('m8_512')
  torch.cuda.synchronize()
  rec.check()
  for u, v in zip(plain, got):
    assert torch.equal(u, v)
  seed, B, T, M, feats = CASES['m8_512']
  L = lib()
  want = {L.ms_kmeans_fit_workspace(3 * T, PK, M, feats), L.ms_kmeans_fit_workspace((B - 3) * T, PK, M, feats),
          L.ms_column_stats_accumulate_workspace(3 * T, 104), L.ms_column_stats_accumulate_workspace((B - 3) * T, 104)}
  assert set(sizes) == want and 0 not in want
  assert all(hw == 1.0 for _, hw in rec.highwater()), rec.highwater()          # a launch writes every byte it asked for


def test_prestep_fit_save_load_end_to_end(tmp_path):
  from mix_stage_amd.prestep import DevicePreStep
  B, T, M, F_ = 4, 16, 4, 128
  feats = ('pose', 'velocity', 'speed')
  poses = [R.make_pose(31, B, T), R.make_pose(32, B, T)]
  rng = np.random.default_rng(33)
  audios = [(rng.normal(0.0, 2.0, size=(B, T, F_)) - 5.0).astype(np.float32) for _ in range(2)]
  f = np.concatenate([R.feature_rows(p, KEEP, 7) for p in poses])
  index = np.sort(np.random.default_rng(7).choice(len(f), M, replace=False))
  ref = R.lloyd(f, f[index])
  assert ref['min_gap'] > GAP_MIN and R.assign(f, ref['centers'])[2] > GAP_MIN
  pm, pv = R.column_stats(np.concatenate(poses).reshape(-1, 104))
  am, av = R.column_stats(np.concatenate(audios).reshape(-1, F_))
  dp, da = [torch.from_numpy(p).to(DEV) for p in poses], [torch.from_numpy(a).to(DEV) for a in audios]
  fitted = DevicePreStep.fit(dp, da, M, feats=feats, device=DEV, seed=7)
  assert fitted.fit_result.n_iter == ref['n_iter']
  path = str(tmp_path / 'prestep.npz')
  fitted.save(path)
  loaded = DevicePreStep.load(path, DEV)
  assert torch.equal(loaded.centers, fitted.centers) and torch.equal(loaded.pose_inv, fitted.pose_inv)
  mirror = DevicePreStep(ref['centers'], pm, pv, am, av, device=DEV, feats=feats)
  for x, a in zip(dp, da):
    a1, l1, y1 = loaded(x, a)
    a0, l0, y0 = mirror(x, a)
    assert torch.equal(l1, l0)
    for got, want in ((a1, a0), (y1, y0)):
      got, want = got.cpu().numpy(), want.cpu().numpy()
      ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
      assert np.all(np.abs(got - want) <= ulp)
