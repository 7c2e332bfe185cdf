"""CPU checks of the pre-step fitting (mix_stage_amd/fit.py, csrc/prestep_fit.hip): the C-ABI's declarations, the host arithmetic
of the size functions against hand-computed values, every refusal (none of them reaches a launch: no GPU is needed), the NumPy
mirror of tests/helpers/kmeans_ref.py against the installed sklearn, the mirror's own rules, and the .npz container."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import kmeans_ref as R
from mix_stage_amd import _lib
from mix_stage_amd.fit import load_prestep_npz, save_prestep_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ms_kmeans_fit_workspace', 'ms_kmeans_fit_state_elems', 'ms_kmeans_fit_accumulate', 'ms_kmeans_fit_update',
       'ms_column_stats_accumulate', 'ms_column_stats_accumulate_workspace')
FAKE = ctypes.c_void_p(0x1000)          # a non-NULL pointer for calls that must be refused before anything reads it


def _err():
  return _lib.lib().ms_last_error().decode()


def test_symbols_are_declared_in_the_header_and_in_signatures_with_matching_arity():
  header = open(os.path.join(ROOT, 'include', 'mixstage.h')).read()
  for name in NEW:
    m = re.search(r'^(?:int|size_t)\s+%s\s*\(([^;]*)\);' % name, header, re.M)
    assert m, name + ' is not declared in include/mixstage.h'
    assert name in _lib.SIGNATURES, name
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
    assert hasattr(_lib.lib(), name), name
  assert _lib.lib().ms_abi_version() == 4
  srcs = re.search(r'^SRCS = (.*)$', open(os.path.join(ROOT, 'mix_stage_amd', 'csrc', 'Makefile')).read(), re.M).group(1).split()
  assert 'prestep_fit.hip' in srcs


def test_one_definition_of_the_feature_row_and_no_timing_scope():
  csrc = os.path.join(ROOT, 'mix_stage_amd', 'csrc')
  fit, ew = open(os.path.join(csrc, 'prestep_fit.hip')).read(), open(os.path.join(csrc, 'elementwise.hip')).read()
  assert 'TimingScope' not in fit and 'atomicAdd' not in fit
  for src in (fit, ew):
    assert '#include "prestep_feat.h"' in src and 'km_nearest_wave(' in src
    assert 'keep[PK / 2 + d]' not in src                 # the arithmetic lives in the header alone


def test_state_and_workspace_arithmetic_against_hand_computed_values():
  L = _lib.lib()
  # state: sums[M][W] | counts[M] | inertia | changed;  PK = 96: W = 96 | 192 | 240 | 48 for feats 1 | 3 | 7 | 4
  assert L.ms_kmeans_fit_state_elems(96, 8, 7) == 8 * 240 + 8 + 2 == 1930
  assert L.ms_kmeans_fit_state_elems(96, 25, 3) == 25 * 192 + 25 + 2 == 4827
  assert L.ms_kmeans_fit_state_elems(96, 1, 1) == 96 + 1 + 2
  assert L.ms_kmeans_fit_state_elems(96, 3, 4) == 3 * 48 + 3 + 2
  # one record per workgroup; a workgroup takes at least 64 rows, a launch has at most 2048 workgroups
  assert L.ms_kmeans_fit_workspace(1, 96, 8, 7) == 1 * 1930 * 8
  assert L.ms_kmeans_fit_workspace(64, 96, 8, 7) == 1 * 1930 * 8
  assert L.ms_kmeans_fit_workspace(65, 96, 8, 7) == 2 * 1930 * 8 == 30880
  assert L.ms_kmeans_fit_workspace(64 * 1024, 96, 8, 7) == 1024 * 1930 * 8
  assert L.ms_kmeans_fit_workspace(64 * 2048 + 1, 96, 8, 7) == 2048 * 1930 * 8
  assert L.ms_kmeans_fit_workspace(1 << 20, 96, 8, 7) == 2048 * 1930 * 8 == 31621120
  # column statistics: (mean, M2) per column and workgroup; at least 256 rows per workgroup, at most 1024 workgroups
  assert L.ms_column_stats_accumulate_workspace(1, 104) == 1 * 2 * 104 * 8
  assert L.ms_column_stats_accumulate_workspace(1000, 104) == 4 * 2 * 104 * 8 == 6656
  assert L.ms_column_stats_accumulate_workspace(1 << 20, 128) == 1024 * 2 * 128 * 8
  # the largest geometry of the path, M = 25 with all three blocks, fits the 160 KiB of LDS: 25 * 241 doubles = 48200 bytes
  assert L.ms_kmeans_fit_workspace(64, 96, 25, 7) == (25 * 240 + 27) * 8


def _accumulate(pose=FAKE, keep=FAKE, centres=FAKE, labels=FAKE, state=FAKE, ws=FAKE, ws_bytes=1 << 30, B=2, T=8, P=104, PK=96, M=8,
                feats=7):
  return _lib.lib().ms_kmeans_fit_accumulate(pose, keep, centres, labels, state, ws, ws_bytes, B, T, P, PK, M, feats, None)


@pytest.mark.parametrize('which', ['pose', 'keep', 'centres', 'labels', 'state', 'ws'])
def test_accumulate_refuses_a_null_pointer(which):
  assert _accumulate(**{which: None}) != 0
  assert 'null' in _err()


@pytest.mark.parametrize('kw, word', [(dict(feats=0), 'feats'), (dict(feats=8), 'feats'), (dict(feats=-1), 'feats'),
                                      (dict(feats=4, PK=95), 'feats'), (dict(feats=7, PK=95), 'feats'), (dict(M=0), 'M 0'),
                                      (dict(M=-3), 'M -3'), (dict(ws_bytes=2 * 1930 * 8 - 1, B=5, T=13), 'workspace too small'),
                                      (dict(ws_bytes=0), 'workspace too small'), (dict(M=100), 'LDS'), (dict(M=1 << 20), 'LDS'),
                                      (dict(B=0), 'bad argument'), (dict(B=1 << 16, T=1 << 15), 'rows')])
def test_accumulate_refusals_carry_a_message(kw, word):
  assert _accumulate(**kw) != 0
  assert word in _err(), _err()


def test_size_functions_refuse_what_accumulate_refuses():
  L = _lib.lib()
  for args in ((64, 96, 8, 0), (64, 96, 8, 8), (64, 95, 8, 4), (64, 96, 0, 7), (64, 96, 100, 7), (0, 96, 8, 7)):
    assert L.ms_kmeans_fit_workspace(*args) == 0 and _err(), args
  for args in ((96, 8, 0), (95, 8, 5), (96, 0, 3), (96, 100, 7)):
    assert L.ms_kmeans_fit_state_elems(*args) == 0 and _err(), args
  assert L.ms_column_stats_accumulate_workspace(0, 104) == 0 and 'bad argument' in _err()
  assert L.ms_column_stats_accumulate_workspace(10, 0) == 0 and 'bad argument' in _err()


def test_update_and_column_stats_refusals():
  L = _lib.lib()
  for i in range(4):
    ptrs = [FAKE] * 4
    ptrs[i] = None
    assert L.ms_kmeans_fit_update(*ptrs, 8, 240, None) != 0 and 'null' in _err()
  assert L.ms_kmeans_fit_update(FAKE, FAKE, FAKE, FAKE, 0, 240, None) != 0 and 'M 0' in _err()
  assert L.ms_kmeans_fit_update(FAKE, FAKE, FAKE, FAKE, 100, 240, None) != 0 and 'more than' in _err()
  for kw in (dict(x=None), dict(state=None), dict(ws=None)):
    a = dict(x=FAKE, state=FAKE, ws=FAKE)
    a.update(kw)
    assert L.ms_column_stats_accumulate(a['x'], 1000, 104, a['state'], a['ws'], 6656, None) != 0 and 'null' in _err()
  assert L.ms_column_stats_accumulate(FAKE, 1000, 104, FAKE, FAKE, 6655, None) != 0 and 'workspace too small' in _err()
  assert L.ms_column_stats_accumulate(FAKE, 0, 104, FAKE, FAKE, 6656, None) != 0 and 'bad argument' in _err()
  assert L.ms_column_stats_accumulate(FAKE, 1000, 0, FAKE, FAKE, 6656, None) != 0 and 'bad argument' in _err()


# ---- the mirror

def test_feature_row_by_hand():
  keep = np.array([1, 2, 4, 5])                     # PK = 4: x block (1, 2), y block (4, 5)
  pose = np.zeros((1, 3, 6), dtype=np.float32)
  pose[0, :, 1] = [1, 4, 4]
  pose[0, :, 4] = [2, 6, 6]
  pose[0, :, 2] = [0, 0, 5]
  pose[0, :, 5] = [0, 0, 12]
  f = R.feature_rows(pose, keep, 7)
  assert f.shape == (3, 10) == (3, R.feature_width(4, 7))
  np.testing.assert_array_equal(f[0], [1, 0, 2, 0, 0, 0, 0, 0, 0, 0])                 # t == 0: velocity and speed are 0
  np.testing.assert_array_equal(f[1], [4, 0, 6, 0, 3, 0, 4, 0, 5, 0])                 # joint 0 moved by (3, 4): speed 5
  np.testing.assert_array_equal(f[2], [4, 5, 6, 12, 0, 5, 0, 12, 0, 13])              # joint 1 moved by (5, 12): speed 13
  np.testing.assert_array_equal(R.feature_rows(pose, keep, 4), f[:, 8:])
  np.testing.assert_array_equal(R.feature_rows(pose, keep, 5), np.concatenate([f[:, :4], f[:, 8:]], axis=1))
  two = R.feature_rows(np.concatenate([pose, pose]), keep, 2)                          # velocity does not cross clips
  np.testing.assert_array_equal(two[3], np.zeros(4))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_mirror_agrees_with_sklearn_on_separated_data(seed):
  from sklearn.cluster import KMeans
  rng = np.random.default_rng(seed)
  M, W, n = 5, 12, 60
  true = rng.normal(0.0, 10.0, size=(M, W))
  f = np.concatenate([true[m] + rng.normal(0.0, 0.3, size=(n, W)) for m in range(M)])
  f = f[rng.permutation(len(f))]
  init = true + rng.normal(0.0, 1.0, size=(M, W))
  ref = R.lloyd(f, init)
  assert ref['empties'] == 0 and ref['min_gap'] > 1e-3            # no relocation, no near tie: the two definitions coincide
  sk = KMeans(n_clusters=M, init=init, n_init=1, algorithm='lloyd', tol=0, max_iter=300).fit(f)
  np.testing.assert_array_equal(sk.labels_, ref['labels'])
  assert np.all(np.abs(sk.cluster_centers_ - ref['centers']) <= 1e-10 * np.abs(ref['centers']).max())
  assert abs(sk.inertia_ - ref['inertia']) <= 1e-10 * ref['inertia']


def test_mirror_first_minimum_wins_and_an_empty_cluster_keeps_its_centre():
  f = np.array([[0.0], [1.0], [2.0], [10.0]])
  labels, d1, gap = R.assign(f, np.array([[1.0], [1.0], [100.0]]))        # two equal centres: the first one takes every row
  np.testing.assert_array_equal(labels, [0, 0, 0, 0])
  assert gap == 0.0
  new, counts = R.update(f, labels, np.array([[1.0], [1.0], [100.0]]))
  np.testing.assert_array_equal(counts, [4, 0, 0])
  np.testing.assert_array_equal(new, [[13.0 / 4], [1.0], [100.0]])
  ref = R.lloyd(f, np.array([[0.0], [9.0], [1000.0]]))
  np.testing.assert_array_equal(ref['labels'], [0, 0, 0, 1])
  np.testing.assert_array_equal(ref['centers'], [[1.0], [10.0], [1000.0]])
  assert ref['empties'] == 1 and ref['counts'].tolist() == [3, 1, 0] and ref['inertia'] == 2.0


def test_mirror_stopping_rules():
  f = np.array([[0.0], [1.0], [2.0], [10.0], [11.0]])
  init = np.array([[0.0], [1.0]])
  full = R.lloyd(f, init)
  # iteration 1: {0} {1,2,10,11} -> (0, 6); 2: {0,1,2} {10,11} -> (1, 10.5); 3: no label changes
  assert full['n_iter'] == 3 and full['centers'].tolist() == [[1.0], [10.5]]
  assert R.lloyd(f, init, max_iter=1)['n_iter'] == 1 and R.lloyd(f, init, max_iter=1)['centers'].tolist() == [[0.0], [6.0]]
  assert R.lloyd(f, init, max_iter=2)['centers'].tolist() == [[1.0], [10.5]]
  # squared shift of iteration 2 is 1 + 4.5^2 = 21.25: a tol at that value stops there, a smaller one goes on
  assert R.lloyd(f, init, tol=21.25)['n_iter'] == 2 and R.lloyd(f, init, tol=21.0)['n_iter'] == 3
  assert R.lloyd(f, init, tol=1e9)['n_iter'] == 1
  # started at the fixed point: the first iteration changes every label from -1 but moves no centre (shift 0 <= tol 0)
  assert R.lloyd(f, full['centers'])['n_iter'] == 1


def test_mirror_column_stats_by_hand():
  mean, var = R.column_stats(np.array([[1.0, 1e8 + 1], [3.0, 1e8 + 3], [5.0, 1e8 + 5]]))
  np.testing.assert_array_equal(mean, [3.0, 1e8 + 3])
  np.testing.assert_array_equal(var, [8.0 / 3, 8.0 / 3])


def test_npz_round_trip_of_the_statistics_container(tmp_path):
  rng = np.random.default_rng(3)
  given = dict(centers=rng.normal(size=(8, 240)), pose_mean=rng.normal(size=104), pose_var=rng.random(104), audio_mean=rng.normal(size=128),
               audio_var=rng.random(128), mask=(0, 7, 8, 9), num_feats=104, eps=1e-8, feats=('pose', 'velocity', 'speed'))
  path = str(tmp_path / 'prestep.npz')
  save_prestep_npz(path, **given)
  back = load_prestep_npz(path)
  assert set(back) == set(given)
  for k in ('centers', 'pose_mean', 'pose_var', 'audio_mean', 'audio_var'):
    assert back[k].dtype == np.float64
    np.testing.assert_array_equal(back[k], given[k])
  assert back['mask'] == (0, 7, 8, 9) and back['feats'] == ('pose', 'velocity', 'speed') and back['num_feats'] == 104 and back['eps'] == 1e-8
  with np.load(path, allow_pickle=False) as z:                        # a plain archive: nothing pickled
    assert sorted(z.files) == sorted(given)


def test_prestep_object_round_trip_on_the_host(tmp_path):
  """DevicePreStep.save / load keep the arguments as given (construction alone needs no GPU; calling it does)."""
  import torch
  from mix_stage_amd.prestep import DevicePreStep
  rng = np.random.default_rng(4)
  a = DevicePreStep(rng.normal(size=(3, 192)), rng.normal(size=104), rng.random(104), rng.normal(size=128), rng.random(128), device='cpu')
  path = str(tmp_path / 'p.npz')
  a.save(path)
  b = DevicePreStep.load(path, device='cpu')
  for k in ('centers', 'pose_mean', 'pose_inv', 'audio_mean', 'audio_inv', 'keep'):
    assert torch.equal(getattr(a, k), getattr(b, k)), k
  assert (a.feats, a.M, a.P, a.PK) == (b.feats, b.M, b.P, b.PK)
  with pytest.raises(TypeError):
    b(torch.zeros(1, 2, 104), torch.zeros(1, 2, 128))
