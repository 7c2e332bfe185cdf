"""bench.py's command line and output dump, without a GPU: a plain run measures the headline only, --full adds the rest, and
--dump-outputs writes float32 / float64 .npy files at the same sample positions in every run, under the size limit."""
import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
  monkeypatch.setattr(sys, 'argv', ['bench.py'] + list(argv))
  return bench.parse()


def test_plain_run_is_headline_only_and_full_is_opt_in(monkeypatch):
  a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
  assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
  a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2', '--full', '--dump-outputs', 'out')
  assert a.full and a.dump_outputs == 'out'


def test_fixed_sample_is_the_same_every_run():
  n = bench.DUMP_SAMPLE * 3 + 5
  a, b = bench._fixed_sample(n), bench._fixed_sample(n)
  assert np.array_equal(a, b) and len(a) == bench.DUMP_SAMPLE
  assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < n
  assert bench._fixed_sample(bench.DUMP_SAMPLE) is None         # small arrays are written whole


def test_save_outputs_dtypes_and_limit(tmp_path):
  bench.save_outputs(str(tmp_path), [('a', torch.ones(3, dtype=torch.bfloat16)), ('b', torch.zeros(2, dtype=torch.float64)),
                                     ('c', np.arange(4, dtype=np.int64))])
  assert np.load(tmp_path / 'a.npy').dtype == np.float32
  assert np.load(tmp_path / 'b.npy').dtype == np.float64
  assert np.load(tmp_path / 'c.npy').dtype == np.float32
  with pytest.raises(SystemExit):
    bench.save_outputs(str(tmp_path / 'big'), [('x', np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, dtype=np.float32))])
  assert not (tmp_path / 'big' / 'x.npy').exists()
