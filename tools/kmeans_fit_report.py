"""One Lloyd iteration of the device k-means fit at a PATS-like size, for orientation (no bar): profiles/kmeans_fit.json.

  python tools/kmeans_fit_report.py [--rows-log2 20] [--out profiles/kmeans_fit.json] [--ratios FILE]

Times ms_kmeans_fit_accumulate + ms_kmeans_fit_update (M = 8, feats = pose|velocity|speed) and ms_column_stats_accumulate on
2^20 rows of 104 fp32 with HIP events, and reports them beside (a) the time reading rows * P * 4 bytes once would take at the
HBM rate measured on this chip (6.29 TB/s float4 copy; 8.0 TB/s on paper) and (b) sklearn's Lloyd iteration on this host's CPU
threads (fit with max_iter = 3 minus fit with max_iter = 1, halved; float64 feature rows built beforehand).  --ratios merges the
worst value / bar figures that tests/test_gpu_prestep_fit.py collects in its WORST table (a JSON file of that dict)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def _median_ms(fn, warm=3, reps=15):
  for _ in range(warm):
    fn()
  torch.cuda.synchronize()
  out = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    out.append(a.elapsed_time(b))
  return dict(median=float(np.median(out)), min=float(min(out)), max=float(max(out)), reps=reps)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rows-log2', type=int, default=20)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmeans_fit.json'))
  ap.add_argument('--ratios', default=None)
  ap.add_argument('--no-sklearn', action='store_true')
  a = ap.parse_args()
  from helpers import kmeans_ref as R
  from mix_stage_amd._lib import check, lib
  from mix_stage_amd.fit import DeviceColumnStats, DeviceKMeansFit

  assert torch.cuda.is_available(), 'needs the MI355X'
  dev, M, T, P = 'cuda:0', 8, 64, 104
  rows = 1 << a.rows_log2
  B = rows // T
  feats = ('pose', 'velocity', 'speed')
  g = torch.Generator(device=dev).manual_seed(0)
  proto = torch.randn(M, 1, P, device=dev, generator=g)
  x = (proto[torch.randint(0, M, (B,), device=dev, generator=g)] +
       torch.cumsum(0.05 * torch.randn(B, T, P, device=dev, generator=g), dim=1)).contiguous()
  km = DeviceKMeansFit(M, feats=feats, device=dev)
  index = np.sort(np.random.default_rng(0).choice(rows, M, replace=False))
  centres = km.feature_rows([x], index).contiguous()
  L, vp = lib(), ctypes.c_void_p
  labels = torch.full((B, T), -1, dtype=torch.int64, device=dev)
  state = torch.zeros(km.state_elems, dtype=torch.float64, device=dev)
  ws = torch.empty(L.ms_kmeans_fit_workspace(rows, km.PK, M, km.feats), dtype=torch.uint8, device=dev)
  c_out, out4 = torch.empty_like(centres), torch.empty(4, dtype=torch.float64, device=dev)
  s = vp(torch.cuda.current_stream().cuda_stream)

  def iteration():
    state.zero_()
    check(L.ms_kmeans_fit_accumulate(vp(x.data_ptr()), vp(km.keep.data_ptr()), vp(centres.data_ptr()), vp(labels.data_ptr()),
                                     vp(state.data_ptr()), vp(ws.data_ptr()), ws.numel(), B, T, P, km.PK, M, km.feats, s), 'accumulate')
    check(L.ms_kmeans_fit_update(vp(state.data_ptr()), vp(centres.data_ptr()), vp(c_out.data_ptr()), vp(out4.data_ptr()), M, km.W, s), 'update')

  lloyd = _median_ms(iteration)
  stats = DeviceColumnStats(P, dev)
  col = _median_ms(lambda: stats.update(x))
  nbytes = rows * P * 4
  report = dict(
      what='one Lloyd iteration (ms_kmeans_fit_accumulate + ms_kmeans_fit_update) and one ms_column_stats_accumulate pass; HIP events, '
           'median of %d behind 3; for orientation, no bar' % lloyd['reps'],
      shape=dict(rows=rows, B=B, T=T, P=P, PK=km.PK, M=M, feats=km.feats, W=km.W),
      device_lloyd_iteration_ms=lloyd, device_column_stats_ms=col,
      hbm_read_once=dict(bytes=nbytes, ms_at_6p29_TBps_measured=nbytes / HBM_MEASURED * 1e3, ms_at_8_TBps_spec=nbytes / HBM_SPEC * 1e3),
      lloyd_over_hbm_read=lloyd['median'] / (nbytes / HBM_MEASURED * 1e3))
  if not a.no_sklearn:
    import sklearn
    from sklearn.cluster import KMeans
    f = R.feature_rows(x.cpu().numpy(), R.keep_columns(), km.feats)
    init = centres.cpu().numpy()

    def fit(n):
      t0 = time.perf_counter()
      KMeans(n_clusters=M, init=init, n_init=1, algorithm='lloyd', tol=0, max_iter=n).fit(f)
      return time.perf_counter() - t0
    fit(1)
    t1, t3 = min(fit(1), fit(1)), min(fit(3), fit(3))
    report['sklearn_lloyd_iteration'] = dict(ms=(t3 - t1) / 2 * 1e3, fit_max_iter_1_ms=t1 * 1e3, fit_max_iter_3_ms=t3 * 1e3,
                                             threads=int(os.environ.get('OMP_NUM_THREADS', 0)) or os.cpu_count(),
                                             sklearn=sklearn.__version__, dtype='float64 feature rows (rows x %d)' % km.W)
    report['sklearn_over_device'] = report['sklearn_lloyd_iteration']['ms'] / lloyd['median']
  if a.ratios:
    report['test_worst_value_over_bar'] = json.load(open(a.ratios))
  with open(a.out, 'w') as fh:
    json.dump(report, fh, indent=1)
    fh.write('\n')
  print(json.dumps(report))


if __name__ == '__main__':
  main()
