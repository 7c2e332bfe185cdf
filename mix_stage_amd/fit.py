"""Fitting what the pre-step consumes, on the MI355X: the k-means centres and the ZNorm statistics.

Reference: KMeans and ZNorm of src/data/transform.py:247-427 and :99-244 fit once per speaker set with sklearn / NumPy on the
CPU and commit the results as HDF5 files.  Here one Lloyd iteration is one pass of ms_kmeans_fit_accumulate over the caller's
batches (the feature row, the distance arithmetic and the first-minimum rule of ms_kmeans_labels; per-cluster sums in fp64, in a
fixed order) followed by ms_kmeans_fit_update; the statistics pass is ms_column_stats_accumulate (two-pass moments per slice of
rows, joined with Chan's update).  The same batches in the same chunking give the same bits, run after run.

PARITY UNPINNED against sklearn: an empty cluster keeps its centre (sklearn relocates it to a far point), and the seeding is
either an array the caller hands in or distinct rows drawn uniformly -- k-means++ seeding is out of scope.
"""
import collections
import ctypes

import numpy as np
import torch

from ._lib import check, lib
from .prestep import feature_geometry

_vp = ctypes.c_void_p

KMeansFitResult = collections.namedtuple('KMeansFitResult', 'centers inertia n_iter counts labels')


def _p(t):
  return _vp(t.data_ptr())


def _stream():
  return _vp(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, device):
  """Scratch for one call, exactly as large as the library's size function says; its contents on entry do not matter."""
  return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def walk(batches):
  """One pass over `batches`: a list of tensors, or a callable that returns a fresh iterator over them."""
  return iter(batches()) if callable(batches) else iter(batches)


def _device_f32(x, what):
  if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
    raise TypeError('%s takes float32 tensors on the MI355X' % what)
  return x.contiguous()


class DeviceColumnStats:
  """Running per-column (count, mean, M2) in fp64 over everything `update` has seen (ZNorm's statistics pass)."""

  def __init__(self, C, device='cuda:0'):
    self.C, self.dev = int(C), torch.device(device)
    self.state = torch.zeros(3 * self.C, dtype=torch.float64, device=self.dev)

  def update(self, x):
    """x (..., C) fp32 on the device: every leading index is a row."""
    x = _device_f32(x, 'DeviceColumnStats.update')
    if x.shape[-1] != self.C:
      raise ValueError('DeviceColumnStats(%d) got %d columns' % (self.C, x.shape[-1]))
    rows = x.numel() // self.C
    if rows == 0:
      return self
    nbytes = lib().ms_column_stats_accumulate_workspace(rows, self.C)
    if nbytes == 0:
      check(1, 'ms_column_stats_accumulate_workspace')
    ws = workspace(nbytes, self.dev)
    check(lib().ms_column_stats_accumulate(_p(x), rows, self.C, _p(self.state), _p(ws), ws.numel(), _stream()), 'ms_column_stats_accumulate')
    return self

  def count(self):
    return int(self.state[0].item())

  def mean(self):
    return self.state[self.C:2 * self.C].clone()

  def var(self, ddof=0):
    return self.state[2 * self.C:] / (self.state[:self.C] - ddof)


class DeviceKMeansFit:
  """Lloyd's k-means on the pre-step's feature row (KMeans.get_feats, transform.py:352-378) of RemoveJoints(pose).

  k-means++ seeding is out of scope: `init` is an (M, W) array or 'rows' (M distinct rows of the data, drawn uniformly)."""

  def __init__(self, num_clusters, mask=(0, 7, 8, 9), num_feats=104, feats=('pose', 'velocity'), device='cuda:0'):
    self.dev = torch.device(device)
    keep, self.feats, self.W = feature_geometry(mask, num_feats, feats)
    self.M, self.P, self.PK = int(num_clusters), int(num_feats), len(keep)
    self.keep = torch.tensor(keep, dtype=torch.int32, device=self.dev)
    self.state_elems = lib().ms_kmeans_fit_state_elems(self.PK, self.M, self.feats)
    if self.state_elems == 0:
      check(1, 'ms_kmeans_fit_state_elems')

  def _check(self, x):
    x = _device_f32(x, 'DeviceKMeansFit.fit')
    if x.dim() != 3 or x.shape[-1] != self.P:
      raise ValueError('pose batches are (B, T, %d), got %s' % (self.P, tuple(x.shape)))
    return x

  def feature_rows(self, batches, index):
    """The feature rows (len(index), W) fp64 of the rows `index` (sorted, into the concatenation of all (b, t) of `batches`)."""
    keep = self.keep.long()
    out, first = [], 0
    index = np.asarray(index, dtype=np.int64)
    for x in walk(batches):
      x = self._check(x)
      B, T, _ = x.shape
      sel = index[(index >= first) & (index < first + B * T)] - first
      first += B * T
      if sel.size == 0:
        continue
      r = torch.as_tensor(sel, device=self.dev)
      flat = x.reshape(B * T, self.P).double()
      cur = flat[r][:, keep]
      prev = flat[(r - 1).clamp(min=0)][:, keep]
      vel = torch.where((r % T > 0)[:, None], cur - prev, torch.zeros_like(cur))
      blocks = []
      if self.feats & 1:
        blocks.append(cur)
      if self.feats & 2:
        blocks.append(vel)
      if self.feats & 4:
        h = self.PK // 2
        blocks.append((vel[:, :h] * vel[:, :h] + vel[:, h:] * vel[:, h:]).sqrt())
      out.append(torch.cat(blocks, dim=1))
    return torch.cat(out, dim=0)

  def _lloyd(self, batches, centres, max_iter, tol):
    L = lib()
    M, W = self.M, self.W
    state = torch.empty(self.state_elems, dtype=torch.float64, device=self.dev)
    out4 = torch.empty(4, dtype=torch.float64, device=self.dev)
    c_in, c_out = centres.clone(), torch.empty_like(centres)
    labels, inertia, n_iter = [], float('nan'), 0
    for it in range(max_iter):
      state.zero_()
      for k, x in enumerate(walk(batches)):
        x = self._check(x)
        B, T, _ = x.shape
        if it == 0:
          labels.append(torch.full((B, T), -1, dtype=torch.int64, device=self.dev))
        if k >= len(labels) or labels[k].shape != (B, T):
          raise ValueError('DeviceKMeansFit.fit: every pass over `batches` must yield the same batches')
        nbytes = L.ms_kmeans_fit_workspace(B * T, self.PK, M, self.feats)
        if nbytes == 0:
          check(1, 'ms_kmeans_fit_workspace')
        ws = workspace(nbytes, self.dev)
        check(L.ms_kmeans_fit_accumulate(_p(x), _p(self.keep), _p(c_in), _p(labels[k]), _p(state), _p(ws), ws.numel(), B, T, self.P,
                                         self.PK, M, self.feats, _stream()), 'ms_kmeans_fit_accumulate')
      if not labels:
        raise ValueError('DeviceKMeansFit.fit: no batches')
      check(L.ms_kmeans_fit_update(_p(state), _p(c_in), _p(c_out), _p(out4), M, W, _stream()), 'ms_kmeans_fit_update')
      shift, _empties, inertia, changed = out4.tolist()          # the iteration's one device-to-host read
      c_in, c_out = c_out, c_in
      n_iter = it + 1
      if changed == 0 or shift <= tol:
        break
    counts = state[M * W:M * W + M].to(torch.int64)
    return KMeansFitResult(c_in, inertia, n_iter, counts, labels)

  def fit(self, batches, init='rows', max_iter=300, tol=0.0, n_init=1, seed=0):
    """batches: a list of fp32 device tensors (B, T, P), or a callable that returns a fresh iterator over them; every Lloyd
    iteration walks it once.  init: an (M, W) array, or 'rows': M distinct feature rows drawn with
    numpy.random.default_rng(seed + restart).choice(N, M, replace=False) (k-means++ seeding is out of scope).  An iteration
    assigns every row to its nearest centre (first minimum wins) and moves each centre to the mean of its rows; a cluster
    without rows keeps its centre.  Iteration stops when no label changed, when the squared centre shift is at most `tol`, or at
    `max_iter`.  n_init > 1 ('rows' only) keeps the restart with the lowest inertia.

    -> KMeansFitResult(centers (M, W) fp64 on the device, inertia, n_iter, counts (M,) int64, labels [(B, T) int64 per batch]);
    inertia, counts and labels are those of the last assignment (against the centres before the last update: the same centres
    when the iteration stopped because no label changed)."""
    if max_iter < 1 or n_init < 1:
      raise ValueError('max_iter and n_init must be at least 1')
    if isinstance(init, str):
      if init != 'rows':
        raise ValueError("init must be an (M, W) array or 'rows'")
      N = sum(self._check(x).shape[0] * x.shape[1] for x in walk(batches))
      if N < self.M:
        raise ValueError('%d rows cannot seed %d clusters' % (N, self.M))
      best = None
      for restart in range(n_init):
        index = np.sort(np.random.default_rng(seed + restart).choice(N, self.M, replace=False))
        res = self._lloyd(batches, self.feature_rows(batches, index).contiguous(), max_iter, tol)
        if best is None or res.inertia < best.inertia:
          best = res
      return best
    if n_init != 1:
      raise ValueError('n_init > 1 needs init=\'rows\': an explicit array gives the same fit every time')
    if not isinstance(init, torch.Tensor):
      init = np.array(init, dtype=np.float64)          # (a copy: the caller's array may be read-only)
    centres = torch.as_tensor(init, dtype=torch.float64).to(self.dev).contiguous()
    if tuple(centres.shape) != (self.M, self.W):
      raise ValueError('init must be (%d, %d), got %s' % (self.M, self.W, tuple(centres.shape)))
    return self._lloyd(batches, centres, max_iter, tol)


def save_prestep_npz(path, centers, pose_mean, pose_var, audio_mean, audio_var, mask, num_feats, eps, feats):
  """The container of a fitted pre-step: a plain .npz (no HDF5), fp64 arrays as they are."""
  def arr(v):
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)
  with open(path, 'wb') as f:
    np.savez(f, centers=arr(centers), pose_mean=arr(pose_mean), pose_var=arr(pose_var), audio_mean=arr(audio_mean),
             audio_var=arr(audio_var), mask=np.asarray(mask, dtype=np.int64), num_feats=np.int64(num_feats), eps=np.float64(eps),
             feats=np.asarray(list(feats), dtype='U16'))


def load_prestep_npz(path):
  """-> the keyword arguments of DevicePreStep (all but the device)."""
  with np.load(path, allow_pickle=False) as z:
    return dict(centers=z['centers'], pose_mean=z['pose_mean'], pose_var=z['pose_var'], audio_mean=z['audio_mean'],
                audio_var=z['audio_var'], mask=tuple(int(j) for j in z['mask']), num_feats=int(z['num_feats']), eps=float(z['eps']),
                feats=tuple(str(f) for f in z['feats']))
