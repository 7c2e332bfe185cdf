"""Per-step pre-processing in front of the GAN path, on the MI355X ("next" row N1 of SURVEY.md section 8f).

Reference: TrainerLateClusterGAN.get_processed_batch (src/model/trainer.py:1290-1308) runs, on the CPU in float64 every
step: KMeans.predict on RemoveJoints(pose) -> cluster labels (src/data/transform.py:352-410), ZNorm of audio and pose
(transform.py:221-226), RemoveJoints of the normalised pose (transform.py:481-507), then copies everything to the
device.  Here the raw batch is copied once and the three transforms are two HIP kernels (fp64 arithmetic inside, like
the reference; fp32 tensors out for the fp32 model).  RemoveJoints follows the inferred `remove_slices` semantics (pycasper
is not in the reference tree).

The k-means centres and the mean / variance vectors are either handed in (the reference commits them as HDF5 files; reading
those stays with the caller) or fitted here on the device: DevicePreStep.fit runs the Lloyd iterations and the statistics
pass of fit.py (KMeans / ZNorm of transform.py:99-244,247-427, sklearn on the CPU in the reference) over the caller's batches,
and save / load keep a fitted pre-step in a plain .npz.
"""
import ctypes

import torch

from ._lib import check, lib

_vp = ctypes.c_void_p


def _p(t):
  return None if t is None else _vp(t.data_ptr())


FEAT_BITS = {'pose': 1, 'velocity': 2, 'speed': 4}


def feature_geometry(mask, num_feats, feats):
  """-> (keep: the surviving columns, x block then y block; the `feats` bit set of the C-ABI; the width of the feature row)."""
  J = num_feats // 2
  kept = [j for j in range(J) if j not in set(mask)]
  keep = [xy * J + j for xy in range(2) for j in kept]
  PK = len(keep)
  feats = tuple(feats)
  unknown = [f for f in feats if f not in FEAT_BITS]
  if unknown or list(feats) != [f for f in ('pose', 'velocity', 'speed') if f in feats]:
    raise ValueError('feats must be a sub-list of [pose, velocity, speed] in that order, got %s' % (feats,))
  bits = sum(FEAT_BITS[f] for f in feats)
  width = sum({'pose': PK, 'velocity': PK, 'speed': PK // 2}[f] for f in feats)
  return keep, bits, width


class DevicePreStep:
  FEAT_BITS = FEAT_BITS

  def __init__(self, centers, pose_mean, pose_var, audio_mean, audio_var, mask=(0, 7, 8, 9), num_feats=104, eps=1e-8,
               device='cuda:0', feats=('pose', 'velocity')):
    """feats: the k-means feature blocks (KMeans.get_feats, transform.py:352-378): argsUtils' default is
    ['pose', 'velocity']; the Mix-StAGE job scripts (src/jobs/mix-stage.py) train with ['pose', 'velocity', 'speed'].
    'acceleration' and 'spatial' are not offered."""
    dev = torch.device(device)
    keep, self.feats, width = feature_geometry(mask, num_feats, feats)
    feats = tuple(feats)
    self.P, self.PK = num_feats, len(keep)
    self.keep = torch.tensor(keep, dtype=torch.int32, device=dev)
    centers = torch.as_tensor(centers, dtype=torch.float64)
    if centers.shape[1] != width:
      raise ValueError('centres must have %d columns (%s of the kept joints), got %d' % (width, ' | '.join(feats), centers.shape[1]))
    self.M = centers.shape[0]
    self.centers = centers.contiguous().to(dev)

    def prep(mean, var):
      mean = torch.as_tensor(mean, dtype=torch.float64).reshape(-1)
      var = torch.as_tensor(var, dtype=torch.float64).reshape(-1)
      std = (var * (var >= 0)).sqrt()
      std = torch.where(std == 0, torch.full_like(std, eps), std)      # transform.py:222-225
      return mean.to(dev), (1.0 / std).to(dev)
    pose_mean, pose_var, audio_mean, audio_var = (torch.as_tensor(v, dtype=torch.float64).reshape(-1).cpu().clone()
                                                  for v in (pose_mean, pose_var, audio_mean, audio_var))
    self.pose_mean, self.pose_inv = prep(pose_mean, pose_var)
    self.audio_mean, self.audio_inv = prep(audio_mean, audio_var)
    self.dev = dev
    # what save() writes: the arguments as given (fp64), not the reciprocals derived from them
    self._saved = dict(centers=centers, pose_mean=pose_mean, pose_var=pose_var, audio_mean=audio_mean, audio_var=audio_var,
                       mask=tuple(int(j) for j in mask), num_feats=int(num_feats), eps=float(eps), feats=feats)

  @classmethod
  def fit(cls, pose_batches, audio_batches, num_clusters, mask=(0, 7, 8, 9), num_feats=104, eps=1e-8, device='cuda:0',
          feats=('pose', 'velocity'), init='rows', max_iter=300, tol=0.0, n_init=1, seed=0):
    """Fit the centres (DeviceKMeansFit on the raw pose) and the four statistics vectors (DeviceColumnStats, population
    variance) on the device and return the DevicePreStep that uses them.  pose_batches / audio_batches: lists of fp32 device
    tensors (B,T,P) / (B,T,F), or callables that return a fresh iterator over them."""
    from .fit import DeviceColumnStats, DeviceKMeansFit, walk
    km = DeviceKMeansFit(num_clusters, mask=mask, num_feats=num_feats, feats=feats, device=device)
    res = km.fit(pose_batches, init, max_iter=max_iter, tol=tol, n_init=n_init, seed=seed)
    pose_stats, audio_stats = DeviceColumnStats(num_feats, device), None
    for x in walk(pose_batches):
      pose_stats.update(x)
    for a in walk(audio_batches):
      if audio_stats is None:
        audio_stats = DeviceColumnStats(a.shape[-1], device)
      audio_stats.update(a)
    if audio_stats is None:
      raise ValueError('DevicePreStep.fit: no audio batches')
    self = cls(res.centers, pose_stats.mean(), pose_stats.var(), audio_stats.mean(), audio_stats.var(), mask=mask,
               num_feats=num_feats, eps=eps, device=device, feats=feats)
    self.fit_result = res
    return self

  def save(self, path):
    """Centres, the four statistics vectors, mask, feats and eps as a plain .npz (fp64 stays fp64)."""
    from .fit import save_prestep_npz
    save_prestep_npz(path, **self._saved)

  @classmethod
  def load(cls, path, device='cuda:0'):
    from .fit import load_prestep_npz
    return cls(device=device, **load_prestep_npz(path))

  def __call__(self, pose_raw, audio_raw):
    """pose_raw (B,T,P) and audio_raw (B,T,F) fp32 on the device -> (audio_norm (B,T,F), labels (B,T) int64,
    y (B,T,P-2*len(mask))) as the reference hands them to the model."""
    if not (pose_raw.is_cuda and audio_raw.is_cuda) or pose_raw.dtype != torch.float32 or audio_raw.dtype != torch.float32:
      raise TypeError('DevicePreStep takes float32 tensors on the MI355X')
    pose_raw, audio_raw = pose_raw.contiguous(), audio_raw.contiguous()
    B, T, P = pose_raw.shape
    F_ = audio_raw.shape[-1]
    assert P == self.P and audio_raw.shape[:2] == (B, T) and F_ == self.audio_mean.numel()
    s = _vp(torch.cuda.current_stream().cuda_stream)
    labels = torch.empty((B, T), dtype=torch.int64, device=self.dev)
    check(lib().ms_kmeans_labels(_p(pose_raw), _p(self.keep), _p(self.centers), _p(labels), B, T, P, self.PK, self.M, self.feats, s),
          'ms_kmeans_labels')
    y = torch.empty((B, T, self.PK), dtype=torch.float32, device=self.dev)
    check(lib().ms_znorm_select(_p(pose_raw), _p(self.keep), _p(self.pose_mean), _p(self.pose_inv), _p(y), B * T, P, self.PK, s),
          'ms_znorm_select')
    a = torch.empty_like(audio_raw)
    check(lib().ms_znorm_select(_p(audio_raw), None, _p(self.audio_mean), _p(self.audio_inv), _p(a), B * T, F_, F_, s),
          'ms_znorm_select')
    return a, labels, y
