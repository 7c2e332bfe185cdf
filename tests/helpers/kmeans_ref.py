"""NumPy float64 references of the pre-step fitting (mix_stage_amd/fit.py, csrc/prestep_fit.hip).

  feature_rows   the feature row of KMeans.get_feats (transform.py:352-378) as ms_kmeans_labels builds it:
                 pose[keep] | velocity | speed, chosen by feats & 1 | 2 | 4; velocity 0 at t == 0 of each clip; speed pairs kept
                 column d with kept column PK/2 + d
  lloyd          deterministic Lloyd: first minimum wins, an empty cluster keeps its centre, stop when no label changed, when
                 the squared centre shift is at most tol, or at max_iter.  Also returns the smallest relative gap
                 (d2 - d1) / d2 between the best and the second-best squared distance over all rows and iterations: where
                 that gap is far above the rounding error of a distance, every correct implementation finds the same labels
  column_stats   two-pass per-column mean and variance

Everything in float64.  The bars of the GPU tests hold for any order of the fp64 additions on either side."""
import numpy as np


def keep_columns(mask=(0, 7, 8, 9), num_feats=104):
  J = num_feats // 2
  kept = [j for j in range(J) if j not in set(mask)]
  return np.array([xy * J + j for xy in range(2) for j in kept], dtype=np.int64)


def feature_width(PK, feats):
  return (PK if feats & 1 else 0) + (PK if feats & 2 else 0) + (PK // 2 if feats & 4 else 0)


def feature_rows(pose, keep, feats):
  """pose (B, T, P) float32 -> (B*T, W) float64."""
  assert 1 <= feats <= 7
  x = np.asarray(pose, dtype=np.float64)[:, :, keep]
  B, T, PK = x.shape
  v = np.zeros_like(x)
  v[:, 1:] = x[:, 1:] - x[:, :-1]
  blocks = []
  if feats & 1:
    blocks.append(x)
  if feats & 2:
    blocks.append(v)
  if feats & 4:
    assert PK % 2 == 0
    h = PK // 2
    blocks.append(np.sqrt(v[..., :h] * v[..., :h] + v[..., h:] * v[..., h:]))
  return np.concatenate(blocks, axis=-1).reshape(B * T, -1)


def assign(f, centres):
  """-> (labels: first minimum wins, the squared distance to that centre per row, the smallest relative gap (d2 - d1) / d2)."""
  d = ((f[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)           # (N, M)
  labels = d.argmin(axis=1)                                              # numpy: the first of equal minima
  d1 = d[np.arange(len(f)), labels]
  if centres.shape[0] > 1:
    rest = d.copy()
    rest[np.arange(len(f)), labels] = np.inf
    d2 = rest.min(axis=1)
    gap = float(np.min(np.where(d2 > 0, (d2 - d1) / np.where(d2 > 0, d2, 1.0), 0.0)))
  else:
    gap = 1.0
  return labels, d1, gap


def update(f, labels, centres):
  """-> (new centres: the mean of each cluster's rows, an empty cluster keeps its centre; counts)."""
  M = centres.shape[0]
  out = centres.copy()
  counts = np.bincount(labels, minlength=M)
  for m in range(M):
    if counts[m]:
      out[m] = f[labels == m].sum(axis=0) / counts[m]
  return out, counts


def lloyd(f, init, max_iter=300, tol=0.0):
  """f (N, W) float64, init (M, W) -> dict(centers, inertia, n_iter, counts, labels, min_gap, empties, last_counts); inertia,
  counts and labels are those of the last assignment, like DeviceKMeansFit.  last_counts[m]: the number of rows behind
  centers[m] -- counts[m], or for a cluster that ended empty the count it had when its centre was last computed (0: never, the
  centre is the initial one)."""
  c = np.array(init, dtype=np.float64)
  last_counts = np.zeros(c.shape[0], dtype=np.int64)
  prev = np.full(len(f), -1, dtype=np.int64)
  min_gap = np.inf
  for it in range(max_iter):
    labels, d1, gap = assign(f, c)
    min_gap = min(min_gap, gap)
    new, counts = update(f, labels, c)
    last_counts = np.where(counts > 0, counts, last_counts)
    shift = float(((new - c) ** 2).sum())
    changed = int((labels != prev).sum())
    c, prev = new, labels
    if changed == 0 or shift <= tol:
      break
  return dict(centers=c, inertia=float(d1.sum()), n_iter=it + 1, counts=counts, labels=labels, min_gap=float(min_gap),
              empties=int((counts == 0).sum()), last_counts=last_counts)


def column_stats(x):
  """x (N, C) -> (mean, population variance) per column, two-pass in float64."""
  x = np.asarray(x, dtype=np.float64)
  mean = x.sum(axis=0) / x.shape[0]
  d = x - mean
  return mean, (d * d).sum(axis=0) / x.shape[0]


def make_pose(seed, B, T, P=104, n_proto=4, walk=0.05, noise=0.02):
  """A few pose prototypes + a cumulative random walk + noise, as float32 (B, T, P): clips cluster around their prototype and
  move, so that the pose, velocity and speed blocks all carry structure."""
  rng = np.random.default_rng(seed)
  protos = rng.normal(0.0, 1.0, size=(n_proto, P))
  which = rng.integers(0, n_proto, size=B)
  steps = rng.normal(0.0, walk, size=(B, T, P)) * (1.0 + which[:, None, None])       # prototypes move at different speeds
  x = protos[which][:, None, :] + np.cumsum(steps, axis=1) + rng.normal(0.0, noise, size=(B, T, P))
  return x.astype(np.float32)


def draw_init(f, M, seed, T=None, skip_first_frame=False):
  """M distinct rows of f as initial centres; skip_first_frame: from t > 0 only (rows at t == 0 have an all-zero velocity / speed
  block: with feats that lack the pose block they coincide, and coinciding centres mean exact ties)."""
  rng = np.random.default_rng(seed)
  pool = np.arange(len(f))
  if skip_first_frame:
    pool = pool[pool % T > 0]
  return f[np.sort(rng.choice(pool, M, replace=False))].copy()
