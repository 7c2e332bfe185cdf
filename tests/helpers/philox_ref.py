"""NumPy mirror of the dropout mask of the ConvNormRelu blocks (mix_stage_amd/csrc/dropout_mask.h, include/mixstage.h):
Philox4x32-10, key (seed lo, seed hi), counter (e >> 2, site, step, 0), element e takes word e & 3; keep iff word >= thr with
thr = min(floor(p * 2^32 + 0.5), 0xffffffff); kept values are multiplied by (float)(1 / (1 - p))."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
  """counter: four arrays (or ints) of 32-bit words, key: two -> the four output words as uint64 arrays holding 32-bit values."""
  c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
  c = list(np.broadcast_arrays(*c))
  k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
  for r in range(10):
    if r:
      k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    p0 = np.uint64(M0) * c[0]
    p1 = np.uint64(M1) * c[2]
    hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
    hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
    c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
  return c


def threshold(p):
  assert 0.0 <= p < 1.0, p
  return min(int(math.floor(p * 4294967296.0 + 0.5)), MASK32)


def scale(p):
  return np.float32(1.0 / (1.0 - p))


def words(n, seed, site, step):
  """The mask words of indices 0 .. n - 1."""
  e = np.arange(n, dtype=np.uint64)
  out = philox4x32_10((e >> np.uint64(2), int(site) & MASK32, int(step) & MASK32, 0), (seed[0], seed[1]))
  sel = (e & np.uint64(3)).astype(np.int64)
  return np.stack(out, axis=0)[sel, np.arange(n)]


def factors(n, p, seed, site, step):
  """mask / (1 - p) of indices 0 .. n - 1 as float32."""
  keep = words(n, seed, site, step) >= np.uint64(threshold(p))
  return np.where(keep, scale(p), np.float32(0.0)).astype(np.float32)


def mask_like(shape, p, seed, site, step, channelwise=False):
  """mask / (1 - p) for a conv output of `shape` (B, C, ...) as a float32 array: element dropout indexes the plain (B, C, HW)
  order, channel dropout (nn.Dropout2d) draws once per (b, c) plane, index b * C + c."""
  shape = tuple(int(v) for v in shape)
  if channelwise:
    f = factors(shape[0] * shape[1], p, seed, site, step).reshape(shape[:2] + (1,) * (len(shape) - 2))
    return np.broadcast_to(f, shape).copy()
  return factors(int(np.prod(shape)), p, seed, site, step).reshape(shape)


def seed_words(seed):
  seed = int(seed)
  return (seed & MASK32, (seed >> 32) & MASK32)


def site_of(module_id, visit):
  return (int(module_id) + (int(visit) << 20)) & MASK32
