"""CPU: the dropout mask of the ConvNormRelu blocks (p > 0) -- the NumPy mirror the GPU tests compare with
(tests/helpers/philox_ref.py) against the Random123 known answers and against csrc/dropout_mask.h compiled for the host, the
threshold rule, the constants of the source, the validation of p, the numbering of the sites, the C-ABI's two sides, and the
statistics of the mask on the mirror alone."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from helpers import philox_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, 'mix_stage_amd', 'csrc')
NEW_SYMBOLS = ('ms_dropout_bn_workspace', 'ms_dropout_bn_fwd', 'ms_dropout_bn_bwd', 'ms_dropout_advance', 'ms_dropout_mask')

# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SEED = (0x1234, 0x5678)


def test_philox_known_answers():
  for ctr, key, out in KAT:
    got = tuple(int(v) for v in R.philox4x32_10(ctr, key))
    assert got == out, ([hex(v) for v in got], [hex(v) for v in out])
  # vectorised over counters: the same words as one call each
  c0 = np.array([0, 0xffffffff, 0x243f6a88], dtype=np.uint64)
  many = R.philox4x32_10((c0, 0, 0, 0), (0, 0))
  assert tuple(int(w[0]) for w in many) == KAT[0][2]
  assert tuple(int(w[1]) for w in many) == tuple(int(v) for v in R.philox4x32_10((0xffffffff, 0, 0, 0), (0, 0)))


def test_threshold_rule():
  from mix_stage_amd import ops
  assert R.threshold(0.25) == 0x40000000 and R.threshold(0.5) == 0x80000000 and R.threshold(0.0) == 0
  assert R.threshold(0.1) == 429496730 == 0x1999999a           # floor(0.1 * 2^32 + 0.5); 0.1 * 2^32 = 429496729.6
  for p in (1.0 - 2.0 ** -53, math.nextafter(1.0, 0.0), 1.0 - 2.0 ** -33):
    assert p < 1.0 and R.threshold(p) == 0xffffffff, p       # next to 1: clamped, never 2^32
  assert R.threshold(1.0 - 2.0 ** -31) == 0xfffffffe
  for p in (0.0, 0.1, 0.25, 0.5, 0.9, 1.0 - 2.0 ** -31, math.nextafter(1.0, 0.0)):
    assert ops.dropout_threshold(p) == R.threshold(p), p
  assert R.scale(0.5) == np.float32(2.0) and R.scale(0.1) == np.float32(1.0 / 0.9)


def test_constants_are_the_ones_in_the_source():
  src = open(os.path.join(CSRC, 'dropout_mask.h')).read()
  m = re.search(r'PHILOX_M0 = 0x([0-9A-Fa-f]+)u, PHILOX_M1 = 0x([0-9A-Fa-f]+)u, PHILOX_W0 = 0x([0-9A-Fa-f]+)u, PHILOX_W1 = 0x([0-9A-Fa-f]+)u', src)
  assert m and tuple(int(v, 16) for v in m.groups()) == (R.M0, R.M1, R.W0, R.W1) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85)
  assert re.search(r'for \(int r = 0; r < 10; \+\+r\)', src)                                   # ten rounds
  assert re.search(r'\(uint32_t\)\(e >> 2\), site, step, 0u, seed_lo, seed_hi, \(int\)\(e & 3\)', src)      # counter, key, word
  assert 'word >= thr ? scale : 0.f' in src and 'p * 4294967296.0 + 0.5' in src
  # every kernel of dropout.hip draws through that one definition
  hip = open(os.path.join(CSRC, 'dropout.hip')).read()
  assert '#include "dropout_mask.h"' in hip and len(re.findall(r'\bdropout_factor\(', hip)) == 2 and 'philox' not in hip.lower().replace('dropout_mask.h', '')
  assert re.search(r'DROPOUT_FUSED_MAX = 256 \* 16;', hip)


def _compiler():
  found = [shutil.which(c) for c in ('g++', 'clang++', 'c++')] + [p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++') if os.path.exists(p)]
  return next((c for c in found if c), None)


def test_source_definition_compiled_for_the_host_equals_the_mirror(tmp_path):
  cxx = _compiler()
  if cxx is None:
    pytest.skip('no C++ compiler on this machine')
  exe = str(tmp_path / 'dropout_mask_host')
  subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                  '-I', CSRC, os.path.join(HERE, 'helpers', 'dropout_mask_host.cpp'), '-o', exe], check=True)
  lines = ['philox %x %x %x %x %x %x' % (ctr + key) for ctr, key, _ in KAT]
  ps = (0.25, 0.1, 0.5, math.nextafter(1.0, 0.0), 1.0 - 2.0 ** -31)
  lines += ['thr %r' % p for p in ps]
  masks = [(70, 0.25, 7, 0, 0x1234, 0x5678), (1001, 0.1, R.site_of(52, 1), 3, 0xdeadbeef, 0xffffffff), (37, 0.5, 0xffffffff, 0xffffffff, 0, 0)]
  lines += ['mask %d %r %d %d %d %d' % m for m in masks]
  r = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120)
  assert r.returncode == 0, r.stderr
  out = r.stdout.strip().splitlines()
  assert len(out) == len(lines)
  for (ctr, key, exp), line in zip(KAT, out):
    assert tuple(int(v, 16) for v in line.split()) == exp
  for p, line in zip(ps, out[len(KAT):]):
    assert int(line, 16) == R.threshold(p), p
  for (n, p, site, step, lo, hi), line in zip(masks, out[len(KAT) + len(ps):]):
    got = np.array([int(v, 16) for v in line.split()], dtype=np.uint32).view(np.float32)
    assert np.array_equal(got, R.factors(n, p, (lo, hi), site, step)), (n, p, site, step)


def test_mask_layouts():
  # element dropout: the plain (B, C, HW) order, a Philox call straddles rows where HW % 4 != 0
  m = R.mask_like((2, 5, 7), 0.25, SEED, 7, 0)
  assert m.shape == (2, 5, 7) and np.array_equal(m.reshape(-1), R.factors(70, 0.25, SEED, 7, 0))
  assert set(np.unique(m)) <= {np.float32(0.0), np.float32(1.0 / 0.75)}
  # channel dropout: one draw per (b, c) plane
  m2 = R.mask_like((2, 5, 3, 7), 0.5, SEED, 7, 0, channelwise=True)
  assert m2.shape == (2, 5, 3, 7) and np.array_equal(m2[:, :, 0, 0].reshape(-1), R.factors(10, 0.5, SEED, 7, 0))
  assert (m2 == m2[:, :, :1, :1]).all()
  assert R.site_of(3, 0) == 3 and R.site_of(3, 1) == 3 + (1 << 20) and R.site_of(1 << 20, 4095) == ((1 << 20) + (4095 << 20)) & 0xffffffff


def test_p_is_validated():
  import mix_stage_amd as A
  from mix_stage_amd import ops
  for bad in (1, 1.0, 1.5, -0.1, float('nan')):
    with pytest.raises(ValueError):
      A.ConvNormRelu(4, 4, p=bad)
    with pytest.raises(ValueError):
      ops.check_dropout_p(bad, 'test')
  with pytest.raises(ValueError):
    ops.check_dropout_p('half', 'test')
  for type_ in ('1d', '2d'):
    blk = A.ConvNormRelu(4, 4, type=type_, p=0.25)
    assert blk._p == 0.25 and blk.dropout.p == 0.25 and blk._drop_id is None and blk._drop_visit == 0
  assert not A.ConvNormRelu(4, 4)._p and not A.ConvNormRelu(4, 4, p=0.0)._p
  with pytest.raises(ValueError):
    ops.dropout_state_words(-1)
  with pytest.raises(ValueError):
    ops.dropout_state_words(0, 1 << 32)
  assert ops.dropout_state_words(0x89abcdef01234567, 0xfffffffe).tolist() == [0x01234567, 0x89abcdef - (1 << 32), -2, 0]
  assert A.manual_dropout_seed(5) == 5 and ops._dropout['seed'] == 5
  A.manual_dropout_seed(0)


def _model(p=0):
  import mix_stage_amd as A
  G = A.JointLateClusterSoftStyle4_G(num_clusters=8, style_dict={i: i for i in range(8)}, shape={}, p=p)
  D = A.Speech2Gesture_D(p=p)
  return A.GAN(G, D, criterion='L1Loss', input_modalities=['audio/log_mel_400'])


def test_site_numbering_follows_modules_order():
  import mix_stage_amd as A
  from mix_stage_amd import layers, ops
  m = _model(p=0.1)
  blocks = [b for b in m.modules() if isinstance(b, layers.ConvNormRelu)]
  # (the reference builds a few blocks of G without handing p on: they stay p == 0 and are numbered like the others)
  dropping = layers.dropout_blocks(m)
  assert dropping == [b for b in blocks if b._p] and len(blocks) - 8 < len(dropping) <= len(blocks) and all(b._p == 0.1 for b in dropping)
  assert all(b._drop_id is None for b in blocks)
  assert A.number_dropout_sites(m) == len(blocks) < (1 << 20)
  assert [b._drop_id for b in blocks] == list(range(len(blocks)))
  assert all(b._drop_visit == 0 and b._drop_state is None for b in blocks)
  # a sub-tree numbered on its own starts at 0 again; blocks with p == 0 are counted, so the ids do not move with p
  assert A.number_dropout_sites(m.D) == len([b for b in m.D.modules() if isinstance(b, layers.ConvNormRelu)])
  assert [b._drop_id for b in m.D.modules() if isinstance(b, layers.ConvNormRelu)][:2] == [0, 1]
  m0 = _model(p=0)
  assert layers.dropout_blocks(m0) == [] and A.number_dropout_sites(m0) == len(blocks)
  # never numbered: ids from the process-wide counter, which starts at 2^20
  a, b = ops.next_dropout_id(), ops.next_dropout_id()
  assert b == a + 1 and a >= (1 << 20)
  # the state_dict does not know about any of it
  assert list(m.state_dict().keys()) == list(m0.state_dict().keys())


def _decl(name, hdr):
  m = re.search(r'\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;' % name, hdr, flags=re.S)
  assert m, '%s is not declared in include/mixstage.h' % name
  return [a.strip() for a in m.group(1).split(',')]


def test_abi_is_still_4_and_the_new_symbols_are_declared_on_both_sides():
  from mix_stage_amd import _lib
  hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mixstage.h')).read(), flags=re.S)
  assert re.search(r'#define\s+MS_ABI_VERSION\s+4\b', hdr)
  L = _lib.lib()
  assert L.ms_abi_version() == 4
  for name in NEW_SYMBOLS:
    args = _decl(name, hdr)
    restype, argtypes = _lib.SIGNATURES[name]
    assert len(args) == len(argtypes), (name, args)
    assert restype is (ctypes.c_size_t if name.endswith('_workspace') else ctypes.c_int), name
    assert hasattr(L, name)
  full = open(os.path.join(ROOT, 'include', 'mixstage.h')).read()
  assert 'layers.py:32-78' in full[full.index('Dropout inside a block'):full.index('ms_dropout_bn_workspace(int B')]
  # one workgroup owns a channel up to 4096 values: no scratch; beyond, the chunk partials of launch_bn_bwd's chunking
  assert L.ms_dropout_bn_workspace(32, 8, 128) == 0 and L.ms_dropout_bn_workspace(2, 8, 2049) == 2 * 8 * 2 * 4
  assert L.ms_dropout_bn_workspace(0, 8, 8) == 0


def _sigma(keep, n, p):
  return (keep - n * (1.0 - p)) / math.sqrt(n * p * (1.0 - p))


def test_keep_rate_is_binomial():
  n = 1 << 20
  for p, step in ((0.1, 0), (0.5, 0), (0.25, 1)):
    f = R.factors(n, p, SEED, 7, step)
    s = _sigma(int((f != 0).sum()), n, p)
    print('p=%g step=%d: %+.2f sigma' % (p, step, s))
    assert abs(s) < 4.0, (p, step, s)
    assert set(np.unique(f)) == {np.float32(0.0), R.scale(p)}


def test_two_sites_or_two_steps_do_not_share_masks():
  n, p, row = 1 << 20, 0.5, 64
  base = R.factors(n, p, SEED, 7, 0) != 0
  agree_p = p * p + (1.0 - p) * (1.0 - p)
  for site, step, seed in ((8, 0, SEED), (7, 1, SEED), (R.site_of(7, 1), 0, SEED), (7, 0, (0x1235, 0x5678)), (7, 0, (0x1234, 0x5679))):
    other = R.factors(n, p, seed, site, step) != 0
    same = base == other
    # element-wise agreement is that of two independent masks (4 sigma), and no row of 64 is shared: chance gives 2^-64 a row
    s = (int(same.sum()) - n * agree_p) / math.sqrt(n * agree_p * (1.0 - agree_p))
    assert abs(s) < 4.0, (site, step, seed, s)
    assert int(same.reshape(-1, row).all(axis=1).sum()) == 0, (site, step, seed)
