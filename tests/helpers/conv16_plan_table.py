"""The plans plan_conv16 / plan_wgrad16 (csrc/conv16_plan.h) can pick for the models' 16-bit conv blocks, and one test shape per
plan class that no other test shape reaches: plain data plus the arithmetic that builds the domain (no torch, no GPU).
tests/test_conv16_plan_table_cpu.py holds the table to the domain through tests/helpers/conv16_plan_host.cpp (the planners built
with the host compiler); tests/test_gpu_conv16_plans.py runs every entry against fp64 in bf16 and fp16.

Domain: every conv block of the generator (audio encoder, UNet, grouped decoder and logits), the style encoder, the cluster
classifier and the discriminator, built from (M, T, B) the way joint_late_cluster_soft_style.py / layers.py / speech2gesture.py
build them, for M in {4, 8, 25}, T in {32, 64, 128, 256}, B in 1..64 (forward, data gradient, weight gradient), and B in
{128, 1024} at T = 64 forward only (inference).  The style encoder's last block needs T >= 64 (its input is T / 32 columns and
the kernel spans 4 with padding 1): at T = 32 the model cannot be built with it, and the block is left out there.

Class keys (strings, as conv16_plan_host.cpp's fields spell them):
  conv16, per direction   dir KW wm wn nwn up2 dma ckx nstg wait refill
  wgrad16                 tp up2 npxt nstg one c1
Ragged bits per kernel instance (KW wm wn up2 dma ckx): r_rows (rows % TH), r_ow (OW % TW), r_mg (Mg % BM), r_k (reduction
channels not a multiple of the stage's 8 * CK8).

Counts (tests/test_conv16_plan_table_cpu.py prints them and asserts the first line's two figures), over 9366 distinct block shapes:
87 plan classes in the domain: 74 of conv16_kernel (forward and data gradient), 13 of the weight gradient;
  12 on the run-time wait path of the K loop (wait counts 4, 5, 9, 12 and the like: no literal loop);
  30 classes were reached by no shape of dispatch_table.B16, fp16_block_table.TABLE or test_gpu_kernels16's CASES_1D / CASES_2D, 8 of
  them on the run-time wait path; among them every KW = 8 class but the production one, and the 128 x 128 upsample-add forward that
  only the B = 1024 inference batch reaches.
59 (kernel instance, ragged bit) pairs in the domain, 27 of them on no existing shape.
The 36 entries below cover the 30 classes and the 27 pairs; each entry names only what no entry before it covers, so taking any
one out leaves a class or a pair without a shape.  18 of them are model layers at a size of the domain (`layer`: audio-encoder,
UNet, style-encoder, discriminator blocks, the three kinds of logits) and run in the layer's mode; the others are the cheapest
shapes found in the class -- a few channels per group, the batch and width that give the workgroup count -- and run as LeakyReLU
blocks.  A model layer whose train-mode BatchNorm would see fewer than 32 values per channel (B = 1 at two columns) is no
representative: its statistics are degenerate and the rounding model cannot hold such a case to the fp16 conditions.

No shape of the domain is refused by either planner (ok = 0 / tp = 0 never appears): the CPU test asserts it.

An entry is an fp16_block_table.C dict (id, nd, B, cin, cout, k, s, p, sp, mode, groups, in_mode, out_f32, seed, bn_fused, ...)
plus
  classes   the class keys the entry exists for (the CPU test checks that the entry lands in each)
  ragged    (instance, bit) pairs the entry exists for
  ref_dev   'cpu' or 'device': where _case runs the fp64 reference
  layer     the model layer whose mode the entry takes, or None: not a model layer (LeakyReLU block)
bn_fused of a BN_TRAIN entry says which BatchNorm form the block takes at its size (1: inside the conv launch, 0: a launch of its
own from the stored 16-bit output); no knob is set -- the GPU test asserts the form from the launch labels and the rounding model
is told."""
import os
import re

from helpers.fp16_block_table import C, BARE, LRELU, BN_TRAIN

MS = (4, 8, 25)
TS = (32, 64, 128, 256)
BS = tuple(range(1, 65))
EVAL_BS = (128, 1024)
EVAL_T = 64
IN_MODE_NO = {'plain': 0, 'bcast': 1, 'up2': 2}
CONV_KEY = ('KW', 'wm', 'wn', 'nwn', 'up2', 'dma', 'ckx', 'nstg', 'wait', 'refill')
WGRAD_KEY = ('tp', 'up2', 'npxt', 'nstg', 'one', 'c1')
INSTANCE_KEY = ('KW', 'wm', 'wn', 'up2', 'dma', 'ckx')
RAGGED_BITS = ('r_rows', 'r_ow', 'r_mg', 'r_k')


def blk(name, nd, B, cin, cout, k, s, p, sp, mode=BN_TRAIN, groups=1, in_mode='plain', out_f32=False):
  return dict(name=name, nd=nd, B=B, cin=cin, cout=cout, k=k, s=s, p=p, sp=tuple(sp), mode=mode, groups=groups, in_mode=in_mode,
              out_f32=out_f32)


def model_blocks(M, T, B):
  """The conv blocks of one training step at (M sub-generators, T frames, batch B): per-group channels, input spatial size."""
  out = []
  # AudioEncoder: (B, 1, T, 128) log-mel; blocks 1, 3, 5 halve both axes, the last is 3 x 8
  h, w = T, 128
  for i, (cin, cout, down) in enumerate(((1, 64, False), (64, 64, True), (64, 128, False), (128, 128, True), (128, 256, False),
                                         (256, 256, True), (256, 256, False))):
    out.append(blk('ae%d' % i, 2, B, cin, cout, 4 if down else 3, 2 if down else 1, 1, (h, w)))
    if down:
      h, w = h // 2, w // 2
  out.append(blk('ae7', 2, B, 256, 256, (3, 8), 1, (1, 3), (h, w)))
  # UNet1D, 256 channels, depth 5: two blocks before, five stride-2 blocks, five upsample-add blocks (sp: the full-resolution side)
  out.append(blk('unet_pre', 1, B, 256, 256, 3, 1, 1, (T,)))
  for d in range(5):
    out.append(blk('unet_down%d' % (T >> d), 1, B, 256, 256, 4, 2, 1, (T >> d,)))
  for d in range(4, -1, -1):
    out.append(blk('unet_up%d' % (T >> d), 1, B, 256, 256, 3, 1, 1, (T >> d,), in_mode='up2'))
  # grouped decoder (the first block reads the shared 256 + 10 channels) and the grouped logits
  out.append(blk('dec0_bcast', 1, B, 266, 256, 3, 1, 1, (T,), groups=M, in_mode='bcast'))
  out.append(blk('dec1', 1, B, 256, 256, 3, 1, 1, (T,), groups=M))
  out.append(blk('logits_g', 1, B, 256, 104, 1, 1, 0, (T,), mode=BARE, groups=M, out_f32=True))
  # PoseStyleEncoder: six halvings after the first block; the last block's scores are fp32
  out.append(blk('pse0', 1, B, 104, 64, 3, 1, 1, (T,)))
  w = T
  for i, (cin, cout) in enumerate(((64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, M))):
    if w + 2 >= 4:
      out.append(blk('pse%d' % (i + 1), 1, B, cin, cout, 4, 2, 1, (w,), out_f32=i == 5))
    w //= 2
  # ClusterClassify: its five inner blocks have unet_pre's geometry
  out.append(blk('cls0', 1, B, 266, 256, 3, 1, 1, (T,)))
  out.append(blk('cls_logits', 1, B, 256, M, 1, 1, 0, (T,), mode=BARE, out_f32=True))
  # Speech2Gesture_D
  out.append(blk('d_conv1', 1, B, 104, 64, 4, 2, 1, (T,), mode=LRELU))
  out.append(blk('d_conv2', 1, B, 64, 128, 4, 2, 1, (T // 2,)))
  out.append(blk('d_conv3', 1, B, 128, 256, 4, 1, 1, (T // 4,)))
  out.append(blk('d_logits', 1, B, 256, 1, 4, 1, 0, (T // 4 - 1,), mode=BARE, out_f32=True))
  return out


def geometry(b):
  """What the planners see of a block (mode and output type do not enter)."""
  return (b['nd'], b['B'], b['cin'], b['cout'], b['groups'], b['k'], b['s'], b['p'], tuple(b['sp']), b['in_mode'])


def domain():
  """-> [(geometry, forward only?)], each geometry once (training wins over forward-only)."""
  seen = {}
  for M in MS:
    for T in TS:
      for B in BS:
        for b in model_blocks(M, T, B):
          seen[geometry(b)] = False
    for B in EVAL_BS:
      for b in model_blocks(M, EVAL_T, B):
        seen.setdefault(geometry(b), True)
  return list(seen.items())


def _two(v):
  return tuple(v) if isinstance(v, tuple) else (v, v)


def host_line(id, geo):
  """One input line of conv16_plan_host.cpp."""
  nd, B, cin, cout, groups, k, s, p, sp, in_mode = geo
  (kh, kw), (sh, sw), (ph, pw) = ((1, k), (1, s), (0, p)) if nd == 1 else (_two(k), _two(s), _two(p))
  H, W = (1, sp[0]) if nd == 1 else sp
  return '%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d' % (id, nd, B, cin, cout, groups, kh, kw, sh, sw, ph, pw, H, W, IN_MODE_NO[in_mode])


def parse_host(text):
  """conv16_plan_host.cpp's output -> {id: {'fwd' | 'dgrad' | 'wgrad': {field: value}}} (values: int, `form` a string)."""
  got = {}
  for line in text.splitlines():
    id, which, *fields = line.split()
    got.setdefault(id, {})[which] = {k: (v if k == 'form' else int(v)) for k, v in (f.split('=') for f in fields)}
  return got


def conv_class(which, f):
  return which + ' ' + ' '.join('%s=%d' % (k, f[k]) for k in CONV_KEY)


def wgrad_class(f):
  return 'wgrad ' + ' '.join('%s=%d' % (k, f[k]) for k in WGRAD_KEY)


def instance(f):
  return ' '.join('%s=%d' % (k, f[k]) for k in INSTANCE_KEY)


def classes_of(plans, fwd_only=False):
  """The class keys of one block's three plans (forward only: the forward's)."""
  out = [conv_class('fwd', plans['fwd'])]
  if not fwd_only:
    out += [conv_class('dgrad', plans['dgrad']), wgrad_class(plans['wgrad'])]
  return out


def ragged_of(plans, fwd_only=False):
  """(instance, bit) pairs the block's conv16 launches have set."""
  return [(instance(plans[w]), bit) for w in (('fwd',) if fwd_only else ('fwd', 'dgrad')) for bit in RAGGED_BITS if plans[w][bit]]


def run_time_wait(cls):
  """Is the class on the K loop's run-time wait path?  (conv16_kernel.h: the literal counts have loops of their own.)"""
  if cls.startswith('wgrad') or ' dma=0' in cls:
    return False
  return int(cls.split(' wait=')[1].split()[0]) not in literal_waits()


_LITERALS = []


def literal_waits():
  """The literal wait counts, read from the one list the kernel and the host program are built from (csrc/conv16_plan.h)."""
  if not _LITERALS:
    with open(os.path.join(os.path.dirname(__file__), '..', '..', 'mix_stage_amd', 'csrc', 'conv16_plan.h')) as f:
      m = re.search(r'#define CONV16_WAIT_LITERALS\(X\)((?: X\(\d+\))+)\n', f.read())
    assert m, 'csrc/conv16_plan.h no longer has CONV16_WAIT_LITERALS'
    _LITERALS.extend(int(v) for v in re.findall(r'X\((\d+)\)', m.group(1)))
  return _LITERALS


def refilled(cls):
  return ' refill=1' in cls


def existing_shapes():
  """[(id, geometry, forward only?)] of the shapes other tests already run through the 16-bit blocks."""
  from helpers.dispatch_table import B16
  from helpers.fp16_block_table import TABLE as FP16_TABLE
  import test_gpu_kernels16 as K
  inm = {K.PLAIN: 'plain', K.BCAST: 'bcast', K.UP2: 'up2'}
  out = [('B16:' + e['id'], geometry(e), e['mode'] == 'BN_EVAL') for e in B16]
  out += [('fp16:' + c['id'], geometry(c), False) for c in FP16_TABLE]
  for name, B, cin, cout, groups, k, s, p, W, mode, in_mode, _ in K.CASES_1D:
    out.append(('k16:' + name, (1, B, cin, cout, groups, k, s, p, (W,), inm[in_mode]), mode == K.BN_EVAL))
  for name, B, cin, cout, k, s, p, H, W in K.CASES_2D:
    out.append(('k16:' + name, (2, B, cin, cout, 1, k, s, p, (H, W), 'plain'), False))
  return out


def P(id, nd, B, cin, cout, k, s, p, sp, classes, ragged=(), ref_dev='cpu', layer=None, **kw):
  kw.setdefault('mode', LRELU if layer is None else BN_TRAIN)
  c = C(id, nd, B, cin, cout, k, s, p, tuple(sp), **kw)
  c.update(classes=tuple(classes), ragged=tuple(ragged), ref_dev=ref_dev, layer=layer)
  return c


ENTRIES = [
    P('ae0_b5_32x128', 2, 5, 1, 64, 3, 1, 1, (32, 128), layer='ae0', mode=BN_TRAIN, bn_fused=0, ref_dev='device',
      classes=(
          'dgrad KW=3 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=4 wait=10 refill=1',
          'fwd KW=3 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=4 wait=10 refill=0',),
      ragged=(
          ('KW=3 wm=1 wn=1 up2=0 dma=1 ckx=1', 'r_k'),
          ('KW=3 wm=1 wn=1 up2=0 dma=1 ckx=1', 'r_mg'),)),
    P('pse4_b16_4', 1, 16, 128, 256, 4, 2, 1, (4,), layer='pse4', mode=BN_TRAIN, bn_fused=1,
      classes=(
          'dgrad KW=2 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=4 nstg=2 wait=0 refill=1',
          'fwd KW=4 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=2 nstg=2 wait=0 refill=1',),
      ragged=(
          ('KW=2 wm=1 wn=1 up2=0 dma=1 ckx=4', 'r_rows'),)),
    P('cls_logits_b33_128', 1, 33, 256, 4, 1, 1, 0, (128,), layer='cls_logits', mode=BARE, out_f32=True,
      classes=(
          'dgrad KW=1 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=2 wait=0 refill=0',),
      ragged=(
          ('KW=1 wm=1 wn=1 up2=0 dma=1 ckx=1', 'r_k'),)),
    P('logits_g_b33_32_g8', 1, 33, 256, 104, 1, 1, 0, (32,), groups=8, layer='logits_g', mode=BARE, out_f32=True, ref_dev='device',
      classes=(
          'fwd KW=1 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=8 wait=12 refill=1',),
      ragged=(
          ('KW=1 wm=1 wn=1 up2=0 dma=1 ckx=1', 'r_mg'),
          ('KW=1 wm=1 wn=1 up2=0 dma=1 ckx=1', 'r_rows'),
          ('KW=1 wm=1 wn=2 up2=0 dma=1 ckx=1', 'r_rows'),)),
    P('1d_k4s2_8to104_g25_b33_31', 1, 33, 8, 104, 4, 2, 1, (31,), groups=25,
      classes=(
          'dgrad KW=2 wm=1 wn=2 nwn=2 up2=0 dma=1 ckx=2 nstg=3 wait=9 refill=0',),
      ragged=(
          ('KW=2 wm=1 wn=2 up2=0 dma=1 ckx=2', 'r_mg'),
          ('KW=2 wm=1 wn=2 up2=0 dma=1 ckx=2', 'r_rows'),
          ('KW=4 wm=1 wn=2 up2=0 dma=1 ckx=1', 'r_k'),
          ('KW=4 wm=1 wn=2 up2=0 dma=1 ckx=1', 'r_ow'),
          ('KW=4 wm=1 wn=2 up2=0 dma=1 ckx=1', 'r_rows'),)),
    P('d_logits_b1_7', 1, 1, 256, 1, 4, 1, 0, (7,), layer='d_logits', mode=BARE, out_f32=True,
      classes=(
          'fwd KW=4 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=2 nstg=3 wait=12 refill=1',)),
    P('pse6_b49_8', 1, 49, 256, 4, 4, 2, 1, (8,), layer='pse6', mode=BN_TRAIN, out_f32=True, bn_fused=0,
      classes=(
          'wgrad tp=4 up2=0 npxt=0 nstg=2 one=0 c1=0',)),
    P('d_conv1_b33_256', 1, 33, 104, 64, 4, 2, 1, (256,), layer='d_conv1', mode=LRELU, ref_dev='device',
      classes=(
          'dgrad KW=2 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=3 wait=4 refill=0',),
      ragged=(
          ('KW=2 wm=1 wn=1 up2=0 dma=1 ckx=1', 'r_mg'),)),
    P('unet_up2_b16_2', 1, 16, 256, 256, 3, 1, 1, (2,), in_mode='up2', layer='unet_up2', mode=BN_TRAIN, bn_fused=1,
      classes=(
          'dgrad KW=3 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=2 nstg=4 wait=20 refill=1',)),
    P('unet_down2_b32_2', 1, 32, 256, 256, 4, 2, 1, (2,), layer='unet_down2', mode=BN_TRAIN, bn_fused=1,
      classes=(
          'dgrad KW=2 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=2 nstg=5 wait=24 refill=0',)),
    P('cls_logits_b33_256', 1, 33, 256, 4, 1, 1, 0, (256,), layer='cls_logits', mode=BARE, out_f32=True,
      classes=(
          'dgrad KW=1 wm=1 wn=2 nwn=2 up2=0 dma=1 ckx=1 nstg=2 wait=0 refill=0',)),
    P('ae0_b3_64x128', 2, 3, 1, 64, 3, 1, 1, (64, 128), layer='ae0', mode=BN_TRAIN, bn_fused=0, ref_dev='device',
      classes=(),
      ragged=(
          ('KW=3 wm=1 wn=2 up2=0 dma=1 ckx=2', 'r_mg'),)),
    P('ae5_b1_8x32', 2, 1, 256, 256, 4, 2, 1, (8, 32), layer='ae5', mode=BN_TRAIN, bn_fused=1, ref_dev='device',
      classes=(
          'dgrad KW=2 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=4 nstg=3 wait=13 refill=1',)),
    P('2d_k3x8s1_8to8_b3_64x128', 2, 3, 8, 8, (3, 8), 1, (1, 3), (64, 128), ref_dev='device',
      classes=(
          'dgrad KW=8 wm=1 wn=2 nwn=2 up2=0 dma=1 ckx=2 nstg=3 wait=11 refill=1',
          'fwd KW=8 wm=1 wn=2 nwn=2 up2=0 dma=1 ckx=2 nstg=3 wait=11 refill=1',),
      ragged=(
          ('KW=8 wm=1 wn=2 up2=0 dma=1 ckx=2', 'r_ow'),)),
    P('logits_g_b5_32_g25', 1, 5, 256, 104, 1, 1, 0, (32,), groups=25, layer='logits_g', mode=BARE, out_f32=True, ref_dev='device',
      classes=(),
      ragged=(
          ('KW=1 wm=1 wn=2 up2=0 dma=1 ckx=2', 'r_rows'),)),
    P('1d_k3s1_8to8_g25_b33_31', 1, 33, 8, 8, 3, 1, 1, (31,), groups=25,
      classes=(
          'dgrad KW=3 wm=1 wn=2 nwn=2 up2=0 dma=1 ckx=2 nstg=2 wait=0 refill=0',),
      ragged=(
          ('KW=3 wm=1 wn=2 up2=0 dma=1 ckx=2', 'r_rows'),)),
    P('logits_g_b33_32_g4', 1, 33, 256, 104, 1, 1, 0, (32,), groups=4, layer='logits_g', mode=BARE, out_f32=True, ref_dev='device',
      classes=(
          'dgrad KW=1 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=5 wait=6 refill=0',)),
    P('d_conv1_b48_256', 1, 48, 104, 64, 4, 2, 1, (256,), layer='d_conv1', mode=LRELU, ref_dev='device',
      classes=(
          'dgrad KW=2 wm=1 wn=2 nwn=2 up2=0 dma=1 ckx=2 nstg=2 wait=0 refill=0',)),
    P('pse0_b33_256', 1, 33, 104, 64, 3, 1, 1, (256,), layer='pse0', mode=BN_TRAIN, bn_fused=0, ref_dev='device',
      classes=(
          'dgrad KW=3 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=3 wait=5 refill=0',)),
    P('1d_k4s2_64to8_g8_b33_128', 1, 33, 64, 8, 4, 2, 1, (128,), groups=8, seed=1,
      classes=(
          'fwd KW=4 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=2 wait=0 refill=1',),
      ragged=(
          ('KW=2 wm=1 wn=2 up2=0 dma=1 ckx=1', 'r_rows'),)),
    P('1d_k3s1_104to8_g8_b33_63', 1, 33, 104, 8, 3, 1, 1, (63,), groups=8,
      classes=(
          'fwd KW=3 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=4 wait=10 refill=1',),
      ragged=(
          ('KW=3 wm=1 wn=2 up2=0 dma=1 ckx=1', 'r_rows'),)),
    P('ae1_b5_32x128', 2, 5, 64, 64, 4, 2, 1, (32, 128), layer='ae1', mode=BN_TRAIN, bn_fused=0, ref_dev='device',
      classes=(
          'dgrad KW=2 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=5 wait=12 refill=0',)),
    P('1d_k3s1_266to1_b64_256_up2', 1, 64, 266, 1, 3, 1, 1, (256,), in_mode='up2',
      classes=(),
      ragged=(
          ('KW=3 wm=2 wn=2 up2=0 dma=1 ckx=1', 'r_mg'),)),
    P('1d_k3s1_8to104_g8_b33_31_bcast', 1, 33, 8, 104, 3, 1, 1, (31,), groups=8, in_mode='bcast', seed=2,
      classes=(),
      ragged=(
          ('KW=3 wm=1 wn=1 up2=0 dma=1 ckx=1', 'r_rows'),)),
    P('2d_k4s2_256to8_b64_5x9', 2, 64, 256, 8, 4, 2, 1, (5, 9), ref_dev='device',
      classes=(),
      ragged=(
          ('KW=2 wm=2 wn=2 up2=0 dma=1 ckx=1', 'r_rows'),)),
    P('2d_k3x8s1_8to8_b33_32x16', 2, 33, 8, 8, (3, 8), 1, (1, 3), (32, 16), ref_dev='device',
      classes=(),
      ragged=(
          ('KW=8 wm=1 wn=1 up2=0 dma=1 ckx=1', 'r_ow'),)),
    P('1d_k4s2_64to8_g25_b64_31', 1, 64, 64, 8, 4, 2, 1, (31,), groups=25,
      classes=(
          'fwd KW=4 wm=1 wn=2 nwn=2 up2=0 dma=1 ckx=1 nstg=3 wait=9 refill=0',)),
    P('1d_k1s1_8to256_g25_b33_31', 1, 33, 8, 256, 1, 1, 0, (31,), groups=25,
      classes=(),
      ragged=(
          ('KW=1 wm=2 wn=2 up2=0 dma=1 ckx=1', 'r_rows'),)),
    P('unet_down128_b33_128', 1, 33, 256, 256, 4, 2, 1, (128,), layer='unet_down128', mode=BN_TRAIN, bn_fused=1, ref_dev='device',
      classes=(
          'dgrad KW=2 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=5 wait=12 refill=1',)),
    P('2d_k3x8s1_8to256_b64_5x9', 2, 64, 8, 256, (3, 8), 1, (1, 3), (5, 9), ref_dev='device',
      classes=(),
      ragged=(
          ('KW=8 wm=1 wn=2 up2=0 dma=1 ckx=2', 'r_rows'),)),
    P('1d_k3s1_8to128_b192_256_up2', 1, 192, 8, 128, 3, 1, 1, (256,), in_mode='up2', ref_dev='device',
      classes=(
          'fwd KW=3 wm=2 wn=2 nwn=2 up2=1 dma=0 ckx=1 nstg=0 wait=-1 refill=0',)),
    P('1d_k3s1_8to256_g25_b33_31_bcast', 1, 33, 8, 256, 3, 1, 1, (31,), groups=25, in_mode='bcast', ref_dev='device',
      classes=(),
      ragged=(
          ('KW=3 wm=2 wn=2 up2=0 dma=1 ckx=1', 'r_rows'),)),
    P('2d_k3x8s1_64to8_b33_32x16', 2, 33, 64, 8, (3, 8), 1, (1, 3), (32, 16), seed=2, ref_dev='device',
      classes=(
          'fwd KW=8 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=4 wait=10 refill=1',)),
    P('2d_k3x8s1_8to64_b33_32x16', 2, 33, 8, 64, (3, 8), 1, (1, 3), (32, 16), seed=1, ref_dev='device',
      classes=(
          'dgrad KW=8 wm=1 wn=1 nwn=2 up2=0 dma=1 ckx=1 nstg=4 wait=10 refill=1',)),
    P('2d_k3x8s1_8to128_b96_32x16', 2, 96, 8, 128, (3, 8), 1, (1, 3), (32, 16), seed=2, ref_dev='device',
      classes=(
          'fwd KW=8 wm=2 wn=2 nwn=2 up2=0 dma=1 ckx=1 nstg=2 wait=0 refill=1',),
      ragged=(
          ('KW=8 wm=2 wn=2 up2=0 dma=1 ckx=1', 'r_ow'),)),
    P('2d_k3x8s1_256to8_b192_8x16', 2, 192, 256, 8, (3, 8), 1, (1, 3), (8, 16), seed=2, ref_dev='device',
      classes=(
          'dgrad KW=8 wm=2 wn=2 nwn=2 up2=0 dma=1 ckx=1 nstg=2 wait=0 refill=1',)),
]

BY_ID = {c['id']: c for c in ENTRIES}
