"""The queued weight gradients (ops.enable_deferred_wgrad: ms_bwd_options.defer_wgrad_launch, ms_wgrad_flush,
ms_wgrad_reduce_multi), one entry per case, as plain data in the style of dispatch_table.py and ew_table.py.
tests/test_gpu_wgrad_queue.py runs every entry as ONE backward pass over all its blocks and compares each block with fp64;
tests/test_wgrad_queue_table_cpu.py recomputes the claims and ties the constants below to the sources.

An entry:
  id       unique name
  blocks   the batch: independent conv blocks, each a dict of
             nd, B, cin, cout, groups, k, s, p, sp, mode, in_mode, prec   (the fields of dispatch_table.py; cin / cout per group)
             out_f32                                                      (16-bit BARE blocks: fp32 output, the score layers)
  twice    every block's module is applied to two inputs in the one backward pass (the discriminator's fake and real use)
  want     what the case exists for, typed by hand: {'launches': [(queue, jobs), ...] in any order, 'kinds': [wave_kind per wave
           job, in block order], 'families': [family per block], 'splits1': number of blocks with splits == 1 (at least),
           'slabs': number of blocks with splits > 1 (at least)} -- each key optional
  claims   what the mirrors below compute for the blocks (compute_claims): per block its family, wave_kind, splits, workgroups,
           whether it is queued; per entry the multi-job launches (label regex, jobs, workgroups) and the reduction's jobs.  The CPU
           guard recomputes them and checks them against `want`; the GPU test checks them against the launch labels.
  expect   regexes: each must match a launch label of the batch's backward pass (built from the claims)
  forbid   regexes: none may match one (the unqueued launches of a queued block)
  why      the case in words

The mirrors restate the host code that decides where a block's weight gradient runs:
  plan_wgrad_patch + wgrad_wave_ok + wave_setup   csrc/wgrad_patch.hip   (family wave / patch, else gather; wave_kind; splits)
  wgrad_splits, shape_of                          csrc/conv_igemm.hip    (gather kernel: splits, kernel shape 0..4)
  plan_wgrad16, wg16_npxt_queued                  csrc/wgrad16.hip       (16-bit: taps, slots, splits)
  pack_jobs + the three flush routines            csrc/job_queue.h       (jobs per launch, rollover at the job limit)
  launch_reduce_splits_multi                      csrc/conv_igemm.hip    (wave / 16-byte / scalar form, blocks per job)"""
import re

from helpers.dispatch_table import TABLE as DISPATCH

# ---- constants of the sources (tests/test_wgrad_queue_table_cpu.py ties each to its line by regex) -----------------------------------
WGP_MAX_JOBS = 48              # csrc/kernels.h
WG_MAX_JOBS = 24               # csrc/kernels.h
WG16_MAX_JOBS = 20             # csrc/conv16.h
MAX_LAUNCH_WGS = 0x3fffffff    # csrc/job_queue.h
REDUCE_BATCH_MAX = 96          # csrc/kernels.h
WGRAD_STEPS_PER_WG = 96        # csrc/wgrad_patch.hip g_wgrad_steps_per_wg
WGRAD_MIN_WGS = 48             # csrc/wgrad_patch.hip g_wgrad_min_wgs
WGRAD_TILES_PER_WG = 16        # csrc/wgrad_patch.hip g_wgrad_tiles_per_wg
WGRAD_PATCH_TARGET_WGS = 768   # csrc/wgrad_patch.hip g_wgrad_patch_target_wgs
PATCH_MIN_TILES = 4            # csrc/wgrad_patch.hip `pl.n_tiles < (g_patch_min_wgs > 0 ? 4 : 1)` (g_patch_min_wgs = 32)
GATHER_TILE_TARGET = 512       # csrc/conv_igemm.hip wgrad_splits
WG16_TARGET_WGS = 128          # csrc/wgrad16.hip g_wgrad16_target_wgs
WG16_NPX = 5                   # csrc/wgrad16.hip
WG16_SPLITS_MAX = 64           # csrc/wgrad16.hip plan_wgrad16
REDUCE_WAVE_SPLITS = 32        # csrc/conv_igemm.hip launch_reduce_splits_multi: `splits >= 32 && n <= 65536`
REDUCE_WAVE_N = 65536
REDUCE_PER_BLOCK = 1024        # csrc/conv_igemm.hip launch_reduce_splits_multi: min(cdiv(n, 1024), 512) blocks of 256 threads
REDUCE_BLOCK_CAP = 512


def cdiv(a, b):
  return (a + b - 1) // b


def Bk(nd, B, cin, cout, groups, k, s, p, sp, mode='BN_TRAIN', in_mode='plain', prec='fp32', out_f32=False):
  return dict(nd=nd, B=B, cin=cin, cout=cout, groups=groups, k=k, s=s, p=p, sp=tuple(sp), mode=mode, in_mode=in_mode, prec=prec,
              out_f32=out_f32)


def geometry(b):
  """-> dict(KH, KW, SH, SW, PH, PW, H, W, OH, OW) as ops.ConvGeom.desc builds the descriptor (1-D: KH = SH = 1, PH = 0, H = 1)."""
  two = lambda v: (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else ((int(v), int(v)) if b['nd'] == 2 else (1, int(v)))
  KH, KW = two(b['k'])
  SH, SW = two(b['s'])
  PH, PW = two(b['p'])
  if b['nd'] == 1:
    KH, SH, PH, H, W = 1, 1, 0, 1, b['sp'][0]
  else:
    H, W = b['sp']
  return dict(KH=KH, KW=KW, SH=SH, SW=SW, PH=PH, PW=PW, H=H, W=W, OH=(H + 2 * PH - KH) // SH + 1, OW=(W + 2 * PW - KW) // SW + 1)


# ---- fp32: csrc/wgrad_patch.hip ----------------------------------------------------------------------------------------------------------
def plan_wgrad_patch(nd, Cog, Kg, groups, KH, KW, SH, SW, B, OH, OW, W, up2, batched):
  """plan_wgrad_patch with g_precision = 0, g_wgrad_wave = 1 -> None (the gather kernel takes the layer) or
  dict(tw, n_tiles, wave, splits, tiles_per_split)."""
  S = SW
  if nd == 2 and SH != SW:
    return None
  known = (KH, KW, S) in ((1, 3, 1), (1, 4, 2), (1, 4, 1), (1, 1, 1), (3, 3, 1), (4, 4, 2), (3, 8, 1))
  if not known:
    return None
  if (OW < 16) if nd == 1 else (OW < 15):
    return None
  rows, imgs = (B, 1) if nd == 1 else (OH, B)
  tw = (64 if OW > 32 else 32 if OW > 16 else 16) if nd == 1 else (32 if OW > 16 else 16)
  th = 64 // tw
  tiles_y, tiles_x = cdiv(rows, th), cdiv(OW, tw)
  n_tiles = imgs * tiles_y * tiles_x
  if n_tiles < PATCH_MIN_TILES:
    return None
  wshape = (KH, KW, S) in ((1, 3, 1), (1, 4, 2), (1, 1, 1), (3, 3, 1), (4, 4, 2))
  wragged = (OW & 15) != 0
  if ((wshape or (KH, KW, S) == (3, 8, 1)) and W > 0 and (W & 3) == 0 and Kg >= 64 and
      (Cog > 64 or (Kg >= 256 and KH * KW > 1 and not up2 and not wragged)) and (not up2 or (KH == 1 and KW == 3)) and
      (not wragged or (S == 1 and not up2))):
    wave = 2 if Cog <= 64 else 1
    bm, bn = (64, 256) if wave == 2 else (128, 128)
    wbase = cdiv(Cog, bm) * cdiv(Kg, bn) * groups
    n_steps = imgs * rows * cdiv(OW, 16)
    if batched:
      want = max(1, n_steps // max(1, WGRAD_STEPS_PER_WG))
      floor_ = min(max(1, n_steps // 4), cdiv(WGRAD_MIN_WGS, max(1, wbase)))
      sp = max(want, floor_)
    else:
      sp = max(1, WGRAD_PATCH_TARGET_WGS // wbase) if wbase < WGRAD_PATCH_TARGET_WGS else 1
      sp = min(sp, max(1, n_steps // 4))
    sp = min(sp, max(1, n_tiles))
    tps = cdiv(n_tiles, sp)
    return dict(tw=tw, n_tiles=n_tiles, wave=wave, splits=cdiv(n_tiles, tps), tiles_per_split=tps, tiles_y=tiles_y, tiles_x=tiles_x)
  base = cdiv(Cog, 64) * cdiv(Kg, 64) * groups
  splits = max(1, WGRAD_PATCH_TARGET_WGS // base) if base < WGRAD_PATCH_TARGET_WGS else 1
  splits = min(splits, max(1, n_tiles))
  if batched:
    want = max(1, n_tiles // max(1, WGRAD_TILES_PER_WG))
    floor_ = min(max(1, n_tiles), cdiv(WGRAD_MIN_WGS, max(1, base)))
    splits = min(splits, max(want, floor_))
  tps = cdiv(n_tiles, splits)
  return dict(tw=tw, n_tiles=n_tiles, wave=0, splits=cdiv(n_tiles, tps), tiles_per_split=tps, tiles_y=tiles_y, tiles_x=tiles_x)


def wave_kind(b, pl):
  """wgrad_wave_ok + wave_mode + wave_setup for a queued job (no in-launch counters; tensors of the allocator are 16-byte
  aligned) -> the job's wave_kind (2..7), or 0: the 64 x 64 patch kernel takes the layer."""
  g = geometry(b)
  KH, KW, S, up2 = g['KH'], g['KW'], g['SW'], b['in_mode'] == 'up2'
  if not pl['wave']:
    return 0
  if (KH, KW, S) not in ((1, 3, 1), (1, 4, 2), (1, 1, 1), (3, 3, 1), (4, 4, 2), (3, 8, 1)):
    return 0
  if up2 and not (KH == 1 and KW == 3):
    return 0
  if (KW == 1 and g['PW'] != 0) or g['PW'] > 3:
    return 0
  cin_tot = b['cin'] * (1 if b['in_mode'] == 'bcast' else b['groups'])
  ctot = b['cout'] * b['groups']
  H, W, OH, OW = g['H'], g['W'], g['OH'], g['OW']
  # plane_strides (csrc/block_geom.h): 1-D rows are the batch items; (cols, img, chan, row)
  src = (W, 0, W, cin_tot * W) if b['nd'] == 1 else (W, cin_tot * H * W, H * W, W)
  out = (OW, 0, OW, ctot * OW) if b['nd'] == 1 else (OW, ctot * OH * OW, OH * OW, OW)
  if (src[0] | src[1] | src[2] | src[3]) & 3:
    return 0
  dy_aligned = ((out[0] & 15) | ((out[1] | out[2] | out[3]) & 3)) == 0
  if not dy_aligned and (up2 or S != 1 or b['cout'] <= 64):
    return 0
  mode = 2 if up2 else (0 if dy_aligned else 1)
  assert not (mode and (pl['wave'] == 2 or S != 1)), 'wave_setup refuses this layer'
  return 5 + mode if mode else 2 * S + (1 if pl['wave'] == 2 else 0)


def wgrad_c1(b):
  """wgrad_c1_of (csrc/api.hip, csrc/conv_c1.hip): the single-input-channel 3 x 3 block, launched at once."""
  g = geometry(b)
  return (b['prec'] == 'fp32' and b['groups'] == 1 and b['cin'] == 1 and b['cout'] == 64 and (g['KH'], g['KW'], g['SH'], g['SW']) == (3, 3, 1, 1) and
          (g['PH'], g['PW']) == (1, 1) and g['H'] > 1 and b['in_mode'] == 'plain' and (g['W'] & 3) == 0)


def gather_splits(Cog, Kg, groups, npix):
  tiles = cdiv(Cog, 64) * cdiv(Kg, 64) * groups
  splits = cdiv(GATHER_TILE_TARGET, tiles) if tiles < GATHER_TILE_TARGET else 1
  return max(1, min(splits, cdiv(npix, 64)))


def gather_shape(KH, KW, up2):
  if KH == 1 and KW == 4 and not up2:
    return 0
  if KH == 1 and KW == 3:
    return 2 if up2 else 1
  return 4 if up2 else 3


def plan_fp32(b, batched=True):
  """Where an fp32 block's weight gradient runs in trainer mode -> dict(family, queue, kind, splits, wgs, length, queued)."""
  g = geometry(b)
  Cog, Kg, groups, up2 = b['cout'], b['cin'] * g['KH'] * g['KW'], b['groups'], b['in_mode'] == 'up2'
  if wgrad_c1(b):
    return dict(family='c1', queue=None, kind=0, splits=max(2, min(1024, cdiv(b['B'] * g['H'], 4))), wgs=0, length=0, queued=False)
  pl = plan_wgrad_patch(b['nd'], Cog, Kg, groups, g['KH'], g['KW'], g['SH'], g['SW'], b['B'], g['OH'], g['OW'], g['W'], up2, batched)
  if pl is None:
    sp = gather_splits(Cog, Kg, groups, b['B'] * g['OH'] * g['OW'])
    return dict(family='gather', queue=('gather', gather_shape(g['KH'], g['KW'], up2)), kind=0, splits=sp,
                wgs=cdiv(Kg, 64) * cdiv(Cog, 64) * groups * sp, length=0, queued=True)
  kind = wave_kind(b, pl)
  sp = pl['splits']
  if kind:
    bm, bn = (64, 256) if pl['wave'] == 2 else (128, 128)
    imgs = pl['n_tiles'] // max(1, pl['tiles_y'] * pl['tiles_x'])
    rows = b['B'] if b['nd'] == 1 else g['OH']
    n_steps = imgs * rows * cdiv(g['OW'], 16)
    return dict(family='wave', queue=('wave',), kind=kind, splits=sp, wgs=cdiv(Kg, bn) * cdiv(Cog, bm) * groups * sp,
                length=4 * cdiv(n_steps, sp), queued=True)
  return dict(family='patch', queue=('patch', g['KH'], g['KW'], g['SW'], pl['tw'], 1 if up2 else 0), kind=0, splits=sp,
              wgs=cdiv(Kg, 64) * cdiv(Cog, 64) * groups * sp, length=4 * pl['tiles_per_split'], queued=True)


# ---- 16-bit: csrc/wgrad16.hip -------------------------------------------------------------------------------------------------------------
def wg16_xpitch(thpcx):
  return ((thpcx + 11) & ~15) + 4


def wg16_npxt_queued(npx):
  """Slots of input rows a queued job's kernel instance keeps in registers: the 5-slot instance up to 5 slots (the unqueued launch
  takes the 3-slot instance up to 3), else the per-tile loop."""
  return 5 if npx <= 5 else 0


def wg16_npxt(npx):
  return 3 if npx <= 3 else 5 if npx <= 5 else 0


def plan_16(b):
  """plan_wgrad16 + queue_wgrad16 -> dict(family, queue, npx, splits, wgs, queued)."""
  g = geometry(b)
  KH, KW, SW, OW, OH, up2 = g['KH'], g['KW'], g['SW'], g['OW'], g['OH'], b['in_mode'] == 'up2'
  Cog, Cig, groups = b['cout'], b['cin'], b['groups']
  rows, imgs = (b['B'], 1) if b['nd'] == 1 else (OH, b['B'])
  tp = 1 if KW == 1 else 3 if KW == 3 else 4 if KW % 4 == 0 else 2 if KW == 2 else 0
  assert tp, 'no 16-bit weight-gradient kernel'
  ktg = KW // tp
  tw = 1
  while tw < OW:
    tw <<= 1
  tw = min(tw, 64)
  th = 64 // tw
  pcx = (tw - 1) * SW + tp
  xv = 8 * wg16_xpitch(th * pcx)
  npx = cdiv(xv, 256)
  assert not (up2 and npx > WG16_NPX) and xv <= 65535
  tiles_y, tiles_x = cdiv(rows, th), cdiv(OW, tw)
  n_tiles = imgs * tiles_y * tiles_x
  base = cdiv(Cog, 64) * cdiv(Cig, 64) * groups * KH * ktg
  splits = max(1, min(cdiv(WG16_TARGET_WGS, base), n_tiles // 2))
  splits = min(splits, WG16_SPLITS_MAX)
  tps = cdiv(n_tiles, max(1, splits))
  splits = cdiv(n_tiles, tps)
  c1 = (not up2) and Cig == 1 and groups == 1 and KH * KW <= 9
  if Cig == 1 and groups == 1 and (KH, KW, SW) == (3, 3, 1) and not up2:
    col_tiles, total_rows = cdiv(OW, 64), imgs * rows
    row_splits = max(1, min(256 // col_tiles, total_rows // 8))
    splits = cdiv(total_rows, cdiv(total_rows, row_splits)) * col_tiles
  if c1:
    return dict(family='c1_16', queue=None, kind=0, npx=npx, splits=splits, wgs=0, length=0, queued=False)
  return dict(family='h16', queue=('h16', b['prec'], 3 if up2 else tp, 1 if up2 else 0, 0 if up2 else wg16_npxt_queued(npx)), kind=0, npx=npx,
              npxt_unqueued=0 if up2 else wg16_npxt(npx), splits=splits, wgs=cdiv(Cig, 64) * cdiv(Cog, 64) * groups * KH * ktg * splits, length=0,
              queued=True)


def plan(b, batched=True):
  return plan_16(b) if b['prec'] in ('bf16', 'fp16') else plan_fp32(b, batched)


# ---- the flush routines and the reduction -----------------------------------------------------------------------------------------------
def weight_elems(b):
  g = geometry(b)
  return b['cout'] * b['groups'] * b['cin'] * g['KH'] * g['KW']


def _label_regex(queue, jobs, wgs):
  if queue[0] == 'wave':
    return r'^wgrad_wave_multi_kernel<0,0,0,0,0>\|conv_wgrad_wave multi k0x0 s0 tw0 up0 jobs%d wgs%d$' % (jobs, wgs)
  if queue[0] == 'patch':
    _, KH, KW, S, tw, up2 = queue
    return (r'^wgrad_patch_multi_kernel<%d,%d,%d,%d,%d>\|conv_wgrad_patch multi k%dx%d s%d tw%d up%d jobs%d wgs%d$'
            % (KH, KW, S, tw, up2, KH, KW, S, tw, up2, jobs, wgs))
  if queue[0] == 'gather':
    return r'^wgrad_multi_kernel<%d>\|conv_wgrad_gather multi shape%d jobs%d wgs%d$' % (queue[1], queue[1], jobs, wgs)
  _, prec, tp, up2, _ = queue
  return (r'^wgrad16_multi_kernel<%s,%d,%d>\|conv_wgrad_cb8 multi taps%d up%d jobs%d wgs%d$'
          % ('bf16' if prec == 'bf16' else 'f16', tp, up2, tp, up2, jobs, wgs))


def flush_launches(plans):
  """The multi-job launches one ms_wgrad_flush makes of these queued jobs (given in queue order) -> [(queue key, [job indices])].
  The packing rule is pack_jobs in csrc/job_queue.h (tests/test_job_queue_cpu.py runs it against this mirror without a GPU): the jobs
  of the first unlaunched job's instance, in order, a launch ending at the family's job limit or before the job that would take its
  workgroups past MAX_LAUNCH_WGS.  wgrad_patch_flush first stable-sorts by workgroup length (longest first), WGP_MAX_JOBS at a time;
  wgrad_gather_flush goes by shape 0..4, WG_MAX_JOBS at a time; wgrad16_flush groups by (type, taps, input form, slots) in queue
  order, WG16_MAX_JOBS at a time."""
  out = []
  patch = [i for i, p in enumerate(plans) if p['queued'] and p['family'] in ('wave', 'patch')]
  patch.sort(key=lambda i: -plans[i]['length'])                    # (sorted() is stable, like std::stable_sort)
  gather = [i for i, p in enumerate(plans) if p['queued'] and p['family'] == 'gather']
  h16 = [i for i, p in enumerate(plans) if p['queued'] and p['family'] == 'h16']

  def launches(queue, mine, limit):
    cur, wgs = [], 0
    for k in mine:
      if cur and (len(cur) == limit or wgs + plans[k]['wgs'] > MAX_LAUNCH_WGS):
        out.append((queue, cur))
        cur, wgs = [], 0
      cur.append(k)
      wgs += plans[k]['wgs']
    if cur:
      out.append((queue, cur))

  def by_head(order, limit):
    done = set()
    for i in order:
      if i in done:
        continue
      mine = [k for k in order if k not in done and plans[k]['queue'] == plans[i]['queue']]
      done.update(mine)
      launches(plans[i]['queue'], mine, limit)
  by_head(patch, WGP_MAX_JOBS)
  for shape in range(5):
    launches(('gather', shape), [i for i in gather if plans[i]['queue'][1] == shape], WG_MAX_JOBS)
  by_head(h16, WG16_MAX_JOBS)
  return out


def reduce_form(n, splits, aligned=True):
  """launch_reduce_splits_multi + reduce_splits_multi_kernel -> (form, workgroups) of one job."""
  if splits >= REDUCE_WAVE_SPLITS and n <= REDUCE_WAVE_N:
    return 'wave', cdiv(n, 4)
  blocks = max(1, min(cdiv(n, REDUCE_PER_BLOCK), REDUCE_BLOCK_CAP))
  return ('vec16' if (n & 3) == 0 and aligned else 'scalar'), blocks


def reduce_launches(n_jobs):
  """jobs per launch of one ms_wgrad_reduce_multi call."""
  return [min(REDUCE_BATCH_MAX, n_jobs - at) for at in range(0, n_jobs, REDUCE_BATCH_MAX)]


# unqueued launches of a block's weight gradient (and the single-job reduction): none may appear for a queued block
UNQUEUED = (r'\|conv_wgrad_wave k', r'^wgrad_patch_kernel<', r'^wgrad_kernel<', r'^wgrad16_kernel<', r'^wgrad_reduce_splits ')
AT_ONCE = {'c1': r'^wgrad_c1_3x3_kernel\|conv_wgrad_c1 ', 'c1_16': r'^wgrad16_c1_kernel<(bf16|f16)>\|conv_wgrad_cb8 c1 '}


def compute_claims(blocks, twice=False):
  plans = [plan(b) for b in blocks]
  launches = []
  for queue, idx in flush_launches(plans):
    launches.append(dict(queue=queue, jobs=len(idx), wgs=sum(plans[i]['wgs'] for i in idx), blocks=idx,
                         label=_label_regex(queue, len(idx), sum(plans[i]['wgs'] for i in idx))))
  # the reduction: one job per block with slabs (first round); a module's second use adds one job per parameter in a second round
  slabs = [i for i, p in enumerate(plans) if p['splits'] > 1]
  rounds = [len(slabs)]
  if twice:
    per_block = [4 if b['mode'] == 'BN_TRAIN' else 2 for b in blocks]            # dw, dbias (+ dgamma, dbeta) temporaries
    first = [per_block[i] if i not in slabs else per_block[i] - 1 for i in range(len(blocks))]
    # (the temporaries' jobs are queued as the second use's backward runs, the slab job after the first use's: a slot's first job
    # goes to round 1, its second to round 2 -- dw of a block with slabs has two jobs, everything else one)
    rounds = [len(slabs) + sum(first), len(slabs)]
  reduce_jobs = [n for r in rounds if r for n in reduce_launches(r)]
  return dict(blocks=[dict(family=p['family'], kind=p['kind'], splits=p['splits'], wgs=p['wgs'], queued=p['queued'], npx=p.get('npx'),
                           npxt=(p['queue'][4] if p['family'] == 'h16' else None), npxt_unqueued=p.get('npxt_unqueued')) for p in plans],
              launches=launches, reduce_jobs=reduce_jobs)


def Q(id, blocks, want, why, twice=False):
  claims = compute_claims(blocks, twice)
  expect = [l['label'] for l in claims['launches']] + [r'^wgrad_reduce_multi jobs%d$' % n for n in sorted(set(claims['reduce_jobs']))]
  expect += sorted(set(AT_ONCE[c['family']] for c in claims['blocks'] if c['family'] in AT_ONCE))
  forbid = list(UNQUEUED) if (all(c['queued'] for c in claims['blocks']) and not twice) else []
  return dict(id=id, blocks=blocks, twice=twice, want=want, claims=claims, expect=tuple(expect), forbid=tuple(forbid), why=why)


def _from_dispatch(eid):
  e = next(e for e in DISPATCH if e['id'] == eid)
  assert e['prec'] == 'fp32' and not e['pair']
  return Bk(e['nd'], e['B'], e['cin'], e['cout'], e['groups'], e['k'], e['s'], e['p'], e['sp'], e['mode'], e['in_mode'])


def _as(prec, blocks):
  return [dict(b, prec=prec) for b in blocks]


# ---- the blocks ------------------------------------------------------------------------------------------------------------------------
# (B is the smallest at which the planner still gives the layer to the family: a patch / wave layer needs 4 pixel tiles of 64)
WAVE_ALL = [
    Bk(1, 8, 96, 136, 1, 3, 1, 1, (32,)),                          # kind 2: 128 x 128 tile, ragged in rows (136) and columns (288); slabs
    Bk(1, 4, 104, 64, 1, 3, 1, 1, (64,)),                          # kind 3: 64 x 256 tile, Kg = 312
    Bk(1, 8, 128, 128, 1, 4, 2, 1, (64,)),                         # kind 4
    Bk(1, 8, 64, 64, 1, 4, 2, 1, (64,)),                           # kind 5
    Bk(1, 4, 128, 128, 1, 3, 1, 1, (40,)),                         # kind 6: dy rows of 40 = 2.5 runs of 16
    Bk(1, 8, 128, 128, 1, 3, 1, 1, (32,), in_mode='up2'),          # kind 7
    Bk(1, 4, 64, 104, 4, 1, 1, 0, (64,), mode='BARE'),             # kind 2, 1 x 1, grouped
    Bk(1, 4, 74, 128, 4, 3, 1, 1, (64,), in_mode='bcast'),         # kind 2, shared input
    Bk(2, 2, 64, 128, 1, 3, 1, 1, (16, 32)),                       # 2-D 3 x 3
    Bk(2, 2, 64, 64, 1, 4, 2, 1, (16, 32)),                        # 2-D 4 x 4 stride 2
    Bk(2, 2, 128, 128, 1, (3, 8), 1, (1, 3), (8, 16)),             # 2-D (3, 8): OW = 15, ragged
    Bk(1, 4, 96, 136, 8, 3, 1, 1, (64,)),                          # the first block's layer with 8 groups: 48 tiles -> splits == 1
]
PATCH_ALL = [
    Bk(1, 4, 16, 64, 1, 3, 1, 1, (64,)),                           # Kg = 48 < 64
    Bk(1, 4, 128, 128, 1, 3, 1, 1, (34,)),                         # W % 4 != 0; same instance (tw64) as the block above
    Bk(1, 8, 16, 64, 1, 3, 1, 1, (32,)),                           # tw32
    Bk(1, 16, 64, 128, 1, 4, 1, 1, (17,)),                         # 1 x 4 stride 1: no wave instance
    Bk(1, 8, 32, 64, 1, 3, 1, 1, (32,), in_mode='up2'),            # patch kernel, upsample-add input
    Bk(2, 2, 1, 64, 1, 3, 1, 1, (16, 32)),                         # the single-input-channel form: launched at once
]
GATHER_ALL = [
    Bk(1, 4, 64, 64, 1, 4, 2, 1, (8,)), Bk(1, 4, 128, 72, 1, 4, 2, 1, (4,)),                         # shape 0
    Bk(1, 16, 64, 64, 1, 3, 1, 1, (8,)),                                                             # shape 1; 128 pixels: two slabs
    Bk(1, 4, 64, 64, 1, 3, 1, 1, (8,), in_mode='up2'),                                               # shape 2
    Bk(1, 4, 64, 8, 1, 1, 1, 0, (8,), mode='BARE'), Bk(2, 2, 32, 32, 1, 3, 1, 1, (4, 8)),            # shape 3
]
H16_ALL = [
    Bk(1, 4, 64, 8, 1, 1, 1, 0, (64,), mode='BARE', out_f32=True),                                   # taps 1
    Bk(1, 4, 64, 64, 1, 3, 1, 1, (64,)), Bk(1, 4, 64, 64, 1, 3, 1, 1, (16,)),                        # taps 3, npx 3: the 5-slot instance
    Bk(1, 4, 64, 64, 1, 4, 2, 1, (64,)),                                                             # taps 4, npx 5
    Bk(1, 6, 64, 64, 1, 4, 2, 1, (4,)),
    Bk(1, 4, 128, 256, 1, 4, 1, 1, (16,)),
    Bk(1, 4, 64, 64, 1, 3, 1, 1, (16,), in_mode='up2'), Bk(1, 4, 64, 64, 1, 3, 1, 1, (2,), in_mode='up2'),
    Bk(1, 4, 128, 128, 4, 3, 1, 1, (64,)),
    Bk(1, 4, 74, 128, 4, 3, 1, 1, (64,), in_mode='bcast'),
    Bk(2, 2, 64, 128, 1, 3, 1, 1, (8, 16)), Bk(2, 2, 64, 64, 1, 4, 2, 1, (16, 32)), Bk(2, 3, 64, 128, 1, (3, 8), 1, (1, 3), (8, 16)),
    Bk(2, 2, 1, 64, 1, 3, 1, 1, (16, 32)),                                                           # first audio layer: launched at once
]
MIXED = [WAVE_ALL[0], WAVE_ALL[11], PATCH_ALL[0], PATCH_ALL[5], GATHER_ALL[0], GATHER_ALL[2], WAVE_ALL[10]]
HEADLINE_IDS = ['unet_pre', 'unet_down64', 'unet_up64', 'dec1', 'dec0_bcast', 'pse0', 'cls0', 'd_conv3']
TWICE = [WAVE_ALL[0], WAVE_ALL[11], GATHER_ALL[2], PATCH_ALL[0]]
PREFILL = MIXED + _as('bf16', [H16_ALL[1], H16_ALL[3], H16_ALL[4], H16_ALL[13]])

TABLE = [
    Q('wave_all_kinds', WAVE_ALL, dict(launches=[('wave', 12)], kinds=[2, 3, 4, 5, 6, 7, 2, 2, 2, 5, 6, 2], splits1=1, slabs=1),
      'every instance of wgrad_wave_multi_kernel (wave_kind 2..7: stride x tile arrangement, ragged dy rows, upsample-add input), 1-D and '
      '2-D, grouped and shared-input layers, in ONE launch whose job table holds twelve jobs; the last block (48 column / row tiles) '
      'writes dw itself (accumulate = 1), the others leave slabs.  (The eleven layers of the issue plus that block: a B = 2, T = 16 '
      'layer has one pixel tile and goes to the gather kernel, plan_wgrad_patch needs four.)'),
    Q('wave_rollover', [Bk(1, 16, 24, 72, 1, 3, 1, 1, (16,)) for _ in range(50)], dict(launches=[('wave', 48), ('wave', 2)]),
      '50 jobs of one instance: wgrad_patch_flush rolls over at WGP_MAX_JOBS = 48 (B = 16: four pixel tiles, the planner\'s floor)'),
    Q('patch_instances', PATCH_ALL,
      dict(launches=[(('patch', 1, 3, 1, 64, 0), 2), (('patch', 1, 3, 1, 32, 0), 1), (('patch', 1, 4, 1, 16, 0), 1), (('patch', 1, 3, 1, 32, 1), 1)],
           families=['patch'] * 5 + ['c1']),
      'the layers the lean kernel refuses (Kg < 64, rows not 16-byte aligned, 1 x 4 stride 1, few channels on an upsample-add input): '
      'wgrad_patch_multi_kernel, one launch per (kernel shape, tile width, input form); the single-input-channel block launches at once'),
    Q('gather_shapes', GATHER_ALL, dict(launches=[(('gather', 0), 2), (('gather', 1), 1), (('gather', 2), 1), (('gather', 3), 2)]),
      'wgrad_multi_kernel (fewer than 16 output frames): kernel shapes 0..3, a workgroup rebuilds (gx, gy, bz) from its flat id.  Shape 4 '
      '(an upsample-add input under a kernel other than 1 x 3) has no block: ops.conv_block accepts the upsample-add input for any kernel, '
      'but the model only builds k3 up-path blocks and plan / dgrad coverage of other kernels on that input is not claimed anywhere'),
    Q('gather_rollover', [Bk(1, 2, 64, 64, 1, 3, 1, 1, (4,)) for _ in range(26)], dict(launches=[(('gather', 1), 24), (('gather', 1), 2)], splits1=26),
      '26 jobs of one shape: wgrad_gather_flush rolls over at WG_MAX_JOBS = 24; every job adds into dw itself'),
    Q('mixed_families', MIXED, dict(families=['wave', 'wave', 'patch', 'c1', 'gather', 'gather', 'wave']),
      'one backward pass holding blocks of all three fp32 families: ms_wgrad_flush drains three queues'),
    Q('headline_mix', [_from_dispatch(i) for i in HEADLINE_IDS], dict(families=['wave'] * 7 + ['gather'], slabs=5, splits1=2),
      'the production layers at B = 32 under the batched planner\'s splits (g_wgrad_batched), which the dispatch table never runs'),
    Q('h16_all@bf16', _as('bf16', H16_ALL), dict(families=['h16'] * 13 + ['c1_16']),
      'wgrad16_multi_kernel: every taps / input-form instance; blocks of up to 3 slots run on the 5-slot instance when queued'),
    Q('h16_all@fp16', _as('fp16', H16_ALL), dict(families=['h16'] * 13 + ['c1_16']), 'the same in fp16'),
    Q('h16_rollover', _as('bf16', [Bk(1, 2, 64, 64, 1, 3, 1, 1, (16,)) for _ in range(22)]),
      dict(launches=[(('h16', 'bf16', 3, 0, 5), 20), (('h16', 'bf16', 3, 0, 5), 2)]), '22 jobs of one instance: wgrad16_flush rolls over at WG16_MAX_JOBS = 20'),
    Q('used_twice@fp32', TWICE, dict(families=['wave', 'wave', 'gather', 'patch']),
      'one module applied to two inputs in one backward pass: the second use writes temporaries that a later reduction round adds', twice=True),
    Q('used_twice@bf16', _as('bf16', [H16_ALL[1], H16_ALL[4], H16_ALL[8]]), dict(families=['h16'] * 3), 'the same in bf16', twice=True),
    Q('prefilled_slot', PREFILL, dict(splits1=2, slabs=2),
      'queued writes ADD: with the gradient buffer pre-filled, every queued block\'s slot is the pattern plus its gradient, bit for bit'),
]
BY_ID = {e['id']: e for e in TABLE}

# ---- ms_wgrad_reduce_multi called directly: (id, [(n, splits, out offset in floats)]) -----------------------------------------------------
REDUCE_CASES = (
    [('splits%d' % s, [(1000, s, 0)]) for s in (1, 7, 8, 9, 31, 32, 33, 64, 65)] +
    [('n%d_splits32' % n, [(n, 32, 0)]) for n in (1, 3, 4, 5, 65536, 65537)] +
    [('n524292_splits2', [(524292, 2, 0)]), ('out_offset_1', [(1000, 7, 1)]), ('jobs97', [(8 + i % 5, 1 + i % 4, 0) for i in range(97)]),
     ('jobs0', [])])


def check_want(e):
  """The hand-typed purpose of an entry against its computed claims -> list of misses (empty: the shapes reach their branches)."""
  c, w, miss = e['claims'], e['want'], []
  if 'launches' in w:
    norm = lambda q: q if isinstance(q, tuple) else (q,)
    got = sorted((l['queue'], l['jobs']) for l in c['launches'])
    if got != sorted((norm(q), n) for q, n in w['launches']):
      miss.append(('launches', got))
  if 'kinds' in w and [b['kind'] for b in c['blocks'] if b['family'] == 'wave'] != w['kinds']:
    miss.append(('kinds', [b['kind'] for b in c['blocks']]))
  if 'families' in w and [b['family'] for b in c['blocks']] != w['families']:
    miss.append(('families', [b['family'] for b in c['blocks']]))
  if sum(1 for b in c['blocks'] if b['queued'] and b['splits'] == 1) < w.get('splits1', 0):
    miss.append(('splits1', [b['splits'] for b in c['blocks']]))
  if sum(1 for b in c['blocks'] if b['queued'] and b['splits'] > 1) < w.get('slabs', 0):
    miss.append(('slabs', [b['splits'] for b in c['blocks']]))
  return miss


assert all(re.compile(rx) for e in TABLE for rx in e['expect'] + e['forbid'])
