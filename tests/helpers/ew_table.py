"""The case table of the elementwise / loss / optimizer entry points (launch labels `ew|ew_*` of csrc/elementwise.hip and
csrc/elementwise16.hip, plus the two cb8 <-> plain converters that every 16-bit test builds its inputs with).

One entry per case, in the style of dispatch_table.py:
  id       unique name
  op       the runner of tests/test_gpu_ew_parity.py that executes the case
  labels   launch labels the case MUST produce (a label of a launch that starts with one of these strings)
  forbid   launch labels the case must NOT produce (refused calls launch nothing)
  symbols  the C-ABI functions of include/mixstage.h the case goes through
  via      the Python wrapper used ('lib' = the ctypes symbol itself)
  bar      'exact' | 'round' | 'fp32' (a fixed bar that an existing test of the entry point already set) | 'derived' (4 x the error
           of torch's float32 CPU evaluation of the same formula against the float64 reference, floored at 2 * 2^-24)
  claims   the branch of the launcher / kernel the case exists for, as numbers that tests/test_ew_table_cpu.py recomputes from
           the mirrors below (which it ties to the constants in the sources by regex)
  why      the same in words, with file:line of csrc/elementwise.hip (E:), csrc/elementwise16.hip (E16:) or csrc/adam.hip (A:)
  p        the shape parameters of the runner

The mirrors restate the launchers' grid arithmetic; the CPU guard fails if a constant they use changes in the sources."""

RED_MAX_BLOCKS = 1024          # E:1175
RED_PER_BLOCK = 256 * 8        # E:1409 red_blocks
MIX_TT = 64                    # E:729
MIX_WG_TARGET = 512            # E:1582
EW_BLOCK_CAP = 2048            # E:1675 znorm, E:1720 / E:1732 concat, A:298 Adam
ADAM_PER_BLOCK = 1024          # A:298
CE_REG_MAX = 8                 # E:1069 `C <= 8`
LP_PAIR_MAX = 2048             # E:1856
BN_GY_MAX = 64                 # E:1403
COPY_MULTI_MAX = 8             # E:1888


def cdiv(a, b):
  return (a + b - 1) // b


def red_blocks(n):
  return max(1, min(RED_MAX_BLOCKS, cdiv(n, RED_PER_BLOCK)))


def bwd_chunks(B, C):
  """-> (chunks launched, batch items per chunk, `want` before the cap by B)   (E:1210)"""
  want0 = 1 if C >= 1024 else cdiv(1024, C)
  want = max(1, min(want0, B))
  bpc = cdiv(B, want)
  return cdiv(B, bpc), bpc, want0


def bn_apply_gy(B, HW):
  return max(1, min(BN_GY_MAX, (B * HW + 2047) // 2048))        # E:1403


def mix_chunks(B, P, T):
  """-> (nch, fc, features of the last chunk)   (E:1581-1584)"""
  tiles = cdiv(T, MIX_TT) * B
  nch = max(1, min(P, MIX_WG_TARGET // max(1, tiles)))
  fc = cdiv(P, nch)
  nch = cdiv(P, fc)
  return nch, fc, P - (nch - 1) * fc


def adam_blocks(n):
  return max(1, min(EW_BLOCK_CAP, cdiv(n, ADAM_PER_BLOCK)))


def cap_blocks(total):
  return max(1, min(EW_BLOCK_CAP, cdiv(total, 256)))


TABLE = []


def _case(id, op, labels, symbols, via, bar, why, claims=None, forbid=(), **p):
  TABLE.append(dict(id=id, op=op, labels=list(labels), forbid=list(forbid), symbols=list(symbols), via=via, bar=bar, why=why,
                    claims=dict(claims or {}), p=p))


# ------------------------------------------------------------------------------------------------ softmax mixture
_MIX = ('ew|ew_softmax_mix_fwd', 'ew|ew_softmax_mix_bwd')
_MIX_S = ('ms_softmax_mix_fwd', 'ms_softmax_mix_bwd')
for _id, _B, _M, _P, _T, _why in [
    ('headline', 32, 8, 104, 64, 'the headline step: fc = 7, 15 chunks, a short last chunk of 6 (E:1581-1584; tile stride fc + 1 E:762, e / nf E:767)'),
    ('configs3', 32, 25, 104, 256, 'configs[3]: fc = 26, 4 whole chunks; dscore over M = 25 (E:816)'),
    ('infer1024', 1024, 8, 104, 64, 'inference batch: tiles > 512, so ONE chunk of all 104 features (E:1582)'),
    ('t96', 32, 8, 104, 96, 'T not a multiple of 64 with fc = 13: the part-filled second time tile (nt E:765)'),
    ('t40', 32, 8, 104, 40, 'T < 64 with fc = 7: every tile part-filled'),
    ('m1', 32, 1, 104, 64, 'M = 1: softmax identically 1, dscore identically 0'),
    ('prime67', 8, 8, 67, 64, 'a prime P above 512 / tiles: fc = 2, last chunk of 1'),
    ('old_b3', 3, 8, 104, 64, 'case of test_gpu_kernels.test_softmax_mix: fc = 1'),
    ('old_m1', 2, 1, 104, 64, 'case of test_gpu_kernels.test_softmax_mix: fc = 1, M = 1'),
    ('old_m25', 2, 25, 104, 96, 'case of test_gpu_kernels.test_softmax_mix: fc = 1, M = 25, T = 96'),
    ('old_p7', 1, 4, 7, 33, 'case of test_gpu_kernels.test_softmax_mix: fc = 1, P = 7, T = 33'),
]:
  _n, _f, _l = mix_chunks(_B, _P, _T)
  _case('mix_' + _id, 'softmax_mix', _MIX, _MIX_S, 'ops.softmax_mix', 'derived' if (_M == 25 and not _id.startswith('old')) else 'fp32',
        _why, claims=dict(nch=_n, fc=_f, last=_l), B=_B, M=_M, P=_P, T=_T)

# ------------------------------------------------------------------------------------------------ cross entropy
_CE = ('ew|ew_cross_entropy_fwd', 'ew|ew_cross_entropy_bwd')
_CE_EX = ('ms_cross_entropy_fwd_ex', 'ms_cross_entropy_bwd_ex')
_CE_PLAIN = ('ms_cross_entropy_fwd', 'ms_cross_entropy_bwd')
for _id, _lay, _shape, _C, _scale, _acc, _via, _why in [
    ('bct_c8_r2048', 'bct', (32, 64), 8, 'host', 0, 'ops', 'headline label loss: register path, 2 rows per thread of the single workgroup (E:1069)'),
    ('bct_c8_r8192', 'bct', (32, 256), 8, 'host', 0, 'ops', 'register path, 8 rows per thread summed in fp32 (E:1066)'),
    ('bct_c25_r2048', 'bct', (32, 64), 25, 'dev', 0, 'ops', 'M = 25 classes: the loop path (E:1084-1087), device-resident weight'),
    ('bct_c25_r8192', 'bct', (32, 256), 25, 'host', 0, 'ops', 'configs[3]: the loop path at 8192 rows'),
    ('bct_c9_r150', 'bct', (3, 50), 9, 'host', 0, 'ops', 'C = 9, the first size on the loop path; 150 rows: part-filled waves both ways (E:1066, E:1105)'),
    ('nc_c25_r1000', 'nc', (1000,), 25, 'dev', 0, 'ops', '2-D layout (stride_c = 1) on the loop path; 1000 rows: not a multiple of 1024 or 64'),
    ('nc_c3_r1025', 'nc', (1025,), 3, 'host', 0, 'ops', 'register path with C < 8 (clamped loads E:1073); one row beyond the first pass of the 1024 threads'),
    ('plain_acc_c25', 'bct', (5, 37), 25, 'none', 1, 'lib', 'the plain twins (no ms_loss_scale) and accumulate = 1: dscore += (E:1118)'),
    ('plain_acc_c8', 'nc', (777,), 8, 'none', 1, 'lib', 'the plain twins, register path, accumulate = 1'),
]:
  _rows = 1
  for _v in _shape:
    _rows *= _v
  _case('ce_' + _id, 'cross_entropy', _CE, _CE_PLAIN if _via == 'lib' else _CE_EX, 'lib' if _via == 'lib' else 'ops.cross_entropy',
        'derived' if _rows > 2048 else 'fp32', _why, claims=dict(loop_path=_C > CE_REG_MAX, rows=_rows),
        layout=_lay, shape=_shape, C=_C, scale=_scale, accumulate=_acc)

# ------------------------------------------------------------------------------------------------ L1 / MSE mean
for _n in (1, 2047, 2048, 2049, 212992, 851968, 2101249):
  for _sq in (0, 1):
    _nm = 'l2' if _sq else 'l1'
    _case('lp_%s_n%d' % (_nm, _n), 'lp_mean', ('ew|ew_%s_mean_fwd' % _nm, 'ew|ew_%s_mean_bwd' % _nm), ('ms_lp_mean_fwd_ex', 'ms_lp_mean_bwd_ex'),
          'ops.%s_mean' % _nm, 'fp32',
          {1: 'one element', 2047: 'one part-filled partial block', 2048: 'exactly one partial block', 2049: 'two partial blocks',
           212992: 'headline pose loss (32 x 64 x 104): 104 blocks', 851968: 'configs[3] pose loss: 416 blocks',
           2101249: 'above 1024 * 2048: the capped grid, grid-stride loop runs twice (E:1411)'}[_n] + ' (E:1408-1413); with `b` and with `target`',
          claims=dict(blocks=red_blocks(_n), capped=_n > RED_MAX_BLOCKS * RED_PER_BLOCK), n=_n, squared=_sq, plain=False)
for _sq in (0, 1):
  _nm = 'l2' if _sq else 'l1'
  _case('lp_%s_plain_n2049' % _nm, 'lp_mean', ('ew|ew_%s_mean_fwd' % _nm, 'ew|ew_%s_mean_bwd' % _nm), ('ms_%s_mean_fwd' % _nm, 'ms_%s_mean_bwd' % _nm), 'lib',
        'fp32', 'the plain twins ms_%s_mean_fwd / _bwd (no ms_loss_scale), two partial blocks (E:1843-1854)' % _nm,
        claims=dict(blocks=2, capped=False), n=2049, squared=_sq, plain=True)

for _n in (1, 255, 256, 257, 2048):
  _case('lp_pair_n%d' % _n, 'lp_pair', ('ew|ew_l1_mean_pair_fwd', 'ew|ew_l1_mean_pair_bwd', 'ew|ew_l2_mean_pair_fwd', 'ew|ew_l2_mean_pair_bwd'),
        ('ms_lp_mean_pair_fwd', 'ms_lp_mean_pair_bwd'), 'ops.lp_mean_pair', 'fp32',
        'both criterion terms in one launch against fp64, %d values per half: %s (E:1249-1272)'
        % (_n, {1: 'one value', 255: 'a part-filled pass of the 256 threads', 256: 'one whole pass', 257: 'one value in the second pass',
                2048: 'the largest size taken'}[_n]), claims=dict(taken=_n <= LP_PAIR_MAX), n=_n)
_case('lp_pair_n2049_refused', 'lp_pair_refused', (), ('ms_lp_mean_pair_fwd', 'ms_lp_mean_pair_bwd'), 'lib', 'exact',
      'n = 2049 per half: both calls return an error and launch nothing (E:1856, E:1867)', claims=dict(taken=False),
      forbid=('ew|ew_l1_mean_pair', 'ew|ew_l2_mean_pair'), n=2049)

# ------------------------------------------------------------------------------------------------ gradient norm
for _n, _why in [(1, 'tail only'), (3, 'tail only (n % 4 = 3)'), (4, 'one vector, no tail'), (5, 'one vector + tail of 1'), (1023, '255 vectors + tail of 3'),
                 (2047, 'one block, tail of 3'), (2049, 'two blocks: the remainder vector `if (i < n4)` (E:1204)'),
                 (4095, 'two blocks'), (4097, 'three blocks, tail of 1'), (2 * 2048 * 3 + 1, 'seven blocks'),
                 (15000064, 'production scale (the generator\'s flat gradient): 1024 capped blocks, the two-in-flight loop runs 7 times and the remainder vector is taken by part of the grid')]:
  _case('sqnorm_n%d' % _n, 'sqnorm', ('ew|ew_sqnorm',), ('ms_sqnorm',), 'ops.grad_norm', 'derived',
        _why + '; 16-byte-aligned base (E:1192) and a view offset by one float (the unaligned path E:1212)',
        claims=dict(blocks=red_blocks(_n), capped=_n > RED_MAX_BLOCKS * RED_PER_BLOCK), n=_n)

# ------------------------------------------------------------------------------------------------ Adam
# seg: 'one' | 'chunks' (a boundary at every 64-element chunk; first steps 1, 2, 3, -1 (never), 9 (future) in turn) | 'uneven' (37 segments
# of different lengths, the same first steps).  norms: one entry per step: 'in' (clip inactive) | 'clip' (norm > max_norm) | 'inf' | 'nan'
_ADAM_BIG = 2 * 2048 * 1024 + 64 * 1000
for _id, _n, _seg, _norms, _offset, _why in [
    ('n64_one', 64, 'one', ('in', 'clip', 'in'), True, 'one chunk, one segment: 16 vectors, most threads idle'),
    ('n64000_chunks', 64000, 'chunks', ('clip', 'in', 'clip'), True,
     'a segment boundary at every chunk; segments never updated (-1: p, m, v bit-unchanged, A:258) and starting in the future (A:172); per-segment t = step - first + 1 (A:173)'),
    ('big_uneven', _ADAM_BIG, 'uneven', ('in', 'clip', 'clip'), True,
     'above 2 * 2048 * 1024 elements: capped grid, the two-vector loop runs more than once per thread and the second vector of the last pass is partly off the end (A:248-259)'),
    ('n64000_nonfinite', 64000, 'chunks', ('in', 'inf', 'nan', 'clip'), False,
     'norm = inf, then nan: p, m, v bit-unchanged, step_state[2] == 1, step_state[3] counts, the clock advances: the 4th step uses t = 4 (A:202-204)'),
]:
  _case('adam_seg_' + _id, 'adam', ('ew|ew_adam_step_segmented',), ('ms_adam_step_segmented',), 'ops.adam_step_segmented', 'derived',
        _why + ('; the same steps on views offset by one float (scalar fallback A:283) equal the aligned ones bit for bit' if _offset else ''),
        claims=dict(blocks=adam_blocks(_n), capped=_n > EW_BLOCK_CAP * ADAM_PER_BLOCK, two_passes=_n > 2 * EW_BLOCK_CAP * ADAM_PER_BLOCK),
        n=_n, seg=_seg, norms=_norms, offset=_offset, segmented=True)
for _id, _n, _norms, _why in [
    ('n64001', 64001, ('clip', 'in', 'in'), 'the unsegmented step (A:45), n not a multiple of 4'),
    ('big', _ADAM_BIG, ('in', 'clip', 'in'), 'the unsegmented step on the capped grid: grid-stride loop over 2048 blocks'),
    ('nonorm', 1000, ('none', 'none', 'none'), 'norm = NULL: no clipping (A:33)'),
]:
  _case('adam_plain_' + _id, 'adam', ('ew|ew_adam_step',), ('ms_adam_step',), 'ops.adam_step', 'derived', _why,
        claims=dict(blocks=adam_blocks(_n), capped=_n > EW_BLOCK_CAP * ADAM_PER_BLOCK, two_passes=_n > 2 * EW_BLOCK_CAP * ADAM_PER_BLOCK),
        n=_n, seg='one', norms=_norms, offset=False, segmented=False)

# ------------------------------------------------------------------------------------------------ time resize
for _B, _C, _Tin, _F, _Tout, _why in [
    (32, 256, 8, 15, 64, 'the audio encoder\'s own resize at the headline batch: (8, 15) -> 64 steps, 256 channels'),
    (32, 256, 32, 15, 256, 'the same for configs[3] (T = 256)'),
    (2, 5, 8, 15, 64, 'case of test_gpu_kernels.test_lerp_time'), (2, 5, 8, 7, 64, 'case of test_gpu_kernels.test_lerp_time'),
    (2, 5, 8, 16, 64, 'case of test_gpu_kernels.test_lerp_time (even F: two source columns)'),
    (2, 5, 32, 15, 256, 'case of test_gpu_kernels.test_lerp_time'), (2, 5, 5, 3, 7, 'case of test_gpu_kernels.test_lerp_time (ragged)'),
]:
  _case('lerp_b%d_c%d_%d_%d_%d' % (_B, _C, _Tin, _F, _Tout), 'lerp', ('ew|ew_lerp_time_fwd', 'ew|ew_lerp_time_bwd'),
        ('ms_lerp_time_fwd', 'ms_lerp_time_bwd'), 'ops.lerp_time', 'fp32', _why + ' (E:681, E:696)', B=_B, C=_C, Tin=_Tin, F=_F, Tout=_Tout)

# ------------------------------------------------------------------------------------------------ content || style concat
for _id, _T, _per_clip, _why in [
    ('per_clip', 64, True, 'ids as an expanded (B, 1) view (stride 0 in time)'),
    ('per_frame', 65, False, 'ids as a real (B, T) tensor; dx above the cap as well'),
]:
  _case('concat_' + _id, 'concat', ('ew|ew_concat_style_fwd', 'ew|ew_concat_style_bwd'), ('ms_concat_style_fwd', 'ms_concat_style_bwd'),
        'ops.concat_style', 'fp32',
        _why + '; B * (C + D) * T above the 2048-block cap: the grid-stride loops (E:1720, E:1732); S = 25 with one embedding row no clip uses (gradient exactly 0, E:1044)',
        claims=dict(fwd_capped=32 * (256 + 10) * _T > EW_BLOCK_CAP * 256, dx_capped=32 * 256 * _T > EW_BLOCK_CAP * 256),
        B=32, C=256, D=10, T=_T, S=25, per_clip=_per_clip)

# ------------------------------------------------------------------------------------------------ velocity / transposes
for _B, _T, _P, _why in [
    (32, 70, 50, 'T and P not multiples of 32: part-filled 32 x 32 tiles both ways (E:1125, E:1149)'),
    (32, 33, 7, 'one row / few columns beyond a tile'),
    (1024, 64, 104, 'inference batch: blockIdx.z = 1024'),
]:
  _case('velocity_b%d_t%d_p%d' % (_B, _T, _P), 'velocity', ('ew|ew_velocity_fwd', 'ew|ew_velocity_bwd', 'ew|ew_transpose_btc', 'ew|ew_transpose_bct'),
        ('ms_velocity_fwd', 'ms_velocity_bwd', 'ms_transpose_btc', 'ms_transpose_bct'), 'ops.velocity_cm / to_channel_major / to_time_major', 'exact',
        _why + '; one fp32 subtraction per element, so equality with the rounded fp64 result', B=_B, T=_T, P=_P)

# ------------------------------------------------------------------------------------------------ stand-alone BatchNorm (bn_sync)
_BN = ('ew|ew_bn_stats', 'ew|ew_bn_train_apply', 'ew|ew_bn_bwd_sums', 'ew|ew_bn_bwd_apply')
_BN_S = ('ms_bn_stats', 'ms_bn_train_apply', 'ms_bn_bwd_workspace', 'ms_bn_bwd_sums', 'ms_bn_bwd_apply')
for _C, _B, _HW, _world in [(1, 2047, 1, 1), (1, 8, 256, 2), (64, 32, 64, 1), (64, 3, 683, 2), (256, 32, 64, 2), (256, 2, 16, 1), (1024, 32, 4, 1),
                            (1100, 5, 7, 2), (64, 32, 4096, 2), (7, 1, 2049, 1)]:
  _nchunk, _bpc, _want = bwd_chunks(_B, _C)
  _case('bn_c%d_b%d_hw%d_w%d' % (_C, _B, _HW, _world), 'bn_trio', _BN, _BN_S, 'lib', 'derived',
        'want = %d batch chunks (E:1211) with B = %d %s it: %d chunks of %d; B * HW = %d gives gy = %d (E:1403); statistics of %d rank(s) (E:1372), n_global = %d * B * HW (E:1405)'
        % (_want, _B, 'below' if _B < _want else 'at' if _B == _want else 'above', _nchunk, _bpc, _B * _HW, bn_apply_gy(_B, _HW), _world, _world),
        claims=dict(want=_want, nchunk=_nchunk, bpc=_bpc, gy=bn_apply_gy(_B, _HW)), C=_C, B=_B, HW=_HW, world=_world)

# ------------------------------------------------------------------------------------------------ cb8 layout conversions
_CB8 = ('cb8_from_plain_kernel|cb8_from_plain', 'cb8_to_plain_kernel|cb8_to_plain', 'ew|ew_cb8_from_btc', 'ew|ew_cb8_to_btc')
_CB8_S = ('ms_cb8_from_plain', 'ms_cb8_to_plain', 'ms_cb8_from_btc', 'ms_cb8_to_btc')
for _C in (1, 7, 8, 9, 25, 104, 256):
  for _dt in ('bf16', 'fp16'):
    _case('cb8_c%d_%s' % (_C, _dt), 'cb8', _CB8, _CB8_S, 'ops16.to_cb8 / from_cb8 / btc_to_cb8', 'round',
          'C = %d (%s): to_cb8 of arbitrary fp32 equals torch\'s cast -- pack8 is __builtin_convertvector, round to nearest even (conv16_kernel.h:26-29) -- with zero '
          'pad channels (E16:757); from_cb8 and the round trip of representable values exact; btc_to_cb8 with velocity 0 / 1 (fp32 difference rounded once, '
          'E16:798) and its backward dx[t] = dv[t] - dv[t+1] (E16:819); T = 1, T = 37 and a 2-D (5, 7) map'
          % (_C, 'whole channel blocks' if _C % 8 == 0 else 'a part-filled last channel block'),
          claims=dict(C8=cdiv(_C, 8), ragged=_C % 8 != 0), C=_C, dt=_dt, B=3 if _C != 104 else 32, Ts=(1, 37) if _C != 104 else (1, 64))

# ------------------------------------------------------------------------------------------------ pre-step and metrics
for _B in (32, 1024):
  for _feats in range(1, 8):
    if _B == 1024 and _feats not in (3, 7):
      continue
    _case('prestep_b%d_feats%d' % (_B, _feats), 'prestep', ('ew|ew_kmeans_labels', 'ew|ew_znorm_select'), ('ms_kmeans_labels', 'ms_znorm_select'),
          'prestep.DevicePreStep', 'exact',
          'B = %d, feature subset %d of pose | velocity | speed (1 | 2 | 4) (E:1664): labels bit-exact against the fp64 oracle; znorm_select %s (E:1675)'
          % (_B, _feats, 'above the 2048-block cap: grid-stride loop' if _B * 64 * 96 > EW_BLOCK_CAP * 256 else 'below the cap'),
          claims=dict(znorm_capped=_B * 64 * 96 > EW_BLOCK_CAP * 256), B=_B, T=64, M=8 if _feats != 5 else 25, feats=_feats)
_case('prestep_refusals', 'prestep_refused', (), ('ms_kmeans_labels',), 'lib', 'exact',
      'odd PK where speed is asked, feats = 0 and feats = 8 are refused (E:1664): error code, the label buffer stays untouched '
      '(the TimingScope opens before the argument check, so the label itself is still recorded)')
for _B in (32, 1024):
  _case('metrics_b%d' % _B, 'metrics', ('ew|ew_step_metrics', 'ew|ew_eval_accumulate'), ('ms_step_metrics', 'ms_eval_accumulate'),
        'metrics.DeviceStepMetrics / DeviceEvalAccumulators', 'exact',
        'B = %d (one workgroup per clip, E:1687; fid grid (PK, 2), w1 grid (B, 2), E:1701-1708): fp64 accumulators against the fp64 oracle, histograms and hit counts exact' % _B,
        B=_B, T=64)
_case('metrics_refusals', 'metrics_refused', (), ('ms_step_metrics', 'ms_eval_accumulate'), 'lib', 'exact',
      'more than 64 joints (E:1685); PK > P, odd PK, PK < 2 (E:1698): error code, outputs and accumulators untouched')

# ------------------------------------------------------------------------------------------------ batched copies
_case('copy_multi_11', 'copy_multi', ('ew|ew_copy_multi',), ('ms_copy_multi',), 'ops.copy_multi', 'exact',
      'the buffers of test_gpu_kernels.test_copy_multi_any_sizes_and_dtypes: 11 copies in two launches, odd byte counts, unaligned views, int64', kind='old',
      claims=dict(launches=cdiv(11, COPY_MULTI_MAX)))
_case('copy_multi_9_zero_middle', 'copy_multi', ('ew|ew_copy_multi',), ('ms_copy_multi',), 'lib', 'exact',
      '9 buffers (two launches: 8 + 1) with a zero-byte entry in the middle, which is skipped without a gap in block_end (E:1923)', kind='zero_middle',
      claims=dict(launches=cdiv(9, COPY_MULTI_MAX)))

BY_ID = {e['id']: e for e in TABLE}
