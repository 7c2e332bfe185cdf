"""CPU guard of the elementwise case table (tests/helpers/ew_table.py, run on the GPU by tests/test_gpu_ew_parity.py):
  * every `ew|ew_*` launch label a TimingScope of csrc/*.hip can print has a case, and the table names no label the sources lack;
  * every exported ms_* function of include/mixstage.h whose definition (or the static helper it forwards to) opens an `ew|`
    TimingScope is called by a case -- the _ex and plain twins each at least once;
  * the branch every case claims (chunk sizes of the softmax mixture, capped grids, the loop path of the cross entropy, the batch
    chunks and grid rows of the stand-alone BatchNorm) follows from Python mirrors of the launchers' arithmetic, and the constants of
    those mirrors are the ones in the sources -- a changed constant fails here instead of silently moving a case off its branch."""
import os
import re

from helpers import ew_table as T
from helpers.dispatch_table import EXCLUDED
from test_dispatch_table_cpu import CSRC, timing_formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EW_SOURCES = ('elementwise.hip', 'elementwise16.hip', 'adam.hip')
# entry points of adam.hip that the table does not call: the forms of the segmented step with a feature, each exercised against its
# twin by a GPU test file of its own -> (that file, the ops wrapper it has to call)
ADAM_FORMS = {
    'ms_adam_step_segmented_scaled': ('test_gpu_loss_scale.py', 'ops.adam_step_segmented_scaled'),
    'ms_adam_step_segmented_lr': ('test_gpu_lr_schedule.py', 'ops.adam_step_segmented_lr'),
    'ms_adam_step_segmented_scaled_lr': ('test_gpu_lr_schedule.py', 'ops.adam_step_segmented_scaled_lr'),
    'ms_adam_step_segmented_ema': ('test_gpu_ema.py', 'ops.adam_step_segmented_ema'),
}

# every case of the table by name: a case that is removed or renamed fails here (a new case is added to this list with it)
CASE_IDS = '''
mix_headline mix_configs3 mix_infer1024 mix_t96 mix_t40 mix_m1 mix_prime67 mix_old_b3 mix_old_m1 mix_old_m25 mix_old_p7
ce_bct_c8_r2048 ce_bct_c8_r8192 ce_bct_c25_r2048 ce_bct_c25_r8192 ce_bct_c9_r150 ce_nc_c25_r1000 ce_nc_c3_r1025
ce_plain_acc_c25 ce_plain_acc_c8 lp_l1_n1 lp_l2_n1 lp_l1_n2047 lp_l2_n2047 lp_l1_n2048 lp_l2_n2048 lp_l1_n2049 lp_l2_n2049
lp_l1_n212992 lp_l2_n212992 lp_l1_n851968 lp_l2_n851968 lp_l1_n2101249 lp_l2_n2101249 lp_l1_plain_n2049 lp_l2_plain_n2049
lp_pair_n1 lp_pair_n255 lp_pair_n256 lp_pair_n257 lp_pair_n2048 lp_pair_n2049_refused sqnorm_n1 sqnorm_n3 sqnorm_n4
sqnorm_n5 sqnorm_n1023 sqnorm_n2047 sqnorm_n2049 sqnorm_n4095 sqnorm_n4097 sqnorm_n12289 sqnorm_n15000064 adam_seg_n64_one
adam_seg_n64000_chunks adam_seg_big_uneven adam_seg_n64000_nonfinite adam_plain_n64001 adam_plain_big adam_plain_nonorm
lerp_b32_c256_8_15_64 lerp_b32_c256_32_15_256 lerp_b2_c5_8_15_64 lerp_b2_c5_8_7_64 lerp_b2_c5_8_16_64 lerp_b2_c5_32_15_256
lerp_b2_c5_5_3_7 concat_per_clip concat_per_frame velocity_b32_t70_p50 velocity_b32_t33_p7 velocity_b1024_t64_p104
bn_c1_b2047_hw1_w1 bn_c1_b8_hw256_w2 bn_c64_b32_hw64_w1 bn_c64_b3_hw683_w2 bn_c256_b32_hw64_w2 bn_c256_b2_hw16_w1
bn_c1024_b32_hw4_w1 bn_c1100_b5_hw7_w2 bn_c64_b32_hw4096_w2 bn_c7_b1_hw2049_w1 cb8_c1_bf16 cb8_c1_fp16 cb8_c7_bf16
cb8_c7_fp16 cb8_c8_bf16 cb8_c8_fp16 cb8_c9_bf16 cb8_c9_fp16 cb8_c25_bf16 cb8_c25_fp16 cb8_c104_bf16 cb8_c104_fp16
cb8_c256_bf16 cb8_c256_fp16 prestep_b32_feats1 prestep_b32_feats2 prestep_b32_feats3 prestep_b32_feats4 prestep_b32_feats5
prestep_b32_feats6 prestep_b32_feats7 prestep_b1024_feats3 prestep_b1024_feats7 prestep_refusals metrics_b32 metrics_b1024
metrics_refusals copy_multi_11 copy_multi_9_zero_middle
'''.split()


def _src(name):
  return open(os.path.join(CSRC, name)).read()


def _ew_labels():
  """Every label literal starting with `ew|` of a TimingScope (both arms of a ?:) -> where it is."""
  out = {}
  for where, fmt, _ in timing_formats():
    if fmt.startswith('ew|'):
      assert '%' not in fmt, '%s: an ew label with a conversion needs its own handling here: %r' % (where, fmt)
      out.setdefault(fmt, []).append(where)
  return out


def _functions(src):
  """name -> body text of every top-level `int name(...) {` / `static int name(...) {` / `size_t name(...) {` definition."""
  out = {}
  heads = list(re.finditer(r'^(?:static\s+)?(?:inline\s+)?(?:int|size_t)\s+(\w+)\s*\(', src, re.M))
  for m, nxt in zip(heads, heads[1:] + [None]):
    out[m.group(1)] = src[m.end():nxt.start() if nxt else len(src)]
  return out


def _ew_symbols():
  """Exported ms_* functions that open an `ew|` TimingScope themselves or through a static helper of the same file."""
  header = open(os.path.join(ROOT, 'include', 'mixstage.h')).read()
  exported = set(re.findall(r'\b(ms_\w+)\s*\(', header))
  syms = {}
  for name in EW_SOURCES:
    fns = _functions(_src(name))
    opens = {f for f, body in fns.items() if re.search(r'TimingScope\s+\w+\s*\([^;]*"ew\|', body)}
    for f, body in fns.items():
      if not f.startswith('ms_') or f not in exported:
        continue
      if f in opens or any(re.search(r'\b%s\s*\(' % h, body) for h in opens if not h.startswith('ms_')):
        syms[f] = name
  return syms


def test_every_ew_label_has_a_case_and_no_case_names_a_stale_label():
  src_labels = _ew_labels()
  assert len(src_labels) == 34, sorted(src_labels)
  wanted = set()
  for e in T.TABLE:
    wanted.update(e['labels'])
  missing = sorted((l, w) for l, w in src_labels.items() if l not in wanted)
  assert not missing, 'ew launch labels without a case in tests/helpers/ew_table.py: %s' % missing
  all_fmts = [fmt for _, fmt, _ in timing_formats()]
  stale = sorted(l for l in wanted if l not in src_labels and not (not l.startswith('ew|') and any(f.startswith(l) for f in all_fmts)))
  assert not stale, 'labels of the table that no TimingScope prints: %s' % stale
  for e in T.TABLE:
    for l in e['forbid']:
      assert any(s.startswith(l) for s in src_labels), (e['id'], l)


def test_every_ew_entry_point_is_called_by_a_case():
  syms = _ew_symbols()
  for must in ('ms_adam_step', 'ms_adam_step_segmented', 'ms_lp_mean_fwd_ex', 'ms_l1_mean_fwd', 'ms_l2_mean_bwd', 'ms_cross_entropy_fwd',
               'ms_cross_entropy_bwd_ex', 'ms_cb8_from_btc', 'ms_sqnorm', 'ms_lp_mean_pair_bwd', 'ms_bn_bwd_apply'):
    assert must in syms, (must, sorted(syms))
  called = set()
  for e in T.TABLE:
    called.update(e['symbols'])
  assert set(ADAM_FORMS) <= set(syms), sorted(syms)
  for sym, (test, wrapper) in ADAM_FORMS.items():
    path = os.path.join(ROOT, 'tests', test)
    assert syms[sym] == 'adam.hip' and os.path.exists(path), (sym, test)
    assert re.search(r'\b%s\b\s*[()]' % re.escape(wrapper), open(path).read()), '%s does not call %s' % (test, wrapper)
  missing = sorted(s for s in syms if s not in called and s not in ADAM_FORMS)
  assert not missing, 'C-ABI entry points behind an ew| TimingScope that no case calls: %s' % missing
  header = open(os.path.join(ROOT, 'include', 'mixstage.h')).read()
  unknown = sorted(s for s in called if not re.search(r'\b%s\s*\(' % s, header))
  assert not unknown, 'symbols of the table that include/mixstage.h does not declare: %s' % unknown


def test_mirror_constants_are_the_ones_in_the_sources():
  s = _src('elementwise.hip')
  fns = _functions(s)

  def one(rx, text=s):
    m = re.findall(rx, text)
    assert len(m) >= 1, rx
    assert len(set(m)) == 1, (rx, m)
    return int(m[0])

  assert one(r'#define RED_MAX_BLOCKS (\d+)') == T.RED_MAX_BLOCKS
  assert one(r'#define MIX_TT (\d+)') == T.MIX_TT
  assert re.search(r'\(n \+ 256 \* 8 - 1\) / \(256 \* 8\)', fns['red_blocks']) and T.RED_PER_BLOCK == 256 * 8
  assert 'b > RED_MAX_BLOCKS' in fns['red_blocks']
  mix = fns['ms_softmax_mix_fwd']
  assert one(r'std::min\(P, (\d+) / std::max\(1, tiles\)\)', mix) == T.MIX_WG_TARGET
  assert 'cdiv(T, MIX_TT) * B' in mix and 'fc = cdiv(P, nch)' in mix and 'nch = cdiv(P, fc)' in mix
  for fn, rx in (('ms_znorm_select', r'\(rows \* PK \+ 255\) / 256, (\d+)\)'), ('ms_concat_style_fwd', r'\(total \+ 255\) / 256, (\d+)\)'),
                 ('ms_concat_style_bwd', r'\(total \+ 255\) / 256, (\d+)\)')):
    assert one(rx, fns[fn]) == T.EW_BLOCK_CAP, fn
  adam = _src('adam.hip')
  m = re.findall(r'\(n \+ (\d+)\) / (\d+), (\d+)\)', adam)          # the one grid of both element passes
  assert len(m) == 1 and m == re.findall(r'\(n \+ (\d+)\) / (\d+), (\d+)\)', _functions(adam)['adam_blocks']), m
  assert int(m[0][0]) + 1 == int(m[0][1]) == T.ADAM_PER_BLOCK and int(m[0][2]) == T.EW_BLOCK_CAP
  assert s.count('if (C <= 8)') == 1 and T.CE_REG_MAX == 8
  for fn in ('ms_lp_mean_pair_fwd', 'ms_lp_mean_pair_bwd'):
    assert one(r'n > (\d+)\)', fns[fn]) == T.LP_PAIR_MAX, fn
  assert re.search(r'std::min\(64, \(B \* HW \+ 2047\) / 2048\)', fns['ms_bn_bwd_apply']) and T.BN_GY_MAX == 64
  assert re.search(r'C >= 1024 \? 1 : \(1024 \+ C - 1\) / C', fns['bwd_chunks'])
  assert one(r'COPY_MULTI_MAX = (\d+)') == T.COPY_MULTI_MAX
  # the norm kernel and the segmented Adam's element pass: the alignment tests the offset-by-one-float cases rely on
  assert s.count('& 15) == 0') >= 3
  assert '((size_t)p | (size_t)g | (size_t)m | (size_t)v | (EMA ? (size_t)e : (size_t)0)) & 15) == 0' in adam


def test_mirrors_against_hand_computed_values():
  assert T.mix_chunks(32, 104, 64) == (15, 7, 6)
  assert T.mix_chunks(32, 104, 256) == (4, 26, 26)
  assert T.mix_chunks(1024, 104, 64) == (1, 104, 104)
  assert T.mix_chunks(3, 104, 64) == (104, 1, 1)
  assert [T.bwd_chunks(4096, C)[2] for C in (1, 64, 256, 1024, 1100)] == [1024, 16, 4, 1, 1]
  assert [T.bn_apply_gy(1, n) for n in (2047, 2048, 2049, 131072, 1 << 20)] == [1, 1, 2, 64, 64]
  assert [T.red_blocks(n) for n in (1, 2048, 2049, 212992, 851968, 1024 * 2048 + 1)] == [1, 1, 2, 104, 416, 1024]
  assert T.adam_blocks(64) == 1 and T.adam_blocks(2048 * 1024 + 1) == 2048


def test_every_case_reaches_the_branch_it_claims():
  ids = [e['id'] for e in T.TABLE]
  assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
  assert ids == CASE_IDS, 'cases missing from the table: %s; cases not listed in CASE_IDS: %s' % (sorted(set(CASE_IDS) - set(ids)), sorted(set(ids) - set(CASE_IDS)))
  for e in T.TABLE:
    p, c = e['p'], e['claims']
    assert e['why'] and e['bar'] in ('exact', 'round', 'fp32', 'derived') and e['symbols'] and e['via'], e['id']
    assert e['labels'] or e['op'].endswith('_refused'), e['id']
    if e['op'] == 'softmax_mix':
      assert (c['nch'], c['fc'], c['last']) == T.mix_chunks(p['B'], p['P'], p['T']), e['id']
    elif e['op'] == 'cross_entropy':
      rows = 1
      for v in p['shape']:
        rows *= v
      assert c['loop_path'] == (p['C'] > T.CE_REG_MAX) and c['rows'] == rows, e['id']
    elif e['op'] in ('lp_mean', 'sqnorm'):
      assert c['blocks'] == T.red_blocks(p['n']) and c['capped'] == (T.cdiv(p['n'], T.RED_PER_BLOCK) > T.RED_MAX_BLOCKS), e['id']
    elif e['op'] == 'adam':
      assert c['blocks'] == T.adam_blocks(p['n']) and c['capped'] == (T.cdiv(p['n'], T.ADAM_PER_BLOCK) > T.EW_BLOCK_CAP), e['id']
      assert c['two_passes'] == (p['n'] // 4 > 2 * T.EW_BLOCK_CAP * 256), e['id']
      assert not p['segmented'] or p['n'] % 64 == 0, e['id']
    elif e['op'] == 'bn_trio':
      nchunk, bpc, want = T.bwd_chunks(p['B'], p['C'])
      assert (c['want'], c['nchunk'], c['bpc'], c['gy']) == (want, nchunk, bpc, T.bn_apply_gy(p['B'], p['HW'])), e['id']
    elif e['op'] == 'concat':
      assert c['fwd_capped'] == (T.cdiv(p['B'] * (p['C'] + p['D']) * p['T'], 256) > T.EW_BLOCK_CAP), e['id']
      assert c['dx_capped'] == (T.cdiv(p['B'] * p['C'] * p['T'], 256) > T.EW_BLOCK_CAP), e['id']
    elif e['op'] == 'prestep':
      assert c['znorm_capped'] == (T.cdiv(p['B'] * p['T'] * 96, 256) > T.EW_BLOCK_CAP), e['id']
    elif e['op'] in ('lp_pair', 'lp_pair_refused'):
      assert c['taken'] == (p['n'] <= T.LP_PAIR_MAX), e['id']
    elif e['op'] == 'cb8':
      assert c['C8'] == T.cdiv(p['C'], 8) and c['ragged'] == (p['C'] % 8 != 0), e['id']

  by = T.BY_ID
  # the branches the table exists for, by name (a renamed or removed case fails here)
  assert (by['mix_headline']['claims']['fc'], by['mix_headline']['claims']['nch'], by['mix_headline']['claims']['last']) == (7, 15, 6)
  assert by['mix_configs3']['claims']['fc'] == 26 and by['mix_infer1024']['claims'] == dict(nch=1, fc=104, last=104)
  assert by['mix_t96']['claims']['fc'] > 1 and by['mix_t96']['p']['T'] % 64 and by['mix_t40']['claims']['fc'] > 1 and by['mix_t40']['p']['T'] < 64
  assert by['mix_prime67']['claims']['last'] < by['mix_prime67']['claims']['fc']
  assert all(by[k]['claims']['fc'] == 1 for k in ('mix_old_b3', 'mix_old_m1', 'mix_old_m25', 'mix_old_p7'))
  assert by['ce_bct_c9_r150']['claims']['loop_path'] and not by['ce_bct_c8_r8192']['claims']['loop_path']
  assert by['ce_bct_c25_r8192']['claims'] == dict(loop_path=True, rows=8192) and by['ce_nc_c25_r1000']['claims']['rows'] % 64
  assert by['lp_l1_n2101249']['claims']['capped'] and by['lp_l2_n2101249']['claims']['capped'] and not by['lp_l1_n851968']['claims']['capped']
  assert by['sqnorm_n15000064']['claims']['capped'] and by['sqnorm_n2049']['claims']['blocks'] == 2
  assert by['adam_seg_big_uneven']['claims'] == dict(blocks=2048, capped=True, two_passes=True)
  assert by['adam_plain_big']['claims']['capped'] and not by['adam_seg_n64000_chunks']['claims']['capped']
  assert by['concat_per_clip']['claims']['fwd_capped'] and by['concat_per_frame']['claims'] == dict(fwd_capped=True, dx_capped=True)
  wants = {e['claims']['want'] for e in T.TABLE if e['op'] == 'bn_trio'}
  gys = {e['claims']['gy'] for e in T.TABLE if e['op'] == 'bn_trio'}
  assert {1024, 16, 4, 1} <= wants and {1, 2, 64} <= gys
  bn = [e for e in T.TABLE if e['op'] == 'bn_trio']
  assert {e['p']['B'] * e['p']['HW'] for e in bn} >= {2047, 2048, 2049, 131072} and {e['p']['world'] for e in bn} == {1, 2}
  assert any(e['p']['B'] < e['claims']['want'] for e in bn) and any(e['p']['B'] > e['claims']['want'] for e in bn)
  assert {e['p']['feats'] for e in T.TABLE if e['op'] == 'prestep'} == set(range(1, 8))
  assert {e['p']['B'] for e in T.TABLE if e['op'] == 'prestep'} == {32, 1024} == {e['p']['B'] for e in T.TABLE if e['op'] == 'metrics'}
  assert any(e['claims']['znorm_capped'] for e in T.TABLE if e['op'] == 'prestep')
  assert {(e['p']['C'], e['p']['dt']) for e in T.TABLE if e['op'] == 'cb8'} == {(C, d) for C in (1, 7, 8, 9, 25, 104, 256) for d in ('bf16', 'fp16')}


def test_dispatch_table_points_at_the_ew_parity_test():
  reason, test = EXCLUDED['ew']
  assert reason and test == 'test_gpu_ew_parity.py'
  assert os.path.exists(os.path.join(ROOT, 'tests', test))
