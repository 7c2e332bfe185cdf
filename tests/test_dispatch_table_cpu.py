"""CPU guard of the dispatch table (tests/helpers/dispatch_table.py): every launch-label family of csrc/*.hip is run by a parity
case of tests/test_gpu_dispatch_parity.py or excluded with a reason, and every label regex of the table can match a label some
TimingScope of the sources prints -- so a kernel or launcher added without a parity case, or a table entry left behind by a
renamed label, fails without a GPU."""
import glob
import os
import re

from helpers.dispatch_table import EXCLUDED, TABLE

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mix_stage_amd', 'csrc')
SPEC = re.compile(r'%[-+ #0]*\d*(?:\.(\d+))?(hh|h|ll|l|z|j|t)?([diouxXfeEgGsc%])')
CUT = '< |'            # a family is the label text before the first of these


def _split_args(text):
  """Top-level comma-separated arguments of a call's argument text (strings and brackets respected)."""
  args, depth, cur, i = [], 0, '', 0
  while i < len(text):
    c = text[i]
    if c == '"':
      j = i + 1
      while text[j] != '"':
        j += 2 if text[j] == '\\' else 1
      cur += text[i:j + 1]
      i = j + 1
      continue
    if c in '([{':
      depth += 1
    elif c in ')]}':
      depth -= 1
    if c == ',' and depth == 0:
      args.append(cur.strip()); cur = ''
    else:
      cur += c
    i += 1
  args.append(cur.strip())
  return args


def _literals(expr):
  return [bytes(s, 'utf-8').decode('unicode_escape') for s in re.findall(r'"((?:[^"\\]|\\.)*)"', expr)]


def timing_formats():
  """-> [(file:line, format, [the string literals a %s argument can take, or None per conversion])] for every TimingScope."""
  out = []
  for path in sorted(glob.glob(os.path.join(CSRC, '*.hip'))):
    src = open(path).read()
    for m in re.finditer(r'\bTimingScope\s+\w+\s*\(', src):
      i, depth = m.end(), 1
      while depth:
        c = src[i]
        if c == '"':
          i += 1
          while src[i] != '"':
            i += 2 if src[i] == '\\' else 1
        elif c == '(':
          depth += 1
        elif c == ')':
          depth -= 1
        i += 1
      args = _split_args(src[m.end():i - 1])
      where = '%s:%d' % (os.path.basename(path), src.count('\n', 0, m.start()) + 1)
      fmts = _literals(args[3])
      assert fmts, '%s: no format string literal' % where
      for fmt in fmts:
        conv = [sm for sm in SPEC.finditer(fmt) if sm.group(3) != '%']
        choices = []
        for n, sm in enumerate(conv):
          lits = _literals(args[4 + n]) if sm.group(3) == 's' and 4 + n < len(args) else []
          choices.append(lits or None)
        out.append((where, fmt, choices))
  return out


def _tokens(fmt, choices):
  """The format as a list of regex pieces: one per literal character, one per conversion."""
  toks, pos, n = [], 0, 0
  for sm in SPEC.finditer(fmt):
    toks += [re.escape(c) for c in fmt[pos:sm.start()]]
    pos = sm.end()
    kind = sm.group(3)
    if kind == '%':
      toks.append('%')
      continue
    ch = choices[n]; n += 1
    if kind == 's':
      toks.append('(?:%s)' % '|'.join(re.escape(c) for c in ch) if ch else '.*')
    elif kind in 'fFeEgG':
      toks.append(r'-?\d+' if sm.group(1) == '0' else r'-?[\d.eE+-]+')
    else:
      toks.append(r'-?\d+')
  toks += [re.escape(c) for c in fmt[pos:]]
  return toks


def _families(fmt, choices):
  """The family keys a format can print: its text up to the first '<', ' ' or '|', with every choice of a %s argument there."""
  keys = {''}
  pos, n = 0, 0
  for sm in list(SPEC.finditer(fmt)) + [None]:
    lit = fmt[pos:sm.start() if sm else len(fmt)]
    cut = min([lit.index(c) for c in CUT if c in lit] or [len(lit)])
    keys = {k + lit[:cut] for k in keys}
    if cut < len(lit) or sm is None:
      return keys
    if sm.group(3) == '%':
      keys = {k + '%' for k in keys}
    else:
      ch = choices[n] if sm.group(3) == 's' else None
      n += 1
      if not ch:
        return keys
      nk = set()
      for k in keys:
        for c in ch:
          cc = min([c.index(x) for x in CUT if x in c] or [len(c)])
          nk.add(k + c[:cc])
      keys = nk
      if any(x in ''.join(ch) for x in CUT):
        return keys
    pos = sm.end()
  return keys


def _regex_head(rx):
  """The literal text an anchored label regex starts with (up to its first metacharacter)."""
  assert rx.startswith('^'), 'label regexes are anchored: %r' % rx
  out, i = '', 1
  while i < len(rx):
    c = rx[i]
    if c == '\\':
      if i + 1 >= len(rx) or rx[i + 1].isalnum():
        break
      c = rx[i + 1]
      i += 1
    elif c in '.^$*+?()[]{}|':
      if c in '*?{' and out:
        out = out[:-1]
      break
    out += c
    i += 1
  return out


def _fits(head, toks):
  """Can some label printed by this format start with `head`?"""
  r = ''
  for t in reversed(toks):
    r = '(?:%s%s)?' % (t, r)
  return re.fullmatch(r, head) is not None


def _family_of_head(head):
  cut = min([head.index(c) for c in CUT if c in head] or [len(head)])
  return head[:cut] if cut < len(head) else None


FORMATS = timing_formats()


def test_sources_have_timing_labels():
  assert len(FORMATS) > 60
  fams = set().union(*(_families(f, ch) for _, f, ch in FORMATS))
  for k in ('conv_patch_kernel', 'bn_bwd_fused4', 'bn_bwd_fused', 'act_bwd_fused', 'bn_finalize_apply', 'conv16_kernel', 'ew'):
    assert k in fams, sorted(fams)


def test_every_label_regex_fits_a_timing_format():
  stale = []
  for e in TABLE:
    assert e['expect'], '%s: an entry names the launch(es) it exists for' % e['id']
    for rx in e['expect'] + e['forbid']:
      re.compile(rx)
      head = _regex_head(rx)
      fam = _family_of_head(head)
      ok = fam is not None and any(fam in _families(f, ch) and _fits(head, _tokens(f, ch)) for _, f, ch in FORMATS)
      if not ok:
        stale.append((e['id'], rx, head))
  assert not stale, 'label regexes that no TimingScope format of csrc/*.hip can print: %s' % stale


def test_every_label_family_has_a_parity_case_or_a_reason():
  fam_where = {}
  for where, f, ch in FORMATS:
    for k in _families(f, ch):
      fam_where.setdefault(k, []).append(where)
  covered = set()
  for e in TABLE:
    for rx in e['expect']:
      covered.add(_family_of_head(_regex_head(rx)))
  missing = sorted((k, v) for k, v in fam_where.items() if k not in covered and k not in EXCLUDED)
  assert not missing, 'launch-label families without a parity case in tests/helpers/dispatch_table.py: %s' % missing
  stale = sorted(k for k in EXCLUDED if k not in fam_where)
  assert not stale, 'exclusions of families no source prints: %s' % stale
  both = sorted(k for k in EXCLUDED if k in covered)
  assert not both, 'families both excluded and run by a parity case: %s' % both
  for k, (reason, test) in EXCLUDED.items():
    assert reason and os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), test.split('::')[0])), (k, test)


def test_table_ids_unique_and_cases_well_formed():
  ids = [e['id'] for e in TABLE]
  assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
  for e in TABLE:
    assert e['mode'] in ('BN_TRAIN', 'BN_EVAL', 'LRELU', 'BARE') and e['in_mode'] in ('plain', 'bcast', 'up2'), e['id']
    assert e['prec'] in ('fp32', 'bf16x6', 'bf16', 'fp16') and e['nd'] in (1, 2) and len(e['sp']) == e['nd'], e['id']
    assert not e['knobs'] or e['why'], '%s: a debug knob needs its reason' % e['id']
    assert all(k.startswith('ms_debug_set_') for k in e['knobs']), e['id']
    assert not (e['pair'] and e['prec'] in ('bf16', 'fp16')), e['id']
