"""CPU: every plan class the 16-bit planners can pick for the models' blocks has a test shape.  tests/helpers/conv16_plan_host.cpp
(csrc/conv16_plan.h built with the host compiler under the address and undefined-behaviour sanitizers, as test_job_queue_cpu.py
builds its helper) plans the whole domain of tests/helpers/conv16_plan_table.py, the shapes other tests already run (dispatch_table.B16,
fp16_block_table.TABLE, CASES_1D / CASES_2D of test_gpu_kernels16.py) and the table's entries; a class or an (instance, ragged bit)
pair of the domain that none of them reaches fails here by name.  A threshold that moves in the planner moves the classes: the
new ones show up as missing.  `pytest -s` prints the counts and the classes on the K loop's run-time wait path."""
import os
import re
import shutil
import subprocess

import pytest

from helpers import conv16_plan_table as T
from helpers import dispatch_table as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, 'mix_stage_amd', 'csrc')


def _compiler():
  found = [shutil.which(c) for c in ('g++', 'clang++', 'c++')] + [p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++') if os.path.exists(p)]
  return next((c for c in found if c), None)


def build_program(path):
  cxx = _compiler()
  if cxx is None:
    return None
  subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                  '-I', CSRC, '-I', os.path.join(ROOT, 'include'), os.path.join(HERE, 'helpers', 'conv16_plan_host.cpp'), '-o', path], check=True)
  return path


def plan(program, geos):
  """[geometry] -> [{'fwd' | 'dgrad' | 'wgrad': fields}] as the host program plans them."""
  text = '\n'.join(T.host_line('g%d' % i, g) for i, g in enumerate(geos)) + '\n'
  r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
  got = T.parse_host(r.stdout)
  return [got['g%d' % i] for i in range(len(geos))]


@pytest.fixture(scope='module')
def program(tmp_path_factory):
  exe = build_program(str(tmp_path_factory.mktemp('conv16_plan') / 'conv16_plan_host'))
  if exe is None:
    pytest.skip('no C++ compiler on this machine')
  return exe


@pytest.fixture(scope='module')
def world(program):
  """The domain's classes and ragged pairs, what the existing shapes reach, what each entry reaches."""
  dom = T.domain()
  classes, ragged, refused = {}, {}, []
  for (g, fwd_only), pl in zip(dom, plan(program, [g for g, _ in dom])):
    if not pl['fwd']['ok'] or (not fwd_only and not (pl['dgrad']['ok'] and pl['wgrad']['ok'])):
      refused.append(g)
      continue
    for w in ('fwd',) if fwd_only else ('fwd', 'dgrad'):      # the table and the host program read the literal counts from one list
      assert T.run_time_wait(T.conv_class(w, pl[w])) == (pl[w]['form'] in ('run', 'over')), (g, w, pl[w])
    for c in T.classes_of(pl, fwd_only):
      classes.setdefault(c, g)
    for r in T.ragged_of(pl, fwd_only):
      ragged.setdefault(r, g)
  ex = T.existing_shapes()
  ex_classes, ex_ragged = set(), set()
  for (_, _, fwd_only), pl in zip(ex, plan(program, [g for _, g, _ in ex])):
    ex_classes.update(T.classes_of(pl, fwd_only))
    ex_ragged.update(T.ragged_of(pl, fwd_only))
  entries = {c['id']: pl for c, pl in zip(T.ENTRIES, plan(program, [T.geometry(c) for c in T.ENTRIES]))}
  return dict(classes=classes, ragged=ragged, refused=refused, ex_classes=ex_classes, ex_ragged=ex_ragged, entries=entries)


def test_builder_reproduces_the_dispatch_tables_geometries():
  """The domain's builder against the hand-written lists: the headline model at (M, T, B) = (8, 64, 32) block for block, and the
  T = 256 geometries of configs[3] at (25, 256, 32)."""
  geos = lambda blocks: {T.geometry(b) for b in blocks}
  assert geos(T.model_blocks(8, 64, 32)) == geos(e for e in D.HEADLINE if not e['pair'])
  assert geos(D.C4) <= geos(T.model_blocks(25, 256, 32))
  b16 = geos(e for e in D.B16 if e['B'] == 32)
  assert b16 <= geos(T.model_blocks(8, 64, 32)) | geos(T.model_blocks(4, 64, 32)) | geos(T.model_blocks(25, 256, 32))


def test_no_domain_shape_is_refused(world):
  assert not world['refused'], world['refused'][:8]


def test_every_plan_class_of_the_domain_has_a_shape(world):
  named = {c for e in T.ENTRIES for c in e['classes']}
  missing = {c: g for c, g in world['classes'].items() if c not in world['ex_classes'] and c not in named}
  assert not missing, 'plan classes no test shape reaches (class: a domain shape in it): %s' % missing
  run_time = sorted(c for c in world['classes'] if T.run_time_wait(c))
  conv = [c for c in world['classes'] if not c.startswith('wgrad')]
  new = sorted(c for c in world['classes'] if c not in world['ex_classes'])
  print('\nplan classes: %d (conv16 %d, wgrad16 %d); reached by no shape outside this table: %d, of them on the run-time wait path: %d'
        % (len(world['classes']), len(conv), len(world['classes']) - len(conv), len(new), sum(T.run_time_wait(c) for c in new)))
  print('classes on the run-time wait path (%d):' % len(run_time))
  for c in run_time:
    print('  %s%s' % (c, '' if c in world['ex_classes'] else '   [this table only]'))
  # the figures of the table's docstring are these
  doc = T.__doc__
  assert re.search(r'^%d plan classes' % len(world['classes']), doc, re.M) and '%d on the run-time wait path' % len(run_time) in doc, \
      (len(world['classes']), len(run_time))


def test_every_ragged_bit_of_every_instance_has_a_shape(world):
  named = {tuple(r) for e in T.ENTRIES for r in e['ragged']}
  missing = {r: g for r, g in world['ragged'].items() if r not in world['ex_ragged'] and r not in named}
  assert not missing, 'ragged edges of a kernel instance no test shape has ((instance, bit): a domain shape with it): %s' % missing


@pytest.mark.parametrize('c', T.ENTRIES, ids=[c['id'] for c in T.ENTRIES])
def test_entry_lands_where_it_says(world, c):
  pl = world['entries'][c['id']]
  assert pl['fwd']['ok'] and pl['dgrad']['ok'] and pl['wgrad']['ok'], pl
  got_c, got_r = set(T.classes_of(pl)), set(T.ragged_of(pl))
  assert set(c['classes']) <= got_c, (sorted(set(c['classes']) - got_c), sorted(got_c))
  assert {tuple(r) for r in c['ragged']} <= got_r, (sorted({tuple(r) for r in c['ragged']} - got_r), sorted(got_r))
  # an entry is there for something the domain has and no other shape reaches
  assert c['classes'] or c['ragged']
  assert all(k in world['classes'] and k not in world['ex_classes'] for k in c['classes'])
  assert all(tuple(r) in world['ragged'] and tuple(r) not in world['ex_ragged'] for r in c['ragged'])
  # the mode is the populating model layer's, LeakyReLU for a shape that is no model layer
  assert c['mode'] == ('LRELU' if c['layer'] is None else c['mode']) and len({e['id'] for e in T.ENTRIES}) == len(T.ENTRIES)
