"""csrc/job_queue.h without a GPU: tests/helpers/job_queue_host.cpp drives PendingQueue + pack_jobs with the three families'
ordering and predicate, built with the host compiler under the address and undefined-behaviour sanitizers, and the launches it
prints (instance, jobs in order, workgroups, in launch order) must be those of the Python mirror wgrad_queue_table.flush_launches,
which tests/test_gpu_wgrad_queue.py holds to the real kernels' labels.  The workgroup rollover has no shape that reaches it: its
reference is arithmetic on the inputs."""
import os
import re
import shutil
import subprocess

import pytest

from helpers import wgrad_queue_table as T

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'mix_stage_amd', 'csrc')
LIMIT = {'wave': T.WGP_MAX_JOBS, 'patch': T.WGP_MAX_JOBS, 'gather': T.WG_MAX_JOBS, 'h16': T.WG16_MAX_JOBS}


def _compiler():
  found = [shutil.which(c) for c in ('g++', 'clang++', 'c++')] + [p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++') if os.path.exists(p)]
  return next((c for c in found if c), None)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
  cxx = _compiler()
  if cxx is None:
    pytest.skip('no C++ compiler on this machine')
  exe = str(tmp_path_factory.mktemp('job_queue') / 'job_queue_host')
  subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-pthread',
                  '-DWGP_MAX_JOBS=%d' % T.WGP_MAX_JOBS, '-DWG_MAX_JOBS=%d' % T.WG_MAX_JOBS, '-DWG16_MAX_JOBS=%d' % T.WG16_MAX_JOBS,
                  '-I', CSRC, os.path.join(HERE, 'helpers', 'job_queue_host.cpp'), '-o', exe], check=True)
  return exe


# ---- records: what a plan of the mirror (family, queue, length, wgs, queued) looks like to the program ---------------------------------
def J(family, queue, wgs, length=0, queued=True):
  return dict(family=family, queue=queue, wgs=wgs, length=length, queued=queued)


def _key(queue):
  """A mirror's queue key -> (family letter, the six key numbers of job_queue_host.cpp)."""
  if queue[0] == 'wave':
    return 'p', (0, 0, 0, 0, 0, 1)
  if queue[0] == 'patch':
    return 'p', tuple(queue[1:]) + (0,)
  if queue[0] == 'gather':
    return 'g', (queue[1], 0, 0, 0, 0, 0)
  _, prec, tp, up2, npxt = queue
  return 'h', ({'bf16': 0, 'fp16': 1}[prec], tp, up2, npxt, 0, 0)


def _run(program, cases):
  """cases: [(name, queued plans, discard_before)] -> {name: [(family letter, key, [job indices], workgroups)]} as the program packs
  them.  The first `discard_before` jobs are queued, then discarded."""
  text = []
  for name, plans, discard_before in cases:
    text.append('case %s' % name)
    for i, p in enumerate(plans):
      if i == discard_before and i:
        text.append('discard')
      fam, key = _key(p['queue'])
      text.append('%s %d %d %d %d %d %d %d %d' % ((fam,) + key + (p['length'], p['wgs'])))
    text.append('end')
  r = subprocess.run([program], input='\n'.join(text) + '\n', capture_output=True, text=True, timeout=120)
  assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
  got, cur = {}, None
  for line in r.stdout.splitlines():
    if line.startswith('case '):
      cur = got.setdefault(line[5:], [])
    elif line != 'end':
      head, jobs, wgs = line.split('|')
      head = head.split()
      cur.append((head[0], tuple(int(v) for v in head[1:]), [int(v) for v in jobs.split()], int(wgs)))
  assert list(got) == [c[0] for c in cases]
  return got


def _mirror(plans, discard_before=0):
  live = [dict(p, queued=p['queued'] and i >= discard_before) for i, p in enumerate(plans)]
  return [_key(queue) + (idx, sum(plans[i]['wgs'] for i in idx)) for queue, idx in T.flush_launches(live)]


def _queued_only(plans):
  """The queued plans of a table entry, in queue order (the others are launched at once and never reach a queue)."""
  return [p for p in plans if p['queued']]


def _synthetic():
  W, P, G, H = ('wave',), ('patch', 1, 3, 1, 64, 0), ('gather', 1), ('h16', 'bf16', 3, 0, 5)
  one = {'wave': W, 'patch': P, 'gather': G, 'h16': H}
  cases = [('empty', [], 0), ('one_job', [J('gather', G, 7)], 0)]
  for fam, q in one.items():
    for n in (LIMIT[fam], LIMIT[fam] + 1):
      cases.append(('%s_%d_jobs' % (fam, n), [J(fam, q, 3 + i, length=8) for i in range(n)], 0))
    # MAX + 1 jobs of one instance with jobs of another in between: the second launch of the first instance precedes the other's
    other = {'wave': P, 'patch': W, 'gather': ('gather', 3), 'h16': ('h16', 'fp16', 3, 0, 5)}[fam]
    ofam = {'wave': 'patch', 'patch': 'wave'}.get(fam, fam)
    cases.append(('%s_interleaved' % fam, [J(*((ofam, other) if i % 5 == 2 else (fam, q)), 1 + i, length=4) for i in range(LIMIT[fam] + 12)], 0))
  cases.append(('gather_shapes_4_0_2_0', [J('gather', ('gather', s), 10 + i) for i, s in enumerate((4, 0, 2, 0))], 0))
  cases.append(('gather_every_shape_twice', [J('gather', ('gather', s), 1 + i) for i, s in enumerate((3, 1, 4, 0, 2, 2, 0, 4, 1, 3))], 0))
  # equal lengths keep their queue order, within an instance and between instances; a longer job queued later goes first
  cases.append(('patch_equal_lengths', [J('patch', ('patch', 1, 3, 1, 64 if i % 3 else 32, 0), 1 + i, length=16) for i in range(9)] +
                [J('wave', W, 5, length=16), J('patch', P, 6, length=64), J('wave', W, 7, length=16)], 0))
  cases.append(('patch_lengths_mixed', [J('wave', W, 1 + i, length=(4, 96, 4, 32, 96, 4)[i % 6]) for i in range(60)], 0))
  # every key field separates instances
  keys = [(1, 3, 1, 64, 0), (3, 3, 1, 64, 0), (1, 4, 1, 64, 0), (1, 3, 2, 64, 0), (1, 3, 1, 32, 0), (1, 3, 1, 64, 1)]
  cases.append(('patch_key_fields', [J('patch', ('patch',) + k, 2 + i, length=4) for i, k in enumerate(keys + keys)] + [J('wave', W, 9, length=4)] * 2, 0))
  hkeys = [('bf16', 3, 0, 5), ('fp16', 3, 0, 5), ('bf16', 4, 0, 5), ('bf16', 3, 1, 0), ('bf16', 3, 0, 0)]
  cases.append(('h16_key_fields', [J('h16', ('h16',) + k, 2 + i) for i, k in enumerate(hkeys + hkeys)], 0))
  cases.append(('all_families', [J('h16', H, 1), J('gather', G, 2), J('wave', W, 3, length=8), J('gather', ('gather', 0), 4), J('patch', P, 5, length=8)], 0))
  cases.append(('discarded', [J('wave', W, 1, length=8), J('gather', G, 2), J('h16', H, 3), J('gather', G, 4), J('h16', H, 5), J('patch', P, 6, length=4)], 3))
  return cases


def test_pack_jobs_packs_what_the_mirror_packs(program):
  cases = [(e['id'], _queued_only([T.plan(b) for b in e['blocks']]), 0) for e in T.TABLE] + _synthetic()
  got = _run(program, cases)
  for name, plans, discard_before in cases:
    assert got[name] == _mirror(plans, discard_before), name
  # the cases are what they say
  assert got['empty'] == [] and [len(l[2]) for l in got['one_job']] == [1]
  for fam in LIMIT:
    assert [len(l[2]) for l in got['%s_%d_jobs' % (fam, LIMIT[fam])]] == [LIMIT[fam]]
    assert [len(l[2]) for l in got['%s_%d_jobs' % (fam, LIMIT[fam] + 1)]] == [LIMIT[fam], 1]
  assert [(l[1][0], l[2]) for l in got['gather_shapes_4_0_2_0']] == [(0, [1, 3]), (2, [2]), (4, [0])]
  assert got['patch_equal_lengths'][0][2] == [10, 1, 2, 4, 5, 7, 8] and got['patch_equal_lengths'][1][2] == [0, 3, 6]
  assert len({l[1] for l in got['patch_key_fields']}) == 7 and len({l[1] for l in got['h16_key_fields']}) == 5
  assert sorted(i for l in got['discarded'] for i in l[2]) == [3, 4, 5]
  assert sum(len(l) for l in got.values()) > 60


def test_workgroup_rollover_is_arithmetic_on_the_inputs(program):
  """Three jobs of 0x20000000 workgroups: any two pass 0x3fffffff, so every family launches them one by one; a total of exactly
  0x3fffffff still shares a launch, one more does not."""
  assert re.search(r'constexpr long MAX_LAUNCH_WGS = 0x3fffffff;', open(os.path.join(CSRC, 'job_queue.h')).read()) and T.MAX_LAUNCH_WGS == 0x3fffffff
  one = {'wave': ('wave',), 'patch': ('patch', 1, 3, 1, 64, 0), 'gather': ('gather', 1), 'h16': ('h16', 'bf16', 3, 0, 5)}
  cases = []
  for fam, q in one.items():
    cases.append(('%s_3x' % fam, [J(fam, q, 0x20000000, length=4)] * 3, 0))
    cases.append(('%s_exact' % fam, [J(fam, q, 0x20000000, length=4), J(fam, q, 0x1fffffff, length=4), J(fam, q, 1, length=4)], 0))
    cases.append(('%s_small_between' % fam, [J(fam, q, w, length=4) for w in (0x3ffffff0, 0xf, 1, 0x3ffffffe, 1, 1)], 0))
  got = _run(program, cases)
  for name, plans, _ in cases:
    assert all(l[3] <= 0x3fffffff for l in got[name]), name
    assert got[name] == _mirror(plans), name
  for fam in one:
    assert [(l[2], l[3]) for l in got['%s_3x' % fam]] == [([0], 0x20000000), ([1], 0x20000000), ([2], 0x20000000)]
    assert [(l[2], l[3]) for l in got['%s_exact' % fam]] == [([0, 1], 0x3fffffff), ([2], 1)]
    assert [(l[2], l[3]) for l in got['%s_small_between' % fam]] == [([0, 1], 0x3fffffff), ([2, 3], 0x3fffffff), ([4, 5], 2)]
