"""GPU: what the moving average of the generator's weights costs a captured step, on the headline shape (B=32, T=64, M=S=8), fp32
and bf16 -> profiles/ema.json.  Three configurations, alternating fresh processes, median and range over the rounds:
  * parent   a built checkout of the commit in front of the feature, its default trainer;
  * off      THIS build, ema_decay=None: the entry points and launches of the parent;
  * ema      THIS build, ema_decay=0.999: the G-step's Adam launch is ms_adam_step_segmented_ema, the D-step's is unchanged.
Bars:
  * `off` (G and D) and the D-step of `ema`: the bar of DESIGN 4i -- this build's median is at most the parent's median plus twice
    the parent's own min-max range;
  * the G-step of `ema`: the time it adds is measured against the parent's own `ew|ew_adam_step_segmented` time (the library's
    HIP-event scope around the prep launch and the element pass, mean over eager steps at the same shape).  The element pass goes
    from 7 to 9 16-byte streams: the expectation is 2/7 of that time, the allowance 1.5 x the expectation.
bench.py is not involved: it has no such option and measures the default trainer.

  python tools/ema_report.py --parent /path/to/built/parent/checkout [--out profiles/ema.json] [--rounds 3]

Every child process runs under its own time limit; the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M, S = 32, 8, 8
DECAY = 0.999
ADAM = 'ew|ew_adam_step_segmented'


def child_timing(root, precision, ema):
  sys.path.insert(0, root)                    # the tree under test: its mix_stage_amd, its bench.py, its oracle
  import torch
  import bench
  import mix_stage_amd
  from mix_stage_amd import ops
  from mix_stage_amd.train_step import MixStageTrainStep
  from oracle import mixstage_oracle as O
  assert os.path.abspath(os.path.dirname(os.path.dirname(mix_stage_amd.__file__))) == os.path.abspath(root), mix_stage_amd.__file__
  dev = torch.device('cuda:0')
  audio, pose, labels, style = O.synthetic_batch(B, M=M, S=S)
  batch = [t.to(dev) for t in (audio, labels, pose, style)]
  model = bench.build_model(dev, precision)
  ts = MixStageTrainStep(model, use_graphs=True, **({'ema_decay': DECAY} if ema else {}))
  out = {}
  for kind in 'GD':
    for _ in range(20):                       # capture and warm-up
      ts.step(*batch, kind=kind)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(60):
      ts.step(*batch, kind=kind)
    torch.cuda.synchronize()
    out[kind + '_ms'] = (time.perf_counter() - t0) / 60 * 1e3
  ts.check_health()
  for kind in 'GD':                           # labelled launches of eager steps: the same code path the capture recorded
    ts.use_graphs = False
    try:
      ts.step(*batch, kind=kind)              # (the first eager step creates what only the eager path needs: not timed)
      torch.cuda.synchronize()
      ops.timing_enable(True)
      for _ in range(8):
        ts.step(*batch, kind=kind)
      torch.cuda.synchronize()
      rows = ops.timing_report()
    finally:
      ops.timing_enable(False)
      ts.use_graphs = True
    out[kind + '_launches'] = sum(r['count'] for r in rows) // 8
    out[kind + '_labels'] = {r['label']: r['count'] // 8 for r in rows}
    adam = [r for r in rows if r['label'] == ADAM]
    out[kind + '_adam_ms'] = adam[0]['total_ms'] / adam[0]['count'] if adam else None
  out['n_G'] = int(ts.optim_G.total)
  print('RESULT ' + json.dumps(out))


def run_child(args, limit):
  o = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
  line = [l for l in o.stdout.splitlines() if l.startswith('RESULT ')]
  if o.returncode != 0 or not line:
    sys.stderr.write(o.stdout[-2000:] + o.stderr[-4000:])
    raise SystemExit('child %s failed with exit status %s: nothing more is started' % (args, o.returncode))
  return json.loads(line[0][7:])


def med_range(v):
  return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parent', default=None, help='a BUILT checkout of the commit to compare with')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ema.json'))
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--child', nargs='+', default=None)
  a = ap.parse_args()
  if a.child:
    return child_timing(a.child[0], a.child[1], a.child[2] == '1')
  if not a.parent or not os.path.isdir(os.path.join(a.parent, 'mix_stage_amd')):
    raise SystemExit('--parent: a built checkout of the parent commit is needed for the comparison')
  builds = {'parent': (os.path.abspath(a.parent), '0'), 'off': (ROOT, '0'), 'ema': (ROOT, '1')}
  out = dict(shape=dict(B=B, T=64, M=M, S=S), rounds=a.rounds, ema_decay=DECAY,
             what=dict(timing='captured step, ms per step over 60 replays behind 20, one fresh process per run, the three configurations alternating',
                       parent='the commit in front of the feature, default trainer',
                       off='this build, ema_decay=None', ema='this build, MixStageTrainStep(ema_decay=0.999)',
                       adam='mean time of the %s scope (prep launch + element pass) over 8 eager steps of the kind, HIP events' % ADAM,
                       bar='off G, off D, ema D: median <= parent median + 2 x (parent max - parent min), equal labelled launches; '
                           'ema G: added time <= 1.5 x (2/7 x the parent\'s adam scope time of its G-step)'),
             precisions={})
  ok = True
  for precision in ('fp32', 'bf16'):
    runs = {name: [] for name in builds}
    for r in range(a.rounds):
      for name, (root, flag) in builds.items():
        x = run_child(['--child', root, precision, flag], 300)
        runs[name].append(x)
        print('%s round %d %-6s G %.4f ms  D %.4f ms  adam G %.4f D %.4f ms  launches G %d D %d'
              % (precision, r, name, x['G_ms'], x['D_ms'], x['G_adam_ms'], x['D_adam_ms'], x['G_launches'], x['D_launches']), flush=True)
    timing, verdict = {}, {}
    for name, rr in runs.items():
      timing[name] = dict(G_ms=med_range([x['G_ms'] for x in rr]), D_ms=med_range([x['D_ms'] for x in rr]),
                          G_adam_ms=med_range([x['G_adam_ms'] for x in rr]), D_adam_ms=med_range([x['D_adam_ms'] for x in rr]),
                          G_launches=sorted({x['G_launches'] for x in rr}), D_launches=sorted({x['D_launches'] for x in rr}))
    for name, k in (('off', 'G'), ('off', 'D'), ('ema', 'D')):
      p, n = timing['parent'][k + '_ms'], timing[name][k + '_ms']
      bar = 2 * (p['max'] - p['min'])
      same = all(x[k + '_labels'] == runs['parent'][0][k + '_labels'] for x in runs[name] + runs['parent'])
      verdict[name + '_' + k] = dict(parent_median_ms=p['median'], median_ms=n['median'], parent_range_ms=round(p['max'] - p['min'], 4),
                                     range_ms=round(n['max'] - n['min'], 4), allowed_gap_ms=round(bar, 4),
                                     gap_ms=round(n['median'] - p['median'], 4), within=bool(n['median'] - p['median'] <= bar),
                                     same_labelled_launches=bool(same))
      ok = ok and verdict[name + '_' + k]['within'] and same
    p, n = timing['parent']['G_ms'], timing['ema']['G_ms']
    adam = timing['parent']['G_adam_ms']['median']
    added = n['median'] - p['median']
    same = all(x['G_labels'] == runs['parent'][0]['G_labels'] for x in runs['ema'])
    verdict['ema_G'] = dict(parent_median_ms=p['median'], median_ms=n['median'], parent_adam_ms=adam, added_ms=round(added, 4),
                            ratio_added_to_parent_adam=round(added / adam, 4), expected_ratio=round(2 / 7, 4),
                            allowed_added_ms=round(1.5 * 2 / 7 * adam, 4), within=bool(added <= 1.5 * 2 / 7 * adam),
                            ema_adam_ms=timing['ema']['G_adam_ms']['median'],
                            scope_added_ms=round(timing['ema']['G_adam_ms']['median'] - adam, 4),
                            parent_range_ms=round(p['max'] - p['min'], 4), range_ms=round(n['max'] - n['min'], 4),
                            same_labelled_launches=bool(same), elements=runs['ema'][0]['n_G'])
    ok = ok and verdict['ema_G']['within'] and same
    out['precisions'][precision] = dict(timing=timing, verdict=verdict)
    print(precision, json.dumps(verdict), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)     # after every precision: a later child that fails does not cost this one
    json.dump(out, open(a.out, 'w'), indent=1)
  out['within_bar'] = bool(ok)
  json.dump(out, open(a.out, 'w'), indent=1)
  print('wrote', a.out, 'within the bar:', ok)


if __name__ == '__main__':
  main()
