"""GPU: what frozen BatchNorm statistics do to a captured step, on the headline shape (B=32, T=64, M=S=8) ->
profiles/frozen_bn.json.  One precision per run (--precision fp32 | bf16), stored under precisions/<name>; every
other key of the file (the other precision, the tests' accuracy figures, wall times) is kept.
Configurations, alternating fresh processes, median and range over the rounds:
  * parent    a built checkout of the commit in front of the feature, its default trainer (optional: --parent);
  * off       THIS build, freeze_bn=None: the launches of the parent;
  * encoders  THIS build, MixStageTrainStep(freeze_bn=['G.audio_encoder', 'G.unet']);
  * all       THIS build, MixStageTrainStep(freeze_bn=True).
Bar, for `off` only: this build's median is within the parent's own min-max range around the parent's median, and the labelled
launches of a step are the parent's.  The frozen steps' own times are reported, not gated.
bench.py is not involved: it has no such option and measures the default trainer.

  python tools/frozen_bn_report.py [--parent /path/to/built/parent/checkout] [--out profiles/frozen_bn.json] [--rounds 3] [--precision bf16]

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
FREEZE = {'off': None, 'encoders': ['G.audio_encoder', 'G.unet'], 'all': True}


def child_timing(root, precision, config):
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
  kw = {} if config in ('parent', 'off') else {'freeze_bn': FREEZE[config]}
  ts = MixStageTrainStep(model, use_graphs=True, **kw)
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
      for _ in range(4):
        ts.step(*batch, kind=kind)
      torch.cuda.synchronize()
      rows = ops.timing_report()
    finally:
      ops.timing_enable(False)
      ts.use_graphs = True
    out[kind + '_launches'] = sum(r['count'] for r in rows) // 4
    out[kind + '_labels'] = {r['label']: r['count'] // 4 for r in rows}
    out[kind + '_frozen_launches'] = sum(r['count'] for r in rows if r['label'].endswith(' frozen')) // 4
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
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frozen_bn.json'))
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--precision', default='fp32')
  ap.add_argument('--child', nargs='+', default=None)
  a = ap.parse_args()
  if a.child:
    return child_timing(a.child[0], a.child[1], a.child[2])
  builds = {}
  if a.parent:
    if not os.path.isdir(os.path.join(a.parent, 'mix_stage_amd')):
      raise SystemExit('--parent: a built checkout of the parent commit')
    builds['parent'] = os.path.abspath(a.parent)
  builds.update({name: ROOT for name in FREEZE})
  precision = a.precision
  # (the file also carries what other runs and the tests' figures put there -- the other precision, `accuracy`, the wall times:
  # this run replaces its own keys only)
  out = json.load(open(a.out)) if os.path.exists(a.out) else {}
  out.update(shape=dict(B=B, T=64, M=M, S=S),
             what=dict(timing='captured step, ms per step over 60 replays behind 20, one fresh process per run, the configurations alternating',
                       parent='the commit in front of the feature, default trainer', off='this build, freeze_bn=None',
                       encoders="this build, freeze_bn=['G.audio_encoder', 'G.unet']", all='this build, freeze_bn=True',
                       bar='off: |median - parent median| <= parent max - parent min, equal labelled launches; the frozen steps are reported only'))
  runs = {name: [] for name in builds}
  for r in range(a.rounds):
    for name, root in builds.items():
      x = run_child(['--child', root, precision, name], 300)
      runs[name].append(x)
      print('%s round %d %-8s G %.4f ms  D %.4f ms  launches G %d (%d frozen) D %d (%d frozen)'
            % (precision, r, name, x['G_ms'], x['D_ms'], x['G_launches'], x['G_frozen_launches'], x['D_launches'], x['D_frozen_launches']), flush=True)
  timing = {}
  for name, rr in runs.items():
    timing[name] = dict(G_ms=med_range([x['G_ms'] for x in rr]), D_ms=med_range([x['D_ms'] for x in rr]),
                        G_launches=sorted({x['G_launches'] for x in rr}), D_launches=sorted({x['D_launches'] for x in rr}),
                        G_frozen_launches=sorted({x['G_frozen_launches'] for x in rr}), D_frozen_launches=sorted({x['D_frozen_launches'] for x in rr}))
  mine = out.setdefault('precisions', {})[precision] = dict(rounds=a.rounds, timing=timing)
  if 'parent' in runs:
    verdict, ok = {}, True
    for k in 'GD':
      p, n = timing['parent'][k + '_ms'], timing['off'][k + '_ms']
      spread = p['max'] - p['min']
      same = all(x[k + '_labels'] == runs['parent'][0][k + '_labels'] for x in runs['off'] + runs['parent'])
      verdict['off_' + k] = dict(parent_median_ms=p['median'], median_ms=n['median'], parent_spread_ms=round(spread, 4),
                                 gap_ms=round(n['median'] - p['median'], 4), within=bool(abs(n['median'] - p['median']) <= spread),
                                 same_labelled_launches=bool(same))
      ok = ok and verdict['off_' + k]['within'] and same
    mine['verdict'], mine['within_bar'] = verdict, bool(ok)
    print(json.dumps(verdict))
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  json.dump(out, open(a.out, 'w'), indent=1)
  print('wrote', a.out)


if __name__ == '__main__':
  main()
