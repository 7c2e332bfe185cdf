"""GPU: what keeping the learning rate in a device word costs a captured step, on the headline shape (B=32, T=64, M=S=8), fp32 and
bf16 -> profiles/lr_schedule.json:
  * timing    the captured G-step / D-step time of the PARENT build (a built checkout of the commit in front of the feature, lr a
              by-value kernel argument) and of THIS build with lr_schedule=0.99 (ms_adam_step_segmented_lr reads the word):
              alternating fresh processes, median and range over the rounds;
  * launches  the labelled launches of one eager step of each kind (the library's HIP-event scopes), label by label;
  * bar       the one DESIGN 4i used: this build's median is at most the parent's median plus twice the parent's own min-max range.
bench.py is not involved: it has no learning-rate option and measures the default trainer.

  python tools/lr_schedule_report.py --parent /path/to/built/parent/checkout [--out profiles/lr_schedule.json] [--rounds 3]

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
GAMMA = 0.99


def child_timing(root, precision, scheduled):
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
  ts = MixStageTrainStep(model, use_graphs=True, **({'lr_schedule': GAMMA} if scheduled else {}))
  out = {}
  for kind in 'GD':
    for _ in range(20):                       # capture and warm-up
      ts.step(*batch, kind=kind)
    if scheduled:
      ts.epoch_end()                          # (the write between two steps is part of the feature; once per epoch in real use)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(60):
      ts.step(*batch, kind=kind)
    torch.cuda.synchronize()
    out[kind + '_ms'] = (time.perf_counter() - t0) / 60 * 1e3
  ts.check_health()
  for kind in 'GD':                           # labelled launches of one step: the same code path the capture recorded
    ops.timing_enable(True)
    ts.use_graphs = False
    try:
      ts.step(*batch, kind=kind)
      torch.cuda.synchronize()
      rows = ops.timing_report()
    finally:
      ops.timing_enable(False)
      ts.use_graphs = True
    out[kind + '_launches'] = sum(r['count'] for r in rows)
    out[kind + '_labels'] = {r['label']: r['count'] for r in rows}
  if scheduled:
    out['lr'] = list(ts.lr())
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
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lr_schedule.json'))
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--child', nargs='+', default=None)
  a = ap.parse_args()
  if a.child:
    return child_timing(a.child[0], a.child[1], a.child[2] == '1')
  if not a.parent or not os.path.isdir(os.path.join(a.parent, 'mix_stage_amd')):
    raise SystemExit('--parent: a built checkout of the parent commit is needed for the comparison')
  builds = {'parent': (os.path.abspath(a.parent), '0'), 'lr_schedule': (ROOT, '1')}
  out = dict(shape=dict(B=B, T=64, M=M, S=S), rounds=a.rounds, gamma=GAMMA,
             what=dict(timing='captured step, ms per step over 60 replays behind 20, one fresh process per run, the two builds alternating',
                       parent='the commit in front of the feature: lr is a by-value argument of the prep kernel',
                       lr_schedule='this build, MixStageTrainStep(lr_schedule=0.99): the prep kernel reads lr from a device word; one '
                                   'epoch_end() (two 1-word writes) in front of the timed replays',
                       launches='labelled launches (HIP-event scopes of the library) of one eager step of the kind',
                       bar='lr_schedule median <= parent median + 2 x (parent max - parent min); equal labelled launches'),
             precisions={})
  ok = True
  for precision in ('fp32', 'bf16'):
    runs = {name: [] for name in builds}
    for r in range(a.rounds):
      for name, (root, flag) in builds.items():
        runs[name].append(run_child(['--child', root, precision, flag], 300))
        print('%s round %d %-11s G %.4f ms  D %.4f ms  launches G %d D %d' % (precision, r, name, runs[name][-1]['G_ms'], runs[name][-1]['D_ms'],
                                                                              runs[name][-1]['G_launches'], runs[name][-1]['D_launches']), flush=True)
    timing, verdict = {}, {}
    for name, rr in runs.items():
      timing[name] = dict(G_ms=med_range([x['G_ms'] for x in rr]), D_ms=med_range([x['D_ms'] for x in rr]),
                          G_launches=sorted({x['G_launches'] for x in rr}), D_launches=sorted({x['D_launches'] for x in rr}))
    for k in 'GD':
      p, n = timing['parent'][k + '_ms'], timing['lr_schedule'][k + '_ms']
      bar = 2 * (p['max'] - p['min'])
      same = all(x[k + '_labels'] == runs['parent'][0][k + '_labels'] for rr in runs.values() for x in rr)
      verdict[k] = dict(parent_median_ms=p['median'], lr_schedule_median_ms=n['median'], parent_range_ms=round(p['max'] - p['min'], 4),
                        lr_schedule_range_ms=round(n['max'] - n['min'], 4), allowed_gap_ms=round(bar, 4),
                        gap_ms=round(n['median'] - p['median'], 4), within=bool(n['median'] - p['median'] <= bar),
                        same_labelled_launches=bool(same),
                        adam_launches=runs['lr_schedule'][0][k + '_labels'].get('ew|ew_adam_step_segmented'))
      ok = ok and verdict[k]['within'] and same
    out['precisions'][precision] = dict(timing=timing, verdict=verdict, labels_G=runs['lr_schedule'][0]['G_labels'],
                                        labels_D=runs['lr_schedule'][0]['D_labels'])
    print(precision, json.dumps(verdict), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)     # after every precision: a later child that fails does not cost this one
    json.dump(out, open(a.out, 'w'), indent=1)
  out['within_bar'] = bool(ok)
  json.dump(out, open(a.out, 'w'), indent=1)
  print('wrote', a.out, 'within the bar:', ok)


if __name__ == '__main__':
  main()
