"""GPU: what dropout p > 0 costs a captured step, and that p = 0 costs nothing, on the headline shape (B=32, T=64, M=S=8) ->
profiles/dropout.json.  One precision per run (--precision fp32 | bf16), stored under precisions/<name>; every other
key of the file is kept.
Configurations, alternating fresh processes, median and range over the rounds:
  * parent    a built checkout of the commit in front of the feature, its default trainer (optional: --parent);
  * p0        THIS build, p = 0 everywhere: the launches of the parent;
  * nochain   THIS build, p = 0, MS_DECODER_CHAIN=0: the decoder's blocks one by one -- what the decoder leaving its chain costs alone;
  * p01       THIS build, p = 0.1 in every block that takes p (G and D);
  * parent_p01  this tree's Python on the PARENT's library (MS_LIB_PATH = <--parent>/mix_stage_amd/libmixstage_hip.so), p = 0.1 in G and
              D (optional: --parent; for a parent that has the dropout kernels): `p01` across two builds of the library in one call.
Bar, for `p0`: this build's median is within the parent's own min-max range around the parent's median, and the labelled
launches of a step are the parent's.  For `p0` against `parent` and `p01` against `parent_p01` the verdict also says whether the
median is at most the other build's median plus twice its own min-max range (`within_2x`: the bar of a change that must not cost
anything).  The price of p = 0.1 itself is reported, not gated: the price of an opt-in.  For the p = 0.1 steps the labelled
launches of eager steps are split: the ` dropout` passes (their count and the time between their events), the cb8 converters
(the 16-bit modes' round trip: count and time, against p0's) and everything else.
bench.py is not involved: it has no such option and measures the default trainer.

  python tools/dropout_report.py [--parent /path/to/built/parent/checkout] [--out profiles/dropout.json] [--rounds 3] [--precision bf16]

Every child process runs under its own time limit; the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M, S, T, P = 32, 8, 8, 64, 104
CONFIGS = {'p0': 0.0, 'nochain': 0.0, 'p01': 0.1, 'parent_p01': 0.1}


def build_model(dev, precision, p):
  """bench.build_model with p handed to G and D."""
  import mix_stage_amd as A
  from oracle import mixstage_oracle as O
  G = A.JointLateClusterSoftStyle4_G(time_steps=T, out_feats=P, num_clusters=M, style_dict={i: i for i in range(S)},
                                     style_dim=10, lambda_id=0.1, argmax=1, some_grad_flag=1, train_only=1, shape={}, p=p)
  D = A.Speech2Gesture_D(in_channels=P, p=p)
  model = A.GAN(G, D, criterion='L1Loss', input_modalities=['audio/log_mel_400'], update_D_prob_flag=0, no_grad=0)
  model.load_state_dict(O.deterministic_state(model.state_dict()))
  model.G.thresh.value, model.G.thresh.iters = 1, 10 ** 9
  model = model.to(dev)
  if precision == 'bf16':
    A.set_compute_dtype(model, 'bf16')
  return model


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
  model = bench.build_model(dev, precision) if config == 'parent' else build_model(dev, precision, CONFIGS[config])
  ts = MixStageTrainStep(model, use_graphs=True)
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
    for name, pick in (('dropout', lambda l: l.endswith(' dropout')), ('cb8', lambda l: '|cb8_from_plain' in l or '|cb8_to_plain' in l)):
      out['%s_%s_launches' % (kind, name)] = sum(r['count'] for r in rows if pick(r['label'])) // 4
      out['%s_%s_event_ms' % (kind, name)] = sum(r['total_ms'] for r in rows if pick(r['label'])) / 4
    out[kind + '_all_event_ms'] = sum(r['total_ms'] for r in rows) / 4
    # the dropout passes one by one, the largest first: [launches per step, ms per step]
    by = sorted(((r['label'].split('|')[-1], r['count'] // 4, round(r['total_ms'] / 4, 4)) for r in rows if r['label'].endswith(' dropout')),
                key=lambda x: -x[2])
    out[kind + '_dropout_by_label'] = {l: [c, ms] for l, c, ms in by}
  if getattr(ts, '_dropout_state', None) is not None:
    out['dropout_state'] = ts.dropout_state()
  print('RESULT ' + json.dumps(out))


def run_child(args, limit, env=None):
  o = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit,
                     env=dict(os.environ, **(env or {})))
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
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dropout.json'))
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--precision', default='fp32')
  ap.add_argument('--configs', default='parent,p0,nochain,p01,parent_p01', help='the configurations of a round, in the order they run')
  ap.add_argument('--child', nargs='+', default=None)
  a = ap.parse_args()
  if a.child:
    return child_timing(a.child[0], a.child[1], a.child[2])
  if a.parent and not os.path.isdir(os.path.join(a.parent, 'mix_stage_amd')):
    raise SystemExit('--parent: a built checkout of the parent commit')
  builds = {}
  for name in a.configs.split(','):
    if name == 'parent':
      if a.parent:
        builds['parent'] = os.path.abspath(a.parent)
    elif name == 'parent_p01':
      if a.parent:
        builds[name] = ROOT
    elif name in CONFIGS:
      builds[name] = ROOT
    else:
      raise SystemExit('--configs: %r is not one of parent, %s' % (name, ', '.join(CONFIGS)))
  precision = a.precision
  out = json.load(open(a.out)) if os.path.exists(a.out) else {}
  out.update(shape=dict(B=B, T=T, M=M, S=S),
             what=dict(timing='captured step, ms per step over 60 replays behind 20, one fresh process per run, the configurations alternating',
                       parent='the commit in front of the feature, default trainer', p0='this build, p = 0',
                       nochain='this build, p = 0, MS_DECODER_CHAIN=0 (the decoder block by block)', p01='this build, p = 0.1 in G and D', parent_p01="this tree's Python on the parent's library, p = 0.1 in G and D",
                       events='*_event_ms: the time between the HIP events around the labelled launches of EAGER steps, summed per step',
                       bar='p0 against parent: |median - parent median| <= parent max - parent min (within); p01 against parent_p01: median <= parent_p01 '
                           'median + 2 * (its max - its min) (within_2x, also reported for p0); equal labelled launches in both pairs; '
                           'nochain and the price of p01 over p0 are reported only'))
  runs = {name: [] for name in builds}
  for r in range(a.rounds):
    for name, root in builds.items():
      env = {'MS_DECODER_CHAIN': '0'} if name == 'nochain' else None
      if name == 'parent_p01':
        env = {'MS_LIB_PATH': os.path.join(os.path.abspath(a.parent), 'mix_stage_amd', 'libmixstage_hip.so')}
      x = run_child(['--child', root, precision, name], 300, env)
      runs[name].append(x)
      print('%s round %d %-8s G %.4f ms  D %.4f ms  launches G %d (%d dropout) D %d (%d dropout)'
            % (precision, r, name, x['G_ms'], x['D_ms'], x['G_launches'], x['G_dropout_launches'], x['D_launches'], x['D_dropout_launches']), flush=True)
  timing = {}
  for name, rr in runs.items():
    t = timing[name] = {}
    for k in 'GD':
      t[k + '_ms'] = med_range([x[k + '_ms'] for x in rr])
      t[k + '_launches'] = sorted({x[k + '_launches'] for x in rr})
      for part in ('dropout', 'cb8'):
        t['%s_%s_launches' % (k, part)] = sorted({x['%s_%s_launches' % (k, part)] for x in rr})
        t['%s_%s_event_ms' % (k, part)] = round(statistics.median([x['%s_%s_event_ms' % (k, part)] for x in rr]), 4)
      t[k + '_all_event_ms'] = round(statistics.median([x[k + '_all_event_ms'] for x in rr]), 4)
  mine = out.setdefault('precisions', {})[precision] = dict(rounds=a.rounds, order=list(builds), timing=timing)
  # the price of the opt-in, split: the decoder leaving its chain (nochain - p0), everything else that p = 0.1 adds (p01 - nochain: the
  # dropout passes in place of the in-conv BatchNorm, the bare convs, the fused forms that step aside, the converter round trip)
  price = {}
  for k in ('GD' if all(n in runs for n in ('p0', 'nochain', 'p01')) else ''):
    p0, nc, p01 = (timing[n][k + '_ms']['median'] for n in ('p0', 'nochain', 'p01'))
    price[k] = dict(p0_ms=p0, p01_ms=p01, total_ms=round(p01 - p0, 4), decoder_leaves_chain_ms=round(nc - p0, 4), rest_ms=round(p01 - nc, 4),
                    launches_p0=timing['p0'][k + '_launches'], launches_p01=timing['p01'][k + '_launches'],
                    dropout_launches=timing['p01'][k + '_dropout_launches'], dropout_event_ms=timing['p01'][k + '_dropout_event_ms'],
                    cb8_launches_p0=timing['p0'][k + '_cb8_launches'], cb8_launches_p01=timing['p01'][k + '_cb8_launches'],
                    cb8_event_ms_p0=timing['p0'][k + '_cb8_event_ms'], cb8_event_ms_p01=timing['p01'][k + '_cb8_event_ms'],
                    dropout_by_label=runs['p01'][-1][k + '_dropout_by_label'])
  if price:
    mine['price_of_p01'] = price
    print(json.dumps(price))
  pairs = [(new, old) for new, old in (('p0', 'parent'), ('p01', 'parent_p01')) if new in runs and old in runs]
  if pairs:
    verdict, ok, ok_2x = {}, True, True
    for new, old in pairs:
      for k in 'GD':
        p, n = timing[old][k + '_ms'], timing[new][k + '_ms']
        spread = p['max'] - p['min']
        same = all(x[k + '_labels'] == runs[old][0][k + '_labels'] for x in runs[new] + runs[old])
        v = verdict['%s_%s' % (new, k)] = dict(parent_median_ms=p['median'], median_ms=n['median'], parent_spread_ms=round(spread, 4),
                                               gap_ms=round(n['median'] - p['median'], 4), within=bool(abs(n['median'] - p['median']) <= spread),
                                               within_2x=bool(n['median'] <= p['median'] + 2 * spread), same_labelled_launches=bool(same))
        ok = ok and same and (v['within'] if new == 'p0' else v['within_2x'])
        ok_2x = ok_2x and same and v['within_2x']
    mine['verdict'], mine['within_bar'], mine['within_2x_bar'] = verdict, bool(ok), bool(ok_2x)
    print(json.dumps(verdict))
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  json.dump(out, open(a.out, 'w'), indent=1)
  print('wrote', a.out)


if __name__ == '__main__':
  main()
