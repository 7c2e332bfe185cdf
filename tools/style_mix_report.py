"""GPU: what the style-mixing route (ms_concat_style_soft_fwd/bwd in place of torch's matmul + transpose + cat for float style
weights) costs and buys -> profiles/style_mix.json:
  (a) id_path    the path it does not touch: the captured fp32 and bf16 G-step / D-step of the headline shape (B=32, T=64, M=S=8,
                 integer style ids) on a built checkout of the PARENT commit and on THIS build, alternating fresh processes; the bar
                 is DESIGN 4i / 4j's: this build's median is at most the parent's median plus twice the parent's own min-max range;
  (b) g_soft     the captured argmax=0 G-step (softmax of the style encoder's scores as per-clip weights) on this build: the new
                 route against MS_STYLE_SOFT=0, with the labelled launches of one eager step beside it;
  (c) sampler    a replayed StyleTransferSampler.sample_mixed forward at n = 8 windows, S = 8, against the id-form replay of
                 sample_interval and against MS_STYLE_SOFT=0.
(b) and (c) are recorded without a target.  Times are ms per replay over 60 replays behind 20, one fresh process per run, median and
range over the rounds.

  python tools/style_mix_report.py --parent /path/to/built/parent/checkout [--out profiles/style_mix.json] [--rounds 3]

Every child process runs under its own time limit; the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M, S, N_WIN = 32, 8, 8, 8
WARM, REPS = 20, 60


def _tree(root):
  sys.path.insert(0, root)                    # the tree under test: its mix_stage_amd, its bench.py, its oracle
  import mix_stage_amd
  assert os.path.abspath(os.path.dirname(os.path.dirname(mix_stage_amd.__file__))) == os.path.abspath(root), mix_stage_amd.__file__


def _timed(fn):
  import torch
  for _ in range(WARM):
    fn()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(REPS):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / REPS * 1e3


def _labels(fn):
  import torch
  from mix_stage_amd import ops
  ops.timing_enable(True)
  try:
    fn()
    torch.cuda.synchronize()
    rows = ops.timing_report()
  finally:
    ops.timing_enable(False)
  return {r['label']: r['count'] for r in rows}


def child_steps(root, argmax):
  """Captured G / D steps of the headline shape, fp32 and bf16 (argmax=1: the id path; argmax=0: G only, the soft route)."""
  _tree(root)
  import torch
  import bench
  from mix_stage_amd.train_step import MixStageTrainStep
  from oracle import mixstage_oracle as O
  dev = torch.device('cuda:0')
  audio, pose, labels, style = O.synthetic_batch(B, M=M, S=S)
  batch = [t.to(dev) for t in (audio, labels, pose, style)]
  out = {}
  for precision in ('fp32', 'bf16'):
    model = bench.build_model(dev, precision)
    model.G.argmax = argmax
    ts = MixStageTrainStep(model, use_graphs=True)
    for kind in ('GD' if argmax else 'G'):
      out['%s_%s_ms' % (precision, kind)] = _timed(lambda: ts.step(*batch, kind=kind))
    ts.check_health()
    if not argmax:
      ts.use_graphs = False
      lab = _labels(lambda: ts.step(*batch, kind='G'))
      out['%s_G_launches' % precision] = sum(lab.values())
      out['%s_G_concat_labels' % precision] = {k: v for k, v in lab.items() if 'concat_style' in k}
  print('RESULT ' + json.dumps(out))


def child_sampler(root):
  """Replays of the sampler's captured eval forward on one interval of n = 8 windows: float weights (sample_mixed) and ids."""
  _tree(root)
  import torch
  import bench
  from mix_stage_amd import ops
  from mix_stage_amd.sample import StyleTransferSampler
  from oracle import mixstage_oracle as O
  dev = torch.device('cuda:0')
  audio, pose, labels, style = [t.to(dev) for t in O.synthetic_batch(N_WIN, M=M, S=S)]
  model = bench.build_model(dev, 'fp32')
  sampler = StyleTransferSampler(model, num_styles=S, use_graphs=True)
  mixes = [('half', {0: 0.5, 3: 0.5}), ('ramp', ('ramp', {0: 1.0}, {5: 1.0}))]
  sampler.sample_mixed(audio, labels, pose, mixes)
  sampler.sample_interval(audio, labels, pose, torch.full_like(style, 2), all_styles=False)
  graphs = {('mix' if k[0] == 'mix' else 'ids'): e['graph'] for k, e in sampler._graphs.items()}
  assert sorted(graphs) == ['ids', 'mix'], sorted(graphs)
  out = {name + '_replay_ms': _timed(g.replay) for name, g in sorted(graphs.items())}
  eager = StyleTransferSampler(model, num_styles=S, use_graphs=False)
  lab = _labels(lambda: eager.sample_mixed(audio, labels, pose, mixes[:1]))
  out['mix_launches'] = sum(lab.values())
  out['mix_concat_labels'] = {k: v for k, v in lab.items() if 'concat_style' in k}
  out['style_soft'] = bool(ops.style_soft_active())
  print('RESULT ' + json.dumps(out))


def run_child(args, limit, env=None):
  e = dict(os.environ)
  e.pop('MS_STYLE_SOFT', None)
  e.update(env or {})
  o = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit, env=e)
  line = [l for l in o.stdout.splitlines() if l.startswith('RESULT ')]
  if o.returncode != 0 or not line:
    sys.stderr.write(o.stdout[-2000:] + o.stderr[-4000:])
    raise SystemExit('child %s failed with exit status %s: nothing more is started' % (args, o.returncode))
  return json.loads(line[0][7:])


def med_range(v):
  return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v])


def alternate(variants, rounds, label):
  """variants: name -> (child args, env).  -> name -> list of child results, the variants alternating."""
  runs = {name: [] for name in variants}
  for r in range(rounds):
    for name, (args, env) in variants.items():
      runs[name].append(run_child(args, 300, env))
      print('%s round %d %-10s %s' % (label, r, name, json.dumps({k: round(v, 4) for k, v in runs[name][-1].items() if k.endswith('_ms')})),
            flush=True)
  return runs


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--parent', default=None, help='a BUILT checkout of the commit to compare with')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'style_mix.json'))
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--child', nargs='+', default=None)
  a = ap.parse_args()
  if a.child:
    return child_sampler(a.child[1]) if a.child[0] == 'sampler' else child_steps(a.child[1], int(a.child[2]))
  if not a.parent or not os.path.isdir(os.path.join(a.parent, 'mix_stage_amd')):
    raise SystemExit('--parent: a built checkout of the parent commit is needed for the comparison')
  out = dict(shape=dict(B=B, T=64, M=M, S=S, sampler_windows=N_WIN), rounds=a.rounds,
             what=dict(timing='ms per replay over %d replays behind %d, one fresh process per run, the variants alternating' % (REPS, WARM),
                       id_path='captured G / D step with integer style ids (the default trainer): parent commit against this build',
                       g_soft='captured argmax=0 G-step on this build: ms_concat_style_soft_fwd/bwd against MS_STYLE_SOFT=0 (matmul + cat)',
                       sampler='replay of the captured long-sequence eval forward: float weights (sample_mixed), MS_STYLE_SOFT=0, integer ids',
                       bar='id_path only: this build median <= parent median + 2 x (parent max - parent min)'))

  def save():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, 'w'), indent=1)

  # (a) the id path, parent against this build
  runs = alternate({'parent': (['--child', 'steps', os.path.abspath(a.parent), '1'], None), 'this': (['--child', 'steps', ROOT, '1'], None)},
                   a.rounds, 'id_path')
  ok, verdict = True, {}
  for key in ('fp32_G_ms', 'fp32_D_ms', 'bf16_G_ms', 'bf16_D_ms'):
    p, n = med_range([x[key] for x in runs['parent']]), med_range([x[key] for x in runs['this']])
    bar = 2 * (p['max'] - p['min'])
    verdict[key] = dict(parent=p, this=n, allowed_gap_ms=round(bar, 4), gap_ms=round(n['median'] - p['median'], 4),
                        within=bool(n['median'] - p['median'] <= bar))
    ok = ok and verdict[key]['within']
  out['id_path'] = dict(verdict=verdict, within_bar=bool(ok))
  print('id_path', json.dumps({k: (v['gap_ms'], v['allowed_gap_ms'], v['within']) for k, v in verdict.items()}), flush=True)
  save()
  # (b) the argmax=0 G-step, new route against the old one
  runs = alternate({'soft': (['--child', 'steps', ROOT, '0'], None), 'matmul_cat': (['--child', 'steps', ROOT, '0'], {'MS_STYLE_SOFT': '0'})},
                   a.rounds, 'g_soft')
  out['g_soft'] = {name: dict(fp32_G_ms=med_range([x['fp32_G_ms'] for x in rr]), bf16_G_ms=med_range([x['bf16_G_ms'] for x in rr]),
                              fp32_G_launches=rr[0]['fp32_G_launches'], bf16_G_launches=rr[0]['bf16_G_launches'],
                              concat_labels=rr[0]['fp32_G_concat_labels']) for name, rr in runs.items()}
  save()
  # (c) the sampler
  runs = alternate({'soft': (['--child', 'sampler', ROOT], None), 'matmul_cat': (['--child', 'sampler', ROOT], {'MS_STYLE_SOFT': '0'})},
                   a.rounds, 'sampler')
  out['sampler'] = {name: dict(mix_replay_ms=med_range([x['mix_replay_ms'] for x in rr]), ids_replay_ms=med_range([x['ids_replay_ms'] for x in rr]),
                               mix_launches=rr[0]['mix_launches'], concat_labels=rr[0]['mix_concat_labels'], style_soft=rr[0]['style_soft'])
                    for name, rr in runs.items()}
  save()
  print('wrote', a.out, 'id path within the bar:', ok)


if __name__ == '__main__':
  main()
