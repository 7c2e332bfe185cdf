"""GPU: what fp16 training with dynamic loss scaling costs and buys at step level, on the headline shape (B=32, T=64, M=S=8)
-> profiles/fp16_train.json:
  * timing    the captured G-step / D-step time of bf16 and of fp16 + dynamic scaling: alternating fresh processes, median and range
              over the rounds, and the labelled launches of one step of each kind (the library's HIP-event scopes, as
              tools/label_table.py counts them; the aten launches around them come from the same Python in both modes);
  * accuracy  pose L1 and the relative L2 distance of each network's UNSCALED gradient from the fp32 HIP path on the same batch and
              weights, for bf16, fp16 + dynamic, fp16 static S = 1 and fp16 static S = 2^16 (a dynamic scale is measured at the
              scale it settles on: skipped steps leave the weights where they were and are repeated);
  * trajectory  both networks' scales over 200 captured steps of the reference coin flip.
bench.py is not involved and has no fp16 training choice.

  python tools/fp16_train_report.py [--out profiles/fp16_train.json] [--rounds 3] [--steps 200]

Every child process runs under its own time limit; the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, M, S = 32, 8, 8
CONFIGS = {'fp32': ('fp32', None), 'bf16': ('bf16', None), 'fp16_dynamic': ('fp16', 'dynamic'), 'fp16_static_1': ('fp16', 1.0),
           'fp16_static_65536': ('fp16', 65536.0)}


def _trainer(name, use_graphs):
  import torch
  import bench
  import mix_stage_amd as A
  from mix_stage_amd.train_step import MixStageTrainStep
  from oracle import mixstage_oracle as O
  dev = torch.device('cuda:0')
  dtype, ls = CONFIGS[name]
  audio, pose, labels, style = O.synthetic_batch(B, M=M, S=S)
  batch = [t.to(dev) for t in (audio, labels, pose, style)]
  model = bench.build_model(dev, 'bf16' if dtype == 'bf16' else 'fp32')
  if dtype == 'fp16':
    A.set_compute_dtype(model, 'fp16')
  kw = {'loss_scale': ls} if ls is not None else {}
  return MixStageTrainStep(model, use_graphs=use_graphs, **kw), model, batch


def child_timing(name):
  import torch
  from mix_stage_amd import ops
  ts, model, batch = _trainer(name, True)
  out = {}
  for kind in 'GD':
    for _ in range(20):                       # capture, and the dynamic scale settles (a halving per skipped step)
      ts.step(*batch, kind=kind)
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
    out[kind + '_labels'] = len(rows)
  if CONFIGS[name][1] is not None:
    out['loss_scale'] = ts.loss_scale()
  print('RESULT ' + json.dumps(out))


def child_accuracy():
  import torch
  from oracle import mixstage_oracle as O
  res, ref = {}, {}
  for name in CONFIGS:
    ts, model, batch = _trainer(name, False)
    ts.on_bad_step = 'skip'
    row = {}
    for kind in 'GD':
      opt = ts.optim_G if kind == 'G' else ts.optim_D
      model.load_state_dict(O.deterministic_state(model.state_dict()))
      ts.optim_G.reset_state(); ts.optim_D.reset_state()
      tries = 0
      while True:
        S_in = float(opt.seed()) if opt.ls_state is not None else 1.0
        ts.step(*batch, kind=kind)
        tries += 1
        applied = int(opt.step_state[2]) == 0
        if applied or opt.ls_state is None or int(opt.ls_state[4]) == 0 or tries > 30:
          break                               # (an overflow skip left the weights untouched: the same step again, at half the scale)
      live = opt.live_elems(opt.active_params())
      g = opt.flat_g[:live].double() / S_in
      fake = ts.fake_pose.detach().double()
      entry = dict(applied=bool(applied), steps_until_applied=tries, scale=S_in, grad_norm=float(opt.norm))
      if name == 'fp32':
        ref[kind] = (g.clone(), fake.clone())
      else:
        rg, rf = ref[kind]
        entry['pose_l1'] = float((fake - rf).abs().mean())
        entry['grad_rel_l2'] = float((g - rg).norm() / rg.norm()) if applied else None
        entry['grad_zero_fraction_vs_fp32'] = float(((g == 0) & (rg != 0)).double().mean())
      row[kind] = entry
    import warnings
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      ts.check_health()
    res[name] = row
    del ts, model
    torch.cuda.empty_cache()
  print('RESULT ' + json.dumps(res))


def child_trajectory(steps):
  import torch
  torch.manual_seed(0)
  ts, model, batch = _trainer('fp16_dynamic', True)
  log = torch.zeros(steps, 2, 8, dtype=torch.int32, device='cuda:0')
  kinds, first, last = '', None, None
  for i in range(steps):
    kinds += ts.step(*batch)
    log[i, 0].copy_(ts.optim_G.ls_state)
    log[i, 1].copy_(ts.optim_D.ls_state)
    if i in (0, steps - 1):
      vals = [float(l) for l in ts.losses]
      first, last = (vals, last) if i == 0 else (first, vals)
  ts.check_health()
  log = log.cpu()
  scales = log[:, :, 0].contiguous().view(torch.float32)
  changes = [dict(step=i, kind=kinds[i], S_G=float(scales[i, 0]), S_D=float(scales[i, 1]), overflow_skips_G=int(log[i, 0, 3]),
                  overflow_skips_D=int(log[i, 1, 3]))
             for i in range(steps) if i == 0 or i == steps - 1 or not torch.equal(scales[i], scales[i - 1])]
  print('RESULT ' + json.dumps(dict(steps=steps, kinds=kinds, scale_changes=changes, bad_steps=ts.skipped_steps,
                                    final=ts.loss_scale(), losses_first_step=first, losses_last_step=last)))


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
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fp16_train.json'))
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--child', nargs='+', default=None)
  a = ap.parse_args()
  if a.child:
    return {'timing': lambda: child_timing(a.child[1]), 'accuracy': child_accuracy,
            'trajectory': lambda: child_trajectory(int(a.child[1]))}[a.child[0]]()
  runs = {'bf16': [], 'fp16_dynamic': []}
  for r in range(a.rounds):
    for name in runs:
      runs[name].append(run_child(['--child', 'timing', name], 300))
      print('round %d %-13s %s' % (r, name, {k: v for k, v in runs[name][-1].items() if k != 'loss_scale'}), flush=True)
  timing = {}
  for name, rr in runs.items():
    timing[name] = dict(G_ms=med_range([x['G_ms'] for x in rr]), D_ms=med_range([x['D_ms'] for x in rr]),
                        G_launches=sorted({x['G_launches'] for x in rr}), D_launches=sorted({x['D_launches'] for x in rr}),
                        G_labels=sorted({x['G_labels'] for x in rr}), D_labels=sorted({x['D_labels'] for x in rr}))
    if 'loss_scale' in rr[-1]:
      timing[name]['loss_scale_after_timing'] = rr[-1]['loss_scale']
  verdict = {}
  for k in 'GD':
    b, f = timing['bf16'][k + '_ms'], timing['fp16_dynamic'][k + '_ms']
    bar = 2 * (b['max'] - b['min'])
    verdict[k] = dict(bf16_median_ms=b['median'], fp16_median_ms=f['median'], allowed_gap_ms=round(bar, 4),
                      gap_ms=round(f['median'] - b['median'], 4), within=bool(f['median'] - b['median'] <= bar),
                      equal_launch_count=timing['bf16'][k + '_launches'] == timing['fp16_dynamic'][k + '_launches'])
  out = dict(shape=dict(B=B, T=64, M=M, S=S), rounds=a.rounds,
             what=dict(timing='captured step, ms per step over 60 replays behind 20, one fresh process per run, bf16 and fp16 alternating',
                       launches='labelled launches (HIP-event scopes of the library) of one eager step of the kind',
                       bar='fp16 median within 2 x (bf16 max - bf16 min) of the bf16 median; equal launch counts',
                       accuracy='against the fp32 HIP path on the same batch and weights, one step of each kind'),
             timing=timing, verdict=verdict)
  def save():                                 # after every stage: a later child that fails does not cost the earlier ones
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, 'w'), indent=1)
  print(json.dumps(verdict), flush=True)
  save()
  out['accuracy'] = run_child(['--child', 'accuracy'], 420)
  print(json.dumps(out['accuracy']), flush=True)
  save()
  out['trajectory'] = run_child(['--child', 'trajectory', str(a.steps)], 300)
  save()
  print('wrote', a.out)


if __name__ == '__main__':
  main()
