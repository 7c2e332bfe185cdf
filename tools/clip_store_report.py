"""What the device-resident clip store costs and saves at the headline shape (recorded, no bar): profiles/clip_store.json.

  python tools/clip_store_report.py [--parent-tree DIR] [--out profiles/clip_store.json] [--procs 3]

B = 32, T = 64, P = 104, F = 128, M = S = 8, fp32 and bf16; every figure is measured in `--procs` separate processes and reported as
the median over the processes with its range.
 (a) the draw's launches (ms_clip_draw + ms_clip_advance into the step's static buffers) against the form without the store on a
     device-resident raw batch: DevicePreStep.__call__ (three launches) plus the step's copy_multi.  Host-paced loops of 80, wall clock
     per iteration: the cost is launch latency, not bandwidth (1.9 MB in, 1.9 MB out).
 (b) G- and D-step ms of MixStageTrainStep.step_from against ts.step() fed a device-resident pre-processed batch (the copy included,
     inputs_unchanged=False), graphs on, loops of 40 steps, median of 5 loops.
--parent-tree DIR: a built checkout of the parent commit; its ts.step() is measured in the same way (same box, same processes
count) and reported beside this tree's -- the parent has no store, so only the step() figures exist there."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, P, F, M, S = 32, 64, 104, 128, 8, 8


def _loop_ms(fn, n, reps=5, sync=None, before=None):
  """ms per call of fn over loops of n, median of reps; `before` runs ahead of every loop, outside the timed region."""
  out = []
  for _ in range(reps):
    if before is not None:
      before()
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
      fn()
    sync()
    out.append((time.perf_counter() - t0) * 1e3 / n)
  return sorted(out)[len(out) // 2]


def child(tree, step_only):
  sys.path.insert(0, tree)
  sys.path.insert(0, os.path.join(tree, 'tests'))
  import numpy as np
  import torch
  import mix_stage_amd as A
  from mix_stage_amd import ops
  from mix_stage_amd.train_step import MixStageTrainStep
  from test_gpu_model import build_hip_gan
  dev = 'cuda:0'
  sync = torch.cuda.synchronize
  rng = np.random.default_rng(0)
  n_int, n_frames = 40, 400
  poses = [(rng.standard_normal((1, P)) * 40 + 100 + np.cumsum(rng.standard_normal((n_frames, P)), axis=0)).astype(np.float32) for _ in range(n_int)]
  audios = [rng.standard_normal((n_frames, F)).astype(np.float32) for _ in range(n_int)]
  rows, arows = np.concatenate(poses).astype(np.float64), np.concatenate(audios).astype(np.float64)
  centers = np.concatenate([rows[rng.choice(len(rows), M, replace=False)], rng.standard_normal((M, P))], axis=1)
  pre = A.DevicePreStep(centers, rows.mean(0), rows.var(0), arows.mean(0), arows.var(0), mask=(), device=dev)
  # a device-resident raw batch and its pre-processed form: what a caller without the store holds
  first = [i * n_frames for i in range(B)]
  raw_pose = torch.from_numpy(np.stack([rows[s:s + T] for s in first]).astype(np.float32)).to(dev)
  raw_audio = torch.from_numpy(np.stack([arows[s:s + T] for s in first]).astype(np.float32)).to(dev)
  audio, labels, y = pre(raw_pose, raw_audio)
  style = torch.arange(B, device=dev)[:, None].expand(-1, T).contiguous() % S
  out = dict(tree=os.path.abspath(tree))
  store = None
  if not step_only:
    store = A.DeviceClipStore([(torch.from_numpy(p), torch.from_numpy(a), i % S) for i, (p, a) in enumerate(zip(poses, audios))],
                              T=T, hop=5, device=dev, batch_size=B)
    store.new_epoch()
    static = [torch.zeros_like(audio), torch.zeros_like(labels), torch.zeros_like(y), torch.zeros_like(style)]

    def parent_form():
      a, l, yy = pre(raw_pose, raw_audio)
      ops.copy_multi([(static[0], a), (static[1], l), (static[2], yy), (static[3], style)])
    # (an epoch of the store holds 85 steps: every timed loop starts a fresh one, outside the timed region)
    out['draw_ms'] = _loop_ms(lambda: store._launch(pre, *static, None), 80, reps=7, sync=sync, before=store.new_epoch)
    out['prestep_plus_copy_ms'] = _loop_ms(parent_form, 80, reps=7, sync=sync)
  for dtype in ('fp32', 'bf16'):
    torch.manual_seed(5)
    model = build_hip_gan(M, S)
    if dtype != 'fp32':
      A.set_compute_dtype(model, dtype)
    ts = MixStageTrainStep(model, use_graphs=True)
    for kind in ('G', 'D'):
      for _ in range(3):
        ts.step(audio, labels, y, style, kind=kind)
      out['step_%s_%s_ms' % (kind, dtype)] = _loop_ms(lambda: ts.step(audio, labels, y, style, kind=kind), 40, sync=sync)
      if store is not None:
        store.new_epoch()
        for _ in range(3):
          ts.step_from(store, pre, kind=kind)
        out['step_from_%s_%s_ms' % (kind, dtype)] = _loop_ms(lambda: ts.step_from(store, pre, kind=kind), 40, sync=sync, before=store.new_epoch)
    ts.check_health()
  if store is not None:
    store.check()
  print('CLIPSTORE ' + json.dumps(out), flush=True)


def _spread(values):
  v = sorted(values)
  return dict(median=v[len(v) // 2], min=v[0], max=v[-1], range=v[-1] - v[0], processes=len(v))


def _child(tree, step_only):
  cmd = [sys.executable, os.path.abspath(__file__), '--child', '--tree', tree] + (['--step-only'] if step_only else [])
  res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
  lines = [l for l in res.stdout.splitlines() if l.startswith('CLIPSTORE ')]
  if res.returncode != 0 or not lines:
    raise RuntimeError('child failed (%d): %s' % (res.returncode, res.stderr[-2000:]))
  print('done: %s' % lines[-1][:200], file=sys.stderr, flush=True)
  return json.loads(lines[-1][len('CLIPSTORE '):])


def _summary(runs):
  return {k: _spread([r[k] for r in runs]) for k in runs[0] if k != 'tree'}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_store.json'))
  ap.add_argument('--parent-tree', default=None)
  ap.add_argument('--procs', type=int, default=3)
  ap.add_argument('--child', action='store_true')
  ap.add_argument('--tree', default=ROOT)
  ap.add_argument('--step-only', action='store_true')
  a = ap.parse_args()
  if a.child:
    return child(a.tree, a.step_only)
  report = dict(what='clip store at B=%d T=%d P=%d F=%d M=S=%d: ms, median over %d processes with the range; (a) draw_ms vs '
                     'prestep_plus_copy_ms: host-paced loops of 80; (b) step_from vs step(): graphs on, loops of 40 steps, median of 5'
                     % (B, T, P, F, M, a.procs))
  mine, parent = [], []
  for _ in range(a.procs):          # the two trees alternate: a drift of the box falls on both
    if a.parent_tree:
      parent.append(_child(os.path.abspath(a.parent_tree), True))
    mine.append(_child(ROOT, False))
  report['this_tree'] = _summary(mine)
  if a.parent_tree:
    report['parent_tree_step'] = _summary(parent)
  with open(a.out, 'w') as fh:
    json.dump(report, fh, indent=1)
    fh.write('\n')
  print(json.dumps(report))


if __name__ == '__main__':
  main()
