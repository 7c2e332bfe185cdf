#!/usr/bin/env python3
"""Times the eval form of the chained decoder (ms_decoder_chain_eval_fwd) against the blocks one by one for inference shapes.

  python tools/probe_chain_eval.py 1024,8,64,fp16 1,8,640,fp32 1,25,1024,bf16 [--repeats 7] [--launches 10]
                                   [--sampler 10,40] [--json profiles/chain_eval.json] [--commit HASH]

Each positional argument is B,M,T,dtype.  Per shape: warm-up, then `repeats` rounds; a round times `launches` eager launches of
each path between two HIP events, the two paths in alternating order from round to round.  Reported: median, min and max of the
rounds in us per forward, TF/s from the algorithmic FLOPs of the useful frames and the share of the dtype's matrix peak.
--sampler n: StyleTransferSampler.sample_interval on n windows (M = S = 8, graphs on), ms per style with the eval form on / off."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch
import torch.nn as nn

from test_gpu_chain import _build, _inputs

PEAK_TF = {'fp32': 157.3, 'bf16': 2500.0, 'fp16': 2500.0}


def _events(fn, launches):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(launches):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) * 1e3 / launches


def probe_shape(B, M, T, dtn, repeats, launches):
  import mix_stage_amd as A
  from mix_stage_amd import ops, ops16
  from mix_stage_amd.layers import bare_conv
  P = 104
  blocks, logits = _build(M, P, 10)
  x, score = _inputs(B, M, 266, T=T)
  if dtn != 'fp32':
    A.set_compute_dtype(nn.ModuleList(list(blocks) + [logits]), dtn)
    x = ops16.to_cb8(x, ops16.NAME_DT[dtn])
  for m in blocks:
    m.eval()

  def chain():
    res = (ops.decoder_chain if dtn == 'fp32' else ops16.decoder_chain16)(x, blocks, logits, score, P)
    assert res is not None, 'the eval form declined %s' % ((B, M, T, dtn),)
    return res

  def one_by_one():
    z = blocks[0].forward_broadcast(x)
    for m in blocks[1:]:
      z = m(z)
    z = bare_conv(logits, z, out_f32=True)
    return ops.softmax_mix(z, score, P)

  times = {'eval_form': [], 'blocks': []}
  with torch.no_grad():
    for _ in range(3):
      chain(); one_by_one()
    torch.cuda.synchronize()
    for r in range(repeats):
      order = [('eval_form', chain), ('blocks', one_by_one)]
      for name, fn in (order if r % 2 == 0 else order[::-1]):
        times[name].append(_events(fn, launches))
  gflop = 2.0 * B * T * M * (256 * 3 * (266 + 3 * 256) + P * 256) / 1e9
  rec = dict(kind='decoder_segment', B=B, M=M, T=T, dtype=dtn, repeats=repeats, launches_per_repeat=launches, gflop_useful=gflop)
  for name, v in times.items():
    med = statistics.median(v)
    rec[name] = dict(us_median=med, us_min=min(v), us_max=max(v), tf=gflop / med * 1e3, share_of_peak=gflop / med * 1e3 / PEAK_TF[dtn])
  rec['speedup'] = rec['blocks']['us_median'] / rec['eval_form']['us_median']
  print('%-5s B=%d M=%d T=%d: eval form %.1f us [%.1f, %.1f] = %.1f TF (%.3f of peak); blocks one by one %.1f us [%.1f, %.1f] = %.1f TF; x%.2f' %
        (dtn, B, M, T, rec['eval_form']['us_median'], rec['eval_form']['us_min'], rec['eval_form']['us_max'], rec['eval_form']['tf'],
         rec['eval_form']['share_of_peak'], rec['blocks']['us_median'], rec['blocks']['us_min'], rec['blocks']['us_max'], rec['blocks']['tf'],
         rec['speedup']), flush=True)
  return rec


def probe_sampler(n, repeats):
  from oracle import mixstage_oracle as O
  from test_gpu_model import build_hip_gan
  from mix_stage_amd import ops
  from mix_stage_amd.sample import StyleTransferSampler
  M = S = 8
  audio, pose, labels, style = [t.to('cuda:0') for t in O.synthetic_batch(n, M=M, S=S)]
  style = torch.full_like(style, 2)
  hip = build_hip_gan(M, S)
  samplers, times = {}, {'eval_form': [], 'blocks': []}
  for name, on in (('eval_form', True), ('blocks', False)):
    ops.USE_DECODER_CHAIN_EVAL = on
    samplers[name] = StyleTransferSampler(hip, num_styles=S, use_graphs=True)
    samplers[name].sample_interval(audio, labels, pose, style)          # captures the graph
  ops.USE_DECODER_CHAIN_EVAL = True
  for r in range(repeats):
    for name in (('eval_form', 'blocks') if r % 2 == 0 else ('blocks', 'eval_form')):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      samplers[name].sample_interval(audio, labels, pose, style)
      b.record()
      torch.cuda.synchronize()
      times[name].append(a.elapsed_time(b) / S)
  rec = dict(kind='sample_interval', windows=n, M=M, S=S, graphs=True, repeats=repeats)
  for name, v in times.items():
    rec[name] = dict(ms_per_style_median=statistics.median(v), ms_per_style_min=min(v), ms_per_style_max=max(v))
  print('sampler n=%d: eval form %.3f ms per style [%.3f, %.3f]; blocks one by one %.3f [%.3f, %.3f]' %
        (n, rec['eval_form']['ms_per_style_median'], rec['eval_form']['ms_per_style_min'], rec['eval_form']['ms_per_style_max'],
         rec['blocks']['ms_per_style_median'], rec['blocks']['ms_per_style_min'], rec['blocks']['ms_per_style_max']), flush=True)
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('shapes', nargs='*', help='B,M,T,dtype')
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--launches', type=int, default=10)
  ap.add_argument('--sampler', default='', help='comma-separated window counts')
  ap.add_argument('--json', default='')
  ap.add_argument('--commit', default='')
  a = ap.parse_args()
  recs = []
  for spec in a.shapes:
    B, M, T, dtn = spec.split(',')
    recs.append(probe_shape(int(B), int(M), int(T), dtn, a.repeats, a.launches))
  for n in [int(v) for v in a.sampler.split(',') if v]:
    recs.append(probe_sampler(n, a.repeats))
  if a.json:
    out = dict(command='python tools/probe_chain_eval.py ' + ' '.join(sys.argv[1:]), commit=a.commit, device=torch.cuda.get_device_name(0),
               records=recs)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    json.dump(out, open(a.json, 'w'), indent=1)


if __name__ == '__main__':
  main()
