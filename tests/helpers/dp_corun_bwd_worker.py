"""Worker of tests/test_gpu_clip_corun_bwd.py::test_global_bn_two_ranks_make_the_backward_corun_stand_aside: one data-parallel
rank (gloo, all ranks on cuda:0) with bn_sync='global'.  The generator forward and backward on this rank's clips with the backward
co-run switched on and off; one JSON record per rank: data gradients held back, merged launch labels, a digest of every result."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch
import torch.distributed as dist

from oracle import mixstage_oracle as O


def main():
  rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
  dist.init_process_group('gloo', rank=rank, world_size=world)
  torch.cuda.set_device(0)
  from mix_stage_amd import ops, ops16
  from test_gpu_clip_corun import PAIR_MARK, _g_forward, _gan, _labels
  ops.set_bn_sync(True)
  ops16.set_in_launch_meetings(False)      # (two processes share the device: as the trainer does there, train_step.py)
  M = S = 2
  Bl = 2
  batch = O.synthetic_batch(Bl * world, M=M, S=S, seed=17)
  mine = [t[rank * Bl:(rank + 1) * Bl].contiguous() for t in batch]
  rec = dict(rank=rank, bn_sync_active=bool(ops.bn_sync_active()), offered={}, fwd_offered={}, merged={}, digest={})
  for name, on in (('on', True), ('off', False)):
    torch.manual_seed(77)
    model = _gan(M, S)
    old = ops.enable_corun_bwd(on)
    try:
      b0, f0 = ops._corun['bwd_offered'], ops._corun['merges_offered']
      res = {}
      labels = _labels(lambda: res.update(_g_forward(model, mine, True, backward=True)))
      rec['offered'][name] = ops._corun['bwd_offered'] - b0
      rec['fwd_offered'][name] = ops._corun['merges_offered'] - f0
      rec['merged'][name] = sum(c for k, c in labels.items() if PAIR_MARK in k)
    finally:
      ops.enable_corun_bwd(old)
    h = hashlib.sha1()
    for k in sorted(res):
      h.update(k.encode())
      h.update(res[k].detach().contiguous().cpu().numpy().tobytes())
    rec['digest'][name] = h.hexdigest()
    rec['n_tensors'] = len(res)
  torch.cuda.synchronize()
  with open(os.path.join(os.environ['DP_RESULT_DIR'], 'rank%d.json' % rank), 'w') as f:
    json.dump(rec, f)
  dist.barrier()
  dist.destroy_process_group()


if __name__ == '__main__':
  main()
