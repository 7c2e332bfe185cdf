"""GPU: dropout p > 0 at the model level against the float64 oracle.  GAN(JointLateClusterSoftStyle4_G(p=0.1), Speech2Gesture_D(p=0.1))
at the golden size of tests/test_gpu_model.py (B = 4, T = 64, M = S = 8), a G-step and a D-step.  The oracle's `dropout`
sub-modules are replaced HERE by a module that multiplies with the mask the Python mirror (tests/helpers/philox_ref.py) gives for the
same (module id, visit, step) -- the masks are not torch's, so torch's own nn.Dropout cannot be the reference.

Bars, those of test_gpu_model._compare_step: pose L1 <= 1e-4, losses <= 1e-4, gradients within 2e-3 of the parameter's max |grad|
on a flip-free draw (else 3 % relative L2 and a 15 % per-element cap).  A conv bias in front of batch statistics of DROPPED values
has a real gradient (the sum of dy_raw over the kept values): it takes the bar of every other parameter; in front of the batch
statistics of a p = 0 block (the reference builds the cluster classifier without handing p on) it is 0, 5e-5 absolute as there.

Fails without the feature: the first p > 0 block raised NotImplementedError."""
import pytest
import torch

from helpers import philox_ref as R
from oracle import mixstage_oracle as O
from test_gpu_dropout import SEED, _build_gan
from test_gpu_model import DEV, _count_kink_flips, _record_block_outputs, _step

pytestmark = pytest.mark.gpu

M = S = 8
B = 4
P_DROP = 0.1


class _MirrorMask(torch.nn.Module):
  """x * mask / (1 - p) with the mirror's mask of (module id, visit, step); the identity in eval mode, like nn.Dropout."""

  def __init__(self, module_id, p, channelwise):
    super().__init__()
    self.module_id, self.p, self.channelwise, self.visit, self.step = module_id, p, channelwise, 0, 0

  def forward(self, x):
    if not self.training:
      return x
    site = R.site_of(self.module_id, self.visit)
    self.visit += 1
    mask = R.mask_like(tuple(x.shape), self.p, R.seed_words(SEED), site, self.step, self.channelwise)
    return x * torch.from_numpy(mask).to(x.dtype)


def _pair_of_models():
  import mix_stage_amd as A
  hip = _build_gan(P_DROP, M, S)
  ref = O.build_gan(M=M, S=S, dtype=torch.float64, p=P_DROP)
  hb = [(n, m) for n, m in hip.named_modules() if isinstance(m, A.ConvNormRelu)]
  rb = [(n, m) for n, m in ref.named_modules() if isinstance(m, O.ConvNormRelu)]
  assert [n for n, _ in hb] == [n for n, _ in rb]
  assert A.number_dropout_sites(hip) == len(hb)
  masks = []
  for i, ((_, h), (_, r)) in enumerate(zip(hb, rb)):
    assert h._drop_id == i
    if h._p:
      r.dropout = _MirrorMask(i, h._p, isinstance(r.conv, torch.nn.Conv2d))
      masks.append(r.dropout)
    else:
      assert r.dropout.p == 0
  return hip, ref, masks


@pytest.mark.parametrize('kind', ['G', 'D'])
def test_dropout_step_matches_oracle(kind):
  import mix_stage_amd as A
  from mix_stage_amd import layers
  A.manual_dropout_seed(SEED)
  batch = O.synthetic_batch(B, M=M, S=S, seed=77)
  hip, ref, masks = _pair_of_models()
  assert len(masks) == len(layers.dropout_blocks(hip)) > 40
  rec_r, h_r = _record_block_outputs(ref, lambda m: isinstance(m, O.ConvNormRelu))
  rec_h, h_h = _record_block_outputs(hip, lambda m: isinstance(m, A.ConvNormRelu))
  f_ref, l_ref = _step(ref, [t.double() if t.is_floating_point() else t for t in batch], kind, 'cpu')
  f_hip, l_hip = _step(hip, batch, kind, DEV)
  for h in h_r + h_h:
    h.remove()
  # both sides drew the same sites: the visit counts agree block by block, and D ran twice in the D-step on two masks
  visits_h = [b._drop_visit for b in layers.dropout_blocks(hip)]
  assert visits_h == [m.visit for m in masks] and max(visits_h) >= 1
  d_blocks = [b for b in layers.dropout_blocks(hip) if any(b is m for m in hip.D.modules())]
  assert len(d_blocks) == 2 and all(b._drop_visit == (2 if kind == 'D' else 1) for b in d_blocks)
  if kind == 'D':
    assert all(b._drop_visit == 0 for b in layers.dropout_blocks(hip.G))        # (G runs in eval mode there: no mask drawn)
  flips = _count_kink_flips(rec_h, rec_r)
  l1 = (f_hip.detach().cpu().double() - f_ref.detach()).abs().mean().item()
  print(kind, 'pose L1 %.3g flips %d' % (l1, flips))
  assert l1 <= 1e-4, 'pose L1 %g' % l1
  for a, b in zip(l_hip, l_ref):
    assert abs(float(a) - float(b)) <= 1e-4, (float(a), float(b))
  dropping_bias = set(n + '.conv.bias' for n, m in hip.named_modules() if isinstance(m, A.ConvNormRelu) and m._p)
  bad, compared = [], 0
  for (n, p), (_, q) in zip(hip.named_parameters(), ref.named_parameters()):
    if q.grad is None or p.grad is None:
      if (q.grad is None) != (p.grad is None or p.grad.abs().max().item() == 0) and not (kind == 'G' and n.startswith('D.')):
        bad.append((n, 'gradient on one side only'))
      continue
    compared += 1
    scale = q.grad.abs().max().item()
    diff = p.grad.cpu().double() - q.grad
    err = diff.abs().max().item()
    if n.endswith('conv.bias') and (n not in dropping_bias or scale < 5e-5):
      # a p == 0 block: the true gradient is 0, both sides hold the rounding noise of a sum over the channel -- test_gpu_model's bar for
      # it, 5e-5 absolute.  The same sum behind a mask that happens to keep the whole channel (or whose reference gradient lies
      # below that noise) is held to the same figure
      if err > 5e-5:
        bad.append((n, err, scale))
    elif not flips:
      if err > 2e-3 * scale + 1e-7:
        bad.append((n, err, scale))
    else:
      l2 = diff.norm().item() / (q.grad.norm().item() + 1e-30)
      if err > 0.15 * scale + 1e-7 or l2 > 3e-2:
        bad.append((n, err, scale, l2))
  assert compared > 8 and not bad, 'flips=%d %s' % (flips, bad[:8])
  # the running statistics moved as the oracle's did
  after, ref_after = hip.state_dict(), ref.state_dict()
  for k, v in after.items():
    if k.endswith('num_batches_tracked'):
      assert int(v) == int(ref_after[k]), k
    elif '.norm.running_' in k:
      assert (v.cpu().double() - ref_after[k]).abs().max().item() <= 1e-4 * (1 + ref_after[k].abs().max().item()), k
