"""Reference and comparison helpers of tests/test_gpu_wgrad_queue.py, kept free of the device so that
tests/test_wgrad_queue_table_cpu.py can show on CPU tensors that each of them rejects what it is meant to reject.

The reference is the one of test_gpu_dispatch_parity._run_fp32 (fp32 blocks: the block in float64, the LeakyReLU slope mask taken from
the device output) and of test_gpu_kernels16._case (16-bit blocks: float64 on the 16-bit-rounded operands, mask='device'), written
for a block whose module is used once or twice in the backward pass; the bars are theirs, by value and by name:
  fp32     forward 2e-5, gradients 1e-4 of the tensor's max-abs, running statistics 1e-5, at most KINK_MAX slope flips, each
           within 2e-5 of 0 (relative to max |z|), the conv bias gradient before BatchNorm ~ 0
  16-bit   forward 1.2e-2 (2e-5 for fp32 outputs without BatchNorm), gradients 2e-2 (1e-2: fp32 output, no activation) in l2 and
           twice that in max-abs, running mean 1e-4 absolute / running variance 2e-3, slope flips at most 2e-3 of the output and none
           beyond one 16-bit rounding of the conv output."""
import torch
import torch.nn.functional as F

KINK_MAX = 8                   # test_gpu_dispatch_parity.KINK_MAX (tests/test_wgrad_queue_table_cpu.py holds the two equal)
DT16 = {'bf16': torch.bfloat16, 'fp16': torch.float16}
PARAMS = ('dw', 'dbias', 'dgamma', 'dbeta')


def rel_err(a, b):
  """test_gpu_dispatch_parity.rel_err"""
  a, b = a.detach().double().cpu(), b.detach().double().cpu()
  assert a.shape == b.shape, (a.shape, b.shape)
  return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def same_bits(a, b):
  if a is None or b is None:
    return a is None and b is None
  return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def flat_results(r):
  """{name: tensor} of one block's results (per-use lists flattened)."""
  out = {}
  for k, v in r.items():
    if isinstance(v, (list, tuple)):
      out.update({'%s[%d]' % (k, u): t for u, t in enumerate(v)})
    else:
      out[k] = v
  return out


def differing(a, b, keys=None):
  """Names of the results of two runs of a block that are not bit for bit equal."""
  fa, fb = flat_results(a), flat_results(b)
  assert sorted(fa) == sorted(fb), (sorted(fa), sorted(fb))
  return [k for k in sorted(fa) if (keys is None or k.split('[')[0] in keys) and not same_bits(fa[k], fb[k])]


def _nd_kernel(b):
  if b['nd'] == 1:
    return b['k'], b['s'], b['p']
  two = lambda v: tuple(v) if isinstance(v, tuple) else (v, v)
  return two(b['k']), two(b['s']), two(b['p'])


def _round(t, dt):
  return t.double() if dt is None else t.to(dt).to(torch.float64)


def reference(b, params, uses, rm0=None, rv0=None, dev='cpu', slope=0.2, eps=1e-5, momentum=0.1):
  """float64 reference of one block.  params: dict(w, bias, gamma, beta) fp32 tensors (gamma / beta None without BatchNorm);
  uses: [dict(xs=[x] or [a, residual], gy=upstream gradient, y=the device's output (for the slope mask))], in forward order.
  -> dict(y=[..], dx0=[..], dx1=[..], dw, dbias, dgamma, dbeta, rm, rv, aux=[per use: z, raw, zscale, n]) in float64."""
  dt = DT16.get(b['prec'])
  nd, g, mode = b['nd'], b['groups'], b['mode']
  k, s, p = _nd_kernel(b)
  w = _round(params['w'].detach().to(dev), dt).requires_grad_()
  bias = params['bias'].detach().to(dev).double().requires_grad_()
  bn = mode == 'BN_TRAIN'
  gamma = params['gamma'].detach().to(dev).double().requires_grad_() if bn else None
  beta = params['beta'].detach().to(dev).double().requires_grad_() if bn else None
  rm = rm0.detach().to(dev).double().clone() if bn else None
  rv = rv0.detach().to(dev).double().clone() if bn else None
  conv = F.conv2d if nd == 2 else F.conv1d
  dims = (0, 2, 3) if nd == 2 else (0, 2)
  shape = (1, -1, 1, 1) if nd == 2 else (1, -1, 1)
  out = dict(y=[], dx0=[], dx1=[], aux=[])
  for use in uses:
    xs = [x.detach().to(dev) for x in use['xs']]
    if b['in_mode'] == 'up2':
      if dt is None:
        leaves = [xs[0].double().requires_grad_(), xs[1].double().requires_grad_()]
        xin = F.interpolate(leaves[0], scale_factor=2, mode='nearest') + leaves[1]
      else:
        # the kernel adds the two 16-bit tensors and rounds the sum once (test_gpu_kernels16._case)
        a64, r64 = _round(xs[0], dt), _round(xs[1], dt)
        xin = _round((a64.repeat_interleave(2, dim=-1) + r64).float(), dt).requires_grad_()
        leaves = [xin]
    else:
      xin = _round(xs[0], dt).requires_grad_()
      leaves = [xin]
    xcat = torch.cat([xin] * g, 1) if b['in_mode'] == 'bcast' else xin
    raw = conv(xcat, w, bias, stride=s, padding=p, groups=g)
    n = raw.numel() // raw.shape[1]
    if bn:
      mean, var = raw.mean(dims), raw.var(dims, unbiased=False)
      z = (raw - mean.view(shape)) / torch.sqrt(var.view(shape) + eps) * gamma.view(shape) + beta.view(shape)
      zscale = gamma.detach().abs() / torch.sqrt(var.detach() + eps)
      rm = (1 - momentum) * rm + momentum * mean.detach()
      if n > 1:
        rv = (1 - momentum) * rv + momentum * raw.detach().var(dims, unbiased=True)
    else:
      z, zscale = raw, torch.ones(raw.shape[1], dtype=torch.float64, device=raw.device)
    if mode == 'BARE':
      y_ref = z
    else:
      pos = use['y'].detach().to(dev) > 0
      y_ref = torch.where(pos, z, slope * z)
    gy = use['gy'].detach().to(dev)
    y_ref.backward(gy.double() if (dt is None or b['out_f32']) else _round(gy, dt))      # cb8 outputs receive a 16-bit gradient
    out['y'].append(y_ref.detach())
    if b['in_mode'] == 'up2' and dt is not None:
      dxin = xin.grad
      out['dx0'].append(dxin.reshape(dxin.shape[0], dxin.shape[1], -1, 2).sum(-1))
      out['dx1'].append(dxin)
    else:
      out['dx0'].append(leaves[0].grad)
      out['dx1'].append(leaves[1].grad if len(leaves) > 1 else None)
    out['aux'].append(dict(z=z.detach(), raw=raw.detach(), zscale=zscale, n=n))
  out.update(dw=w.grad, dbias=bias.grad, dgamma=gamma.grad if bn else None, dbeta=beta.grad if bn else None, rm=rm, rv=rv)
  return out


def bars(b, got, ref):
  """{check: (measured, bar)} of one block's results against reference(); every bar is the one the module docstring names."""
  dt = DT16.get(b['prec'])
  mode, bn = b['mode'], b['mode'] == 'BN_TRAIN'
  shape = (1, -1, 1, 1) if b['nd'] == 2 else (1, -1, 1)
  errs = {}
  dev = ref['dw'].device
  on = lambda t: t.detach().to(dev).double()
  if dt is None:
    for u, (y, y_ref, aux) in enumerate(zip(got['y'], ref['y'], ref['aux'])):
      if mode != 'BARE':
        z = aux['z']
        flip = (on(y) > 0) != (z > 0)
        zmax = z.abs().max().item()
        errs['kinks (count)[%d]' % u] = (int(flip.sum().item()), KINK_MAX)
        errs['|z| at a kink[%d]' % u] = ((z[flip].abs().max().item() if flip.any() else 0.0) / zmax, 2e-5)
      errs['fwd[%d]' % u] = (rel_err(y, y_ref), 2e-5)
      errs['dx0[%d]' % u] = (rel_err(got['dx0'][u], ref['dx0'][u]), 1e-4)
      if ref['dx1'][u] is not None:
        errs['dx1[%d]' % u] = (rel_err(got['dx1'][u], ref['dx1'][u]), 1e-4)
    errs['dw'] = (rel_err(got['dw'], ref['dw']), 1e-4)
    if bn:
      errs['dgamma'] = (rel_err(got['dgamma'], ref['dgamma']), 1e-4)
      errs['dbeta'] = (rel_err(got['dbeta'], ref['dbeta']), 1e-4)
      errs['dbias(~0)'] = (got['dbias'].abs().max().item(), 1e-4 * max(ref['dw'].abs().max().item(), 1.0))
      errs['running_mean'] = (rel_err(got['rm'], ref['rm']), 1e-5)
      errs['running_var'] = (rel_err(got['rv'], ref['rv']), 1e-5)
    else:
      errs['dbias'] = (rel_err(got['dbias'], ref['dbias']), 1e-4)
    return errs

  # ---- 16-bit: test_gpu_kernels16._case
  u16 = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
  out_tol = 2e-5 if (b['out_f32'] and not bn) else 1.2e-2
  for u, (y, y_ref, aux) in enumerate(zip(got['y'], ref['y'], ref['aux'])):
    if mode != 'BARE':
      z, raw = aux['z'], aux['raw']
      flip = (on(y) > 0) != (z > 0)
      band = u16 * raw.abs() * aux['zscale'].view(shape) + 1e-5 * z.abs().max().item()
      errs['mask flips (fraction)[%d]' % u] = (flip.sum().item() / flip.numel(), 2e-3)
      errs['mask flips beyond one rounding[%d]' % u] = (int((flip & (z.abs() > band)).sum().item()), 0)
    scale = y_ref.abs().max().item() + 1e-6
    errs['fwd[%d]' % u] = ((on(y) - y_ref).abs().max().item() / scale, out_tol)
  tol = 2e-2 if (mode in ('BN_TRAIN', 'LRELU') or not b['out_f32']) else 1e-2

  def close(a, r, what):
    sc = r.abs().max().item() + 1e-9
    d = on(a) - r
    errs[what] = (d.abs().max().item() / sc, 2 * tol + 1e-6 / sc)
    errs[what + ' l2'] = (d.norm().item() / (r.norm().item() + 1e-12), tol)
  close(got['dw'], ref['dw'], 'dw')
  if bn:
    close(got['dgamma'], ref['dgamma'], 'dgamma')
    close(got['dbeta'], ref['dbeta'], 'dbeta')
    errs['running_mean (abs)'] = ((on(got['rm']) - ref['rm']).abs().max().item(), 1e-4)
    if all(a['n'] > 1 for a in ref['aux']):
      errs['running_var'] = ((on(got['rv']) - ref['rv']).abs().max().item() / (1 + ref['rv'].abs().max().item()), 2e-3)
  else:
    close(got['dbias'], ref['dbias'], 'dbias')
  for u in range(len(got['y'])):
    close(got['dx0'][u], ref['dx0'][u], 'dx0[%d]' % u)
    if ref['dx1'][u] is not None:
      close(got['dx1'][u], ref['dx1'][u], 'dx1[%d]' % u)
  return errs


def failed(errs):
  return {k: v for k, v in errs.items() if not v[0] <= v[1]}


def check_labels(entry, labels):
  """labels: {label: launches}.  The entry's expect / forbid regexes, and: the multi-job launches and the slab reductions of the pass
  are exactly the claimed ones (a stale or foreign job would show as another jobsN / wgsN or as one launch more)."""
  import re
  missing = [rx for rx in entry['expect'] if not any(re.search(rx, l) for l in labels)]
  present = [(rx, l) for rx in entry['forbid'] for l in labels if re.search(rx, l)]
  multi = {l: n for l, n in labels.items() if re.search(r'\|conv_wgrad_\w+ multi |^wgrad_reduce_multi ', l)}
  foreign = [l for l in multi if not any(re.search(rx, l) for rx in entry['expect'])]
  want_n = len(entry['claims']['launches']) + len(entry['claims']['reduce_jobs'])
  ok = not missing and not present and not foreign and sum(multi.values()) == want_n
  assert ok, ('%s: expected %s; forbidden %s; not claimed %s; %d multi-job launches, %d claimed; launches: %s'
              % (entry['id'], missing, present, foreign, sum(multi.values()), want_n, sorted(labels.items())))
