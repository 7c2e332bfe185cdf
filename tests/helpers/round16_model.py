"""CPU (torch float64 only): what ONE rounding to a 16-bit type costs at every place where the 16-bit conv-block kernels store
or read a 16-bit tensor -- the error of test_gpu_kernels16._case's own reference, never a device result.

The places (csrc/conv16.h, csrc/api16.hip, csrc/elementwise16.hip):
  y        the block's cb8 output (not with out_f32: the fp32 accumulators are stored as they are)
  dy       the gradient a cb8 output receives (out_f32 blocks receive fp32)
  dy_raw   after the BatchNorm / activation backward (the `dyr` tensor; out_f32 BARE blocks: the conversion of dy to cb8)
  dx       the data gradient (upsample-add: both outputs, the half-length one from the fp32 pair sum)
  w*scale  folded eval blocks (the inference form) round w * gamma / sqrt(var + eps) once, where the reference rounds w
  x_hat    BN_TRAIN backward recovers x_hat and the activation mask from the stored y where BatchNorm + LeakyReLU invert safely
           (conv16.h: bn_inv_unsafe, per 8-channel block) and from the stored 16-bit y_raw elsewhere (and in out_f32 blocks)
With a loss scale S every gradient is multiplied by S before its rounding and divided by S after it.  dw, dbias, dgamma, dbeta
and the statistics stay fp32 results of rounded inputs.

block_model() returns {check: emulated error} under the names and normalisations of _case ('fwd', 'dw', 'dw l2', ...: max-abs
relative to the exact tensor's max-abs, and relative l2), the exact tensor being fp64 on the rounded operands with the
UNROUNDED incoming gradient; plus 'kink share', the share of pre-activations inside _case's kink band.
(_case's reference shares the dy rounding with the device, so for the checks that rounding dominates -- dbeta, the bias gradient
of a cb8 output, the weight gradient of a LeakyReLU block, where dy_raw = dy or 0.2 dy is all but exact -- the device sits far
below the figure here and 3 x it is a loose bar: a wrong type shows in dgamma / dw / dx of the same case, not in those checks.)

gen_operands() / gen_dy() draw a case's tensors; _case draws from them too, so the CPU tests see the tensors of the GPU run."""
import torch
import torch.nn.functional as F

BARE, LRELU, BN_TRAIN, BN_EVAL = 0, 1, 2, 3
PLAIN, BCAST, UP2 = 0, 1, 2
BN_EPS = 1e-5

# significand bits (hidden one included), exponent of the smallest normal, exponent of the largest binade
FORMATS = {torch.bfloat16: (8, -126, 127), torch.float16: (11, -14, 15)}


def unit_roundoff(dt):
  return 2.0 ** -FORMATS[dt][0]


def round16(v, dt):
  """float64 -> nearest value of `dt` (ties to even, gradual underflow, overflow to inf), computed in float64 arithmetic."""
  p, emin, emax = FORMATS[dt]
  v = v.double()
  fin = torch.isfinite(v)
  vv = torch.where(fin, v, torch.zeros_like(v))
  _, e = torch.frexp(vv)                                      # |vv| = m * 2^e, 0.5 <= m < 1: the leading bit has exponent e - 1
  q = torch.ldexp(torch.ones_like(vv), torch.clamp(e - 1, min=emin) - (p - 1))      # spacing of `dt` at vv
  r = torch.round(vv / q) * q                                 # (torch.round: halves to even)
  big = 2.0 ** emax * (2.0 - 2.0 ** (1 - p))
  r = torch.where(r.abs() > big, torch.sign(vv) * float('inf'), r)
  return torch.where(fin, r, v)


def round16_scaled(v, dt, S=1.0):
  """One gradient rounding under the loss scale S."""
  return round16(v * S, dt) / S


def _two(v):
  return tuple(v) if isinstance(v, tuple) else (v, v)


def out_shape(nd, B, ctot, k, s, p, H, W):
  if nd == 1:
    return (B, ctot, (W + 2 * p - k) // s + 1)
  (kh, kw), (sh, sw), (ph, pw) = _two(k), _two(s), _two(p)
  return (B, ctot, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1)


def gen_operands(nd, B, cin, cout, groups, k, s, p, H, W, in_mode=PLAIN, seed=0, fragile=False):
  """The fp32 tensors of one block (CPU), drawn in _case's order: w, bias, gamma, beta, running statistics, input(s).
  'g' is the generator, left where gen_dy() continues."""
  g = torch.Generator().manual_seed(seed)
  sp = (H, W) if nd == 2 else (W,)
  cin_tot = cin if in_mode == BCAST else cin * groups
  kk = (k, k) if (nd == 2 and not isinstance(k, tuple)) else k
  kt = tuple(kk) if isinstance(kk, tuple) else (kk,)
  fan = cin
  for v in kt:
    fan *= v
  o = dict(g=g)
  o['w'] = torch.randn((cout * groups, cin) + kt, generator=g) * fan ** -0.5
  o['bias'] = torch.randn(cout * groups, generator=g) * 0.1
  o['gamma'] = 0.5 + torch.rand(cout * groups, generator=g)
  o['beta'] = torch.randn(cout * groups, generator=g) * 0.1
  if fragile:
    # channels whose BatchNorm + LeakyReLU map does not invert safely (tiny gamma; beta >> gamma): the backward pass must read
    # x_hat from the kept y_raw for their 8-channel blocks, from y for the others (csrc/conv16.h: bn_inv_unsafe)
    o['gamma'][::13] = 1e-4
    o['beta'][5::17] = 3.0
    o['gamma'][5::17] = 0.5
  o['rm'] = torch.randn(cout * groups, generator=g) * 0.1
  o['rv'] = 0.5 + torch.rand(cout * groups, generator=g)
  if in_mode == UP2:
    o['a'] = torch.randn((B, cin_tot, W // 2), generator=g)
    o['r'] = torch.randn((B, cin_tot, W), generator=g)
  else:
    o['x'] = torch.randn((B, cin_tot) + sp, generator=g)
  return o


def gen_dy(o, shape, dy_scale=1.0):
  """The incoming gradient, elements of size dy_scale (drawn after the operands, as _case always did)."""
  dy = torch.randn(tuple(shape), generator=o['g'])
  return dy if dy_scale == 1.0 else dy * dy_scale


MODES = {'BARE': BARE, 'LRELU': LRELU, 'BN_TRAIN': BN_TRAIN, 'BN_EVAL': BN_EVAL}
IN_MODES = {'plain': PLAIN, 'bcast': BCAST, 'up2': UP2}


def case_tensors(c, dy_scale=1.0):
  """(operands, dy) of an entry of helpers/fp16_block_table.py -- the tensors _case draws for it."""
  nd = c['nd']
  H, W = c['sp'] if nd == 2 else (1, c['sp'][0])
  o = gen_operands(nd, c['B'], c['cin'], c['cout'], c['groups'], c['k'], c['s'], c['p'], H, W, IN_MODES[c['in_mode']], c['seed'],
                   c['fragile'])
  dy = gen_dy(o, out_shape(nd, c['B'], c['cout'] * c['groups'], c['k'], c['s'], c['p'], H, W), dy_scale)
  return o, dy


def case_model(c, dt, S=1.0, dy_scale=1.0, mask=None):
  """block_model() of an entry of helpers/fp16_block_table.py, as _case calls it for that entry."""
  o, dy = case_tensors(c, dy_scale)
  return block_model(o, dy, c['nd'], c['groups'], c['s'], c['p'], MODES[c['mode']], IN_MODES[c['in_mode']], c['slope'], c['out_f32'],
                     dt, S, two_launch=c['bn_fused'] == 0, mask=mask or c['mask'])


def _rel(a, b, floor):
  return ((a - b).abs().max() / (b.abs().max() + floor)).item()


def _l2(a, b):
  return ((a - b).norm() / (b.norm() + 1e-12)).item()


def block_model(o, dy, nd, groups, s, p, mode, in_mode=PLAIN, slope=0.2, out_f32=False, dt=torch.float16, S=1.0, dev='cpu',
                two_launch=False, mask='exact', bn_folded=False):
  """{check: emulated error of the reference} for one block; o: gen_operands' fp32 tensors, dy: the fp32 incoming gradient.
  two_launch: BN_TRAIN normalises the STORED 16-bit conv output in a launch of its own (api16.hip: block_fwd16 -- always so
  for out_f32 blocks, otherwise when the in-launch form is switched off or not resident): one more rounding before y's.
  mask: 'exact' | 'device', as _case's.  bn_folded: BN_EVAL folded into the weights."""
  R = lambda t: round16(t, dt)
  RS = lambda t: round16_scaled(t, dt, S)
  D = lambda t: t.detach().to(dev).double()
  w = R(D(o['w'])).requires_grad_()
  b, gam, bet = D(o['bias']), D(o['gamma']), D(o['beta'])
  if in_mode == UP2:
    xin = R(R(D(o['a'])).repeat_interleave(2, dim=-1) + R(D(o['r'])))      # the kernel adds in fp32 and rounds once
  else:
    xin = R(D(o['x']))
  xin.requires_grad_()
  xcat = torch.cat([xin] * groups, 1) if in_mode == BCAST else xin
  conv = F.conv2d if nd == 2 else F.conv1d
  raw_g = conv(xcat, w, b, stride=s, padding=p, groups=groups)
  raw = raw_g.detach()
  ctot = raw.shape[1]
  dims = (0, 2, 3) if nd == 2 else (0, 2)
  shape = (1, -1, 1, 1) if nd == 2 else (1, -1, 1)
  V = lambda t: t.view(shape)
  dy = D(dy) if dy is not None else None
  sl = slope if mode == BN_TRAIN else 0.2
  out = {}

  # ---- exact forward, the emulated stored output, the kink band
  if mode in (BN_TRAIN, BN_EVAL):
    if mode == BN_TRAIN:
      mean, var = raw.mean(dims), raw.var(dims, unbiased=False)
    else:
      mean, var = D(o['rm']), D(o['rv'])
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    xhat = (raw - V(mean)) * V(invstd)
    z = xhat * V(gam) + V(bet)
    zscale = gam.abs() * invstd
    y = F.leaky_relu(z, sl)
  elif mode == LRELU:
    z, zscale = raw, torch.ones(ctot, dtype=torch.float64, device=raw.device)
    y = F.leaky_relu(z, sl)
  else:
    z, y = None, raw
  y_src = y
  if mode == BN_TRAIN and (two_launch or out_f32):
    y_src = F.leaky_relu((R(raw) - V(mean)) * V(invstd) * V(gam) + V(bet), sl)
  if mode == BN_EVAL and bn_folded:
    # the inference form (conv16.hip: prep16 with a scale; elementwise16.hip: bn_fold_kernel): the weights are w * scale rounded
    # ONCE from fp32 -- another rounding of every weight than the reference's round16(w) -- and the shift enters as the bias
    scale = gam * invstd
    w_f = R(D(o['w']) * scale.view((-1,) + (1,) * (w.dim() - 1)))
    y_src = F.leaky_relu(conv(xcat, w_f, (b - mean) * scale + bet, stride=s, padding=p, groups=groups), sl)
  y_em = y_src if out_f32 else R(y_src)
  y_st = None if (mode == BN_TRAIN and out_f32) else y_em      # what the backward pass reads besides y_raw

  def xhat_mask(y_s, raw_s):
    """BN_TRAIN: x_hat and the activation mask as the backward pass recovers them from the stored tensors."""
    xh_r = (raw_s - V(mean)) * V(invstd)
    pos_r = (xh_r * V(gam) + V(bet)) > 0
    if y_s is None:
      return xh_r, pos_r
    # from y where the map inverts safely, per 8-channel block; from y_raw elsewhere (conv16.h: bn_inv_unsafe)
    unsafe_c = (gam.abs() < 1e-3) | (bet.abs() > 4.0 * gam.abs())
    if not slope >= 1e-3:
      unsafe_c = torch.ones_like(unsafe_c)
    blk = F.pad(unsafe_c, (0, (-ctot) % 8)).view(-1, 8).any(1).repeat_interleave(8)[:ctot]
    zz = torch.where(y_s > 0, y_s, y_s / (slope if slope >= 1e-3 else 1.0))
    xh_y = (zz - V(bet)) / V(torch.where(blk, torch.ones_like(gam), gam))
    return torch.where(V(blk), xh_r, xh_y), torch.where(V(blk), pos_r, y_s > 0)

  # mask='device': _case's reference takes its LeakyReLU slopes from the sign of the device output; the exact tensors here take
  # them from the emulated stored tensors likewise, so that a pre-activation within one rounding of 0 is no error of either
  pos_dev = None
  if mask == 'device' and z is not None:
    pos_dev = xhat_mask(y_st, R(raw))[1] if mode == BN_TRAIN else (y_em > 0)
    y = torch.where(pos_dev, z, sl * z)
  out['fwd'] = _rel(y_em, y, 1e-6)
  if z is not None:
    band = unit_roundoff(dt) * raw.abs() * V(zscale) + 1e-5 * z.abs().max()
    out['kink share'] = (z.abs() <= band).double().mean().item()
  else:
    out['kink share'] = 0.0
  if mode == BN_EVAL or dy is None:
    return out

  def bwd(dyv, y_s, raw_s, rnd, pos=None):
    """dy -> (dy_raw, {parameter gradients}); y_s / raw_s: the stored tensors the kernels read; rnd: the dy_raw rounding."""
    if mode == BN_TRAIN:
      n = raw.numel() // ctot
      xh, pos_s = xhat_mask(y_s, raw_s)
      dz = torch.where(pos_s if pos is None else pos, dyv, dyv * sl)
      s1, s2 = dz.sum(dims), (dz * xh).sum(dims)
      dr = V(gam * invstd) * (dz - V(s1) / n - xh * V(s2) / n)
      return rnd(dr), {'dgamma': s2, 'dbeta': s1}
    if mode == LRELU:
      dr = torch.where((y_s > 0) if pos is None else pos, dyv, dyv * sl)
      return rnd(dr), {'dbias': dr.sum(dims)}
    return (rnd(dyv) if out_f32 else dyv), {'dbias': dyv.sum(dims)}

  def conv_bwd(dr):
    dw, dxin = torch.autograd.grad(raw_g, [w, xin], grad_outputs=dr, retain_graph=True)
    return dw, dxin

  # ---- exact backward (unrounded dy, exact x_hat), then the emulated one
  dr0, par0 = bwd(dy, None if mode == BN_TRAIN else y, raw, lambda t: t, pos_dev)
  dw0, dx0 = conv_bwd(dr0)
  dy_em = dy if out_f32 else RS(dy)
  dr1, par1 = bwd(dy_em, y_st, R(raw), RS)
  dw1, dx1 = conv_bwd(dr1)

  def put(what, a, b_):
    out[what] = _rel(a, b_, 1e-9)
    out[what + ' l2'] = _l2(a, b_)
  put('dw', dw1, dw0)
  for kk in par0:
    put(kk, par1[kk], par0[kk])
  if in_mode == UP2:
    pair = lambda t: t.reshape(t.shape[0], t.shape[1], -1, 2).sum(-1)
    put('dx2', RS(dx1), dx0)
    put('dx', RS(pair(dx1)), pair(dx0))
  else:
    put('dx', RS(dx1), dx0)
  return out
