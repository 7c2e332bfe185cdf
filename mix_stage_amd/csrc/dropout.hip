// Dropout inside the ConvNormRelu block (layers.py:32-78 with p > 0): conv (+bias) -> dropout(p) -> BatchNorm -> (Leaky)ReLU.
// The conv runs as the block's MS_BARE launch and leaves y_raw UNDROPPED; the kernels here are the BatchNorm passes of the block
// with the mask regenerated wherever a value of y_raw is read (dropout_mask.h: a counter-based generator, no mask tensor in
// memory): the batch statistics are those of the dropped values x = m * y_raw, m = 0 or 1 / (1 - p).
//   forward   x -> (sum, M2) -> save = mean | invstd | scale | shift, running statistics -> y = lrelu(x * scale + shift)
//   backward  dz = dy * lrelu'(x * scale + shift), x_hat = (x - mean) * invstd,
//             dy_raw = m * gamma * invstd * (dz - mean(dz) - x_hat * mean(dz * x_hat));  dgamma = sum dz * x_hat, dbeta = sum dz
// FZ (frozen BatchNorm, layers.freeze_batchnorm): scale / shift come from the running statistics, which are only read, and the
// backward drops the two batch-mean terms (bn_bwd_out<true>).
// The channel arithmetic is that of bn_passes.h, shared with the forms without dropout; what is added here is the mask policy DropMask.
//   one launch   one workgroup owns a channel of at most 256 * 16 values and keeps them in registers: dropout_bn_fwd_fused_kernel<NE>
//                (bn_reg_moments + bn_channel, as splitk_fwd_epilogue_kernel<NE>) and dropout_bn_bwd_fused_kernel<NE> (bn_bwd_elem / bn_bwd_out)
//   two passes   larger channels, over chunks of batch items: bn_stats_kernel<DropMask> + dropout_bn_apply_kernel (bn_combine_tiles +
//                bn_channel) forward, bn_bwd_reduce_kernel<DropMask, float> + bn_bwd_apply_kernel<FZ, DropMask, false> backward -- the
//                kernels of the plain block, instantiated with the mask
// No workgroup waits for another; every reduction runs in a fixed order (no float atomics): the same bits run to run, captured or eager.
#include <algorithm>

#include <stdint.h>

#include "kernels.h"
#include "bn_passes.h"
#include "dropout_mask.h"

namespace ms {

constexpr int DROPOUT_FUSED_MAX = 256 * 16;      // values per channel (B * HW) of the one-launch forms

struct DropoutSeed { uint32_t lo, hi, step; };
__device__ __forceinline__ DropoutSeed dropout_seed(const DropoutArgs& da) {
  DropoutSeed s;
  s.lo = (uint32_t)da.state[0]; s.hi = (uint32_t)da.state[1]; s.step = (uint32_t)da.state[2];
  return s;
}
// the factor of the value at offset `off` of the (B, C, HW) tensor, in plane b * C + c
__device__ __forceinline__ float dropout_of(const DropoutArgs& da, const DropoutSeed& s, size_t off, int b, int C, int c) {
  const uint64_t e = da.channelwise ? (uint64_t)b * (uint64_t)C + (uint64_t)c : (uint64_t)off;
  return dropout_factor(e, da.thr, da.scale, da.site, s.lo, s.hi, s.step);
}
// ... in a loop over a chunk of batch items: channel dropout draws once per (b, c) plane, so the factor is generated when b changes
// (`channelwise` is a kernel argument: the branch is uniform), not once per value -- the 2-D layers hold thousands of values per plane
struct PlaneFactor { int b; float f; };
__device__ __forceinline__ float dropout_in_loop(const DropoutArgs& da, const DropoutSeed& s, PlaneFactor& pf, size_t off, int b, int C, int c) {
  if (!da.channelwise) return dropout_of(da, s, off, b, C, c);
  if (b != pf.b) { pf.b = b; pf.f = dropout_of(da, s, off, b, C, c); }
  return pf.f;
}
// (a select, not a product: a dropped value is 0 whatever y_raw held)
__device__ __forceinline__ float dropped(float v, float f) { return f != 0.f ? v * f : 0.f; }

// the mask policy of bn_passes.h: x = dropped(y_raw, factor) wherever a value of y_raw is read, dy_raw masked with the same factor
struct DropMask {
  typedef DropoutArgs Args;
  const DropoutArgs& da;
  const DropoutSeed sd;
  PlaneFactor pf = {-1, 0.f};      // the factor of the last (b, c) plane drawn: kept across a kernel's loops, redrawn when b changes
  __device__ __forceinline__ explicit DropMask(const DropoutArgs& a) : da(a), sd(dropout_seed(a)) {}
  __device__ __forceinline__ float factor(size_t off, int b, int C, int c) { return dropout_in_loop(da, sd, pf, off, b, C, c); }     // in a loop over b
  __device__ __forceinline__ float factor_at(size_t off, int b, int C, int c) const { return dropout_of(da, sd, off, b, C, c); }   // anywhere
  __device__ static __forceinline__ float apply(float v, float f) { return dropped(v, f); }
};

// ----------------------------------------------------------------------------------------------
// forward, one launch: channels of at most 256 * NE values
template <int NE, bool FZ>
__global__ __launch_bounds__(256) void dropout_bn_fwd_fused_kernel(const float* __restrict__ y_raw, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float* rm, float* rv,
                                                                   float* __restrict__ y, float* __restrict__ save, int B, int C, int HW,
                                                                   float slope, float eps, float momentum, const DropoutArgs da) {
  prefetch_kernargs<128>();
  const FastDiv fdHW(HW, B * HW);
  __shared__ float red[4];
  const int c = blockIdx.x, t = threadIdx.x, N = B * HW;
  const DropMask mask(da);
  float v[NE];
  size_t off[NE];
  // every load is issued before the first one is consumed (clamped indices instead of branches), the generator runs behind them
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = min(t + i * 256, N - 1);
    const int b = fdHW.div(e), pix = e - b * HW;
    off[i] = ((size_t)b * C + c) * HW + pix;
    v[i] = y_raw[off[i]];
  }
  float s1 = 0.f;
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = min(t + i * 256, N - 1);
    const float f = mask.factor_at(off[i], fdHW.div(e), C, c);
    v[i] = t + i * 256 < N ? DropMask::apply(v[i], f) : 0.f;
    s1 += v[i];
  }
  BNChannel bn;
  if (FZ) {
    bn = frozen_bn(gamma, beta, rm, rv, eps, c);
    if (t == 0) bn_save_store(save, C, c, bn);
  } else {
    const BNMoments<float> m = bn_reg_moments(v, s1, N, red);
    const float var = bn_var(m, N);
    bn = bn_channel(m, var, gamma, beta, c, eps);
    if (t == 0) {
      bn_save_store(save, C, c, bn);
      const float unbiased = bn_unbiased_var(m, N, var);
      running_stats_update(&rm[c], &rv[c], rm[c], rv[c], momentum, bn.mean, unbiased);
    }
  }
#pragma unroll
  for (int i = 0; i < NE; ++i)
    if (t + i * 256 < N) y[off[i]] = lrelu(fmaf(v[i], bn.sc, bn.sh), slope);
}

// ----------------------------------------------------------------------------------------------
// forward, two passes.  grid (C, nchunk); chunk = contiguous range of b_per_chunk batch items.
// pass 1: bn_stats_kernel<DropMask>.  pass 2: every workgroup combines the chunk partials of its channel itself (bn_combine_tiles: the
// statistics of bn_finalize_kernel); chunk 0 records `save` and moves the running statistics; all normalise their chunk.  It is not
// bn_finalize_apply_kernel with a mask: that one prefetches FA_PRE vectors of up to 16 bytes per thread, which the generator sits behind.
// FZ: no pass 1, scale / shift from the running statistics.
template <bool FZ>
__global__ __launch_bounds__(256) void dropout_bn_apply_kernel(const float* __restrict__ y_raw, const float* __restrict__ stats,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float* rm,
                                                               float* rv, float* __restrict__ y, float* __restrict__ save, int B, int C,
                                                               int HW, int b_per_chunk, float slope, float eps, float momentum,
                                                               const DropoutArgs da) {
  prefetch_kernargs<128>();
  __shared__ double red[4];
  const int c = blockIdx.x, ch = blockIdx.y, t = threadIdx.x, nchunk = gridDim.y;
  const int N = B * HW;
  BNChannel bn;
  if (FZ) {
    bn = frozen_bn(gamma, beta, rm, rv, eps, c);
    if (t == 0 && ch == 0) bn_save_store(save, C, c, bn);
  } else {
    const BNMoments<double> m = bn_combine_tiles(stats, nullptr, nchunk, b_per_chunk * HW, N, C, c, red);
    const float var = bn_var(m, N);
    bn = bn_channel(m, var, gamma, beta, c, eps);
    if (t == 0 && ch == 0) {
      bn_save_store(save, C, c, bn);
      const float unbiased = bn_unbiased_var(m, N, var);
      running_stats_update(&rm[c], &rv[c], rm[c], rv[c], momentum, bn.mean, unbiased);
    }
  }
  const int b0 = ch * b_per_chunk, nb = min(b_per_chunk, B - b0);
  const int n = nb * HW;
  DropMask mask(da);
  for (int e = t; e < n; e += 256) {
    const int b = b0 + e / HW, pix = e % HW;
    const size_t off = ((size_t)b * C + c) * HW + pix;
    const float x = DropMask::apply(y_raw[off], mask.factor(off, b, C, c));
    y[off] = lrelu(fmaf(x, bn.sc, bn.sh), slope);
  }
}

// ----------------------------------------------------------------------------------------------
// backward, one launch: channels of at most 256 * NE values (the element functions of bn_bwd_fused_kernel on the dropped values; the
// bias gradient is left to the bare conv's backward, which sums dy_raw).  A kernel of its own, not bn_bwd_fused_kernel<NE, FZ, Mask>:
// that one carries the inversion from the block's output y, the statistics groups and dbias, which a dropout block never has, and this
// one the double path below; one kernel with all of it would be harder to read than the two.
// The smallest instance (NE = 4, at most 1024 values per channel) takes the batch statistics again from the values in its registers
// and carries them, x_hat and the two sums in double: with few values per channel dy_raw is what is left after two projections that
// nearly cancel -- with TWO values x_hat is +-(1 - eps / 2 var) and dy_raw = gamma invstd (dz1 - dz2) / 2 * eps / (var + eps), a
// quantity of which an fp32 x_hat keeps two digits -- and the data and weight gradients of such a block are nothing but that.
// A few dozen double operations per thread; the activation mask still comes from the fp32 x * scale + shift of the forward pass.
template <int NE, bool FZ>
__global__ __launch_bounds__(256) void dropout_bn_bwd_fused_kernel(const float* __restrict__ dy, const float* __restrict__ y_raw,
                                                                   const float* __restrict__ save, const float* __restrict__ gamma,
                                                                   float* __restrict__ dyr, float* dgamma, float* dbeta, int B, int C,
                                                                   int HW, float slope, float eps, const DropoutArgs da) {
  prefetch_kernargs<128>();
  const FastDiv fdHW(HW, B * HW);
  __shared__ float red[4];
  __shared__ double redd[4];
  const int c = blockIdx.x, t = threadIdx.x, n = B * HW;
  const DropMask mask(da);
  const BNChannel bn = bn_save_load(save, C, c);
  const float gm = gamma[c];
  float ry[NE], rg[NE], fm[NE];
  size_t ofs[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = min(t + i * 256, n - 1);
    const int b = fdHW.div(e), pix = e - b * HW;
    ofs[i] = ((size_t)b * C + c) * HW + pix;
    ry[i] = y_raw[ofs[i]];
    rg[i] = dy[ofs[i]];
  }
  float dz[NE], xh[NE];
  float s1 = 0.f, s2 = 0.f;
  if constexpr (NE == 4 && !FZ) {
    double xs = 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const bool ok = t + i * 256 < n;
      const int e = min(t + i * 256, n - 1);
      fm[i] = mask.factor_at(ofs[i], fdHW.div(e), C, c);
      ry[i] = ok ? DropMask::apply(ry[i], fm[i]) : 0.f;                  // (x from here on)
      dz[i] = ok ? bn_dz(rg[i], bn_act_pos(ry[i], bn), slope) : 0.f;
      xs += (double)ry[i];
    }
    const double mean_d = block_sum_256(xs, redd) / (double)n;
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const double d = (double)ry[i] - mean_d;
      q += (t + i * 256 < n) ? d * d : 0.0;
    }
    const double invstd_d = 1.0 / sqrt(block_sum_256(q, redd) / (double)n + (double)eps);
    double xhd[NE], d1 = 0.0, d2 = 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      xhd[i] = (t + i * 256 < n) ? ((double)ry[i] - mean_d) * invstd_d : 0.0;
      d1 += (double)dz[i];
      d2 += (double)dz[i] * xhd[i];
    }
    d1 = block_sum_256(d1, redd);
    d2 = block_sum_256(d2, redd);
    const double gid = (double)gm * invstd_d, m1d = d1 / (double)n, m2d = d2 / (double)n;
#pragma unroll
    for (int i = 0; i < NE; ++i)
      if (t + i * 256 < n) dyr[ofs[i]] = DropMask::apply((float)(gid * ((double)dz[i] - m1d - xhd[i] * m2d)), fm[i]);
    if (t == 0 && dgamma) { dgamma[c] = (float)d2; dbeta[c] = (float)d1; }
    return;
  }
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const bool ok = t + i * 256 < n;
    const int e = min(t + i * 256, n - 1);
    fm[i] = mask.factor_at(ofs[i], fdHW.div(e), C, c);
    const BNBwdElem<float> el = bn_bwd_elem(DropMask::apply(ry[i], fm[i]), rg[i], bn, slope);
    dz[i] = ok ? el.dz : 0.f;
    xh[i] = ok ? el.xh : 0.f;
    s1 += dz[i];
    s2 += dz[i] * xh[i];
  }
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  const float invN = 1.0f / (float)n;
  const float gi = gm * bn.invstd, m1 = s1 * invN, m2 = s2 * invN;
#pragma unroll
  for (int i = 0; i < NE; ++i)
    if (t + i * 256 < n) dyr[ofs[i]] = DropMask::apply(bn_bwd_out<FZ>(gi, dz[i], m1, xh[i], m2), fm[i]);
  if (t == 0 && dgamma) { dgamma[c] = s2; dbeta[c] = s1; }
}

// backward, two passes: bn_bwd_reduce_kernel<DropMask, float> and bn_bwd_apply_kernel<FZ, DropMask, false> of bn_passes.h

// ----------------------------------------------------------------------------------------------
// the step word moves once per training step (one thread: the first launch of the step, eager or captured)
__global__ void dropout_advance_kernel(int32_t* state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) state[2] = (int32_t)((uint32_t)state[2] + 1u);
}

// out[i] = factor of mask index i / inner (inner = 1: element dropout; inner = HW: channel dropout, n = B * C * HW)
__global__ __launch_bounds__(256) void dropout_mask_kernel(float* __restrict__ out, size_t n, int inner, const DropoutArgs da) {
  const DropoutSeed sd = dropout_seed(da);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    out[i] = dropout_factor((uint64_t)(i / (size_t)inner), da.thr, da.scale, da.site, sd.lo, sd.hi, sd.step);
}

static int dropout_args(const char* who, double p, uint32_t site, const int32_t* state, int channelwise, DropoutArgs* da) {
  if (!state) return set_error("%s: the dropout state (4 device words: seed lo, seed hi, step, 0) is NULL", who);
  if (!(p >= 0.0 && p < 1.0)) return set_error("%s: p = %g is outside [0, 1)", who, p);
  da->state = state;
  da->thr = dropout_threshold(p);
  da->scale = (float)(1.0 / (1.0 - p));
  da->site = site;
  da->channelwise = channelwise ? 1 : 0;
  return 0;
}

static int dropout_shape(const char* who, int B, int C, int HW) {
  if (B < 1 || C < 1 || HW < 1) return set_error("%s: B=%d C=%d HW=%d", who, B, C, HW);
  if ((long long)B * HW > 0x7fffffffLL || (unsigned long long)B * C * HW > (1ull << 34))
    return set_error("%s: B=%d C=%d HW=%d is beyond the mask's index range (2^34 values, 2^31 per channel)", who, B, C, HW);
  return 0;
}

}  // namespace ms

using namespace ms;

extern "C" {

size_t ms_dropout_bn_workspace(int B, int C, int HW) {
  if (B < 1 || C < 1 || HW < 1 || (long long)B * HW <= DROPOUT_FUSED_MAX) return 0;
  int bpc;
  return (size_t)bwd_chunks(B, C, &bpc) * C * 2 * sizeof(float);       // forward: chunk statistics; backward: chunk sums
}

int ms_dropout_bn_fwd(const float* y_raw, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y,
                      float* save, int B, int C, int HW, float slope, float eps, float momentum, int frozen, int channelwise, double p,
                      uint32_t site, const int32_t* state, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  DropoutArgs da;
  int rc = dropout_args("ms_dropout_bn_fwd", p, site, state, channelwise, &da);
  if (rc) return rc;
  if ((rc = dropout_shape("ms_dropout_bn_fwd", B, C, HW))) return rc;
  if (!y_raw || !gamma || !beta || !running_mean || !running_var || !y || !save) return set_error("ms_dropout_bn_fwd: a NULL tensor");
  const size_t need = ms_dropout_bn_workspace(B, C, HW);
  if (need && (!workspace || workspace_bytes < need))
    return set_error("ms_dropout_bn_fwd: workspace of %zu bytes, %zu needed (ms_dropout_bn_workspace)", workspace ? workspace_bytes : (size_t)0, need);
  const long n = (long)B * HW;
  if (n <= DROPOUT_FUSED_MAX) {
    const int ne = fused_ne(n);
    // (a frozen block's forward is a bn_apply, a batch-statistics block's a bn_finalize_apply: the families of the forms without dropout)
    TimingScope ts(s, 0, 8.0 * n * C, frozen ? "bn_apply fused<%d> C%d HW%d B%d frozen dropout" : "bn_finalize_apply<%d> C%d HW%d B%d fused dropout",
                   ne, C, HW, B);
    if (ts.skip()) return 0;
    launch_ne_fz(ne, frozen != 0, [&](auto NE, auto FZ) {
      hipLaunchKernelGGL((dropout_bn_fwd_fused_kernel<decltype(NE)::value, decltype(FZ)::value>), dim3(C), dim3(256), 0, s, y_raw, gamma, beta,
                         running_mean, running_var, y, save, B, C, HW, slope, eps, momentum, da);
    });
    return check_launch("dropout_bn_fwd_fused_kernel");
  }
  int bpc;
  const int nchunk = bwd_chunks(B, C, &bpc);
  if (frozen) {
    TimingScope ts(s, 0, 8.0 * n * C, "bn_apply chunks%d C%d HW%d B%d frozen dropout", nchunk, C, HW, B);
    if (ts.skip()) return 0;
    hipLaunchKernelGGL(dropout_bn_apply_kernel<true>, dim3(C, nchunk), dim3(256), 0, s, y_raw, (const float*)nullptr, gamma, beta, running_mean,
                       running_var, y, save, B, C, HW, bpc, slope, eps, momentum, da);
    return check_launch("dropout_bn_apply_kernel");
  }
  TimingScope ts(s, 0, 16.0 * n * C, "bn_finalize_apply<0> C%d HW%d B%d chunks%d dropout", C, HW, B, nchunk);
  if (ts.skip()) return 0;
  hipLaunchKernelGGL(bn_stats_kernel<DropMask>, dim3(C, nchunk), dim3(256), 0, s, y_raw, (float*)workspace, B, C, HW, bpc, da);
  if ((rc = check_launch("bn_stats_kernel"))) return rc;
  hipLaunchKernelGGL(dropout_bn_apply_kernel<false>, dim3(C, nchunk), dim3(256), 0, s, y_raw, (const float*)workspace, gamma, beta, running_mean,
                     running_var, y, save, B, C, HW, bpc, slope, eps, momentum, da);
  return check_launch("dropout_bn_apply_kernel");
}

int ms_dropout_bn_bwd(const float* dy, const float* y_raw, const float* save, const float* gamma, float* dyr, float* dgamma, float* dbeta,
                      int B, int C, int HW, float slope, float eps, int frozen, int channelwise, double p, uint32_t site,
                      const int32_t* state, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  DropoutArgs da;
  int rc = dropout_args("ms_dropout_bn_bwd", p, site, state, channelwise, &da);
  if (rc) return rc;
  if ((rc = dropout_shape("ms_dropout_bn_bwd", B, C, HW))) return rc;
  if (!dy || !y_raw || !save || !gamma || !dyr) return set_error("ms_dropout_bn_bwd: a NULL tensor");
  if ((dgamma == nullptr) != (dbeta == nullptr)) return set_error("ms_dropout_bn_bwd: dgamma and dbeta come together (both or neither)");
  const size_t need = ms_dropout_bn_workspace(B, C, HW);
  if (need && (!workspace || workspace_bytes < need))
    return set_error("ms_dropout_bn_bwd: workspace of %zu bytes, %zu needed (ms_dropout_bn_workspace)", workspace ? workspace_bytes : (size_t)0, need);
  const long n = (long)B * HW;
  if (n <= DROPOUT_FUSED_MAX) {
    const int ne = fused_ne(n);
    TimingScope ts(s, 0, 12.0 * n * C, "bn_bwd_fused<%d> C%d HW%d B%d%s dropout", ne, C, HW, B, frozen ? " frozen" : "");
    if (ts.skip()) return 0;
    launch_ne_fz(ne, frozen != 0, [&](auto NE, auto FZ) {
      hipLaunchKernelGGL((dropout_bn_bwd_fused_kernel<decltype(NE)::value, decltype(FZ)::value>), dim3(C), dim3(256), 0, s, dy, y_raw, save, gamma,
                         dyr, dgamma, dbeta, B, C, HW, slope, eps, da);
    });
    return check_launch("dropout_bn_bwd_fused_kernel");
  }
  int bpc;
  const int nchunk = bwd_chunks(B, C, &bpc);
  TimingScope ts(s, 0, 20.0 * n * C, "bn_bwd(reduce+apply) C%d HW%d B%d%s dropout", C, HW, B, frozen ? " frozen" : "");
  if (ts.skip()) return 0;
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<DropMask, float>), dim3(C, nchunk), dim3(256), 0, s, dy, y_raw, save, (float*)workspace, B, C, HW, bpc, slope, da);
  if ((rc = check_launch("bn_bwd_reduce_kernel"))) return rc;
  if (frozen)
    hipLaunchKernelGGL((bn_bwd_apply_kernel<true, DropMask, false>), dim3(C, nchunk), dim3(256), 0, s, dy, y_raw, save, gamma, (const float*)workspace, dyr,
                       (float*)nullptr, dgamma, dbeta, B, C, HW, bpc, slope, da);
  else
    hipLaunchKernelGGL((bn_bwd_apply_kernel<false, DropMask, false>), dim3(C, nchunk), dim3(256), 0, s, dy, y_raw, save, gamma, (const float*)workspace, dyr,
                       (float*)nullptr, dgamma, dbeta, B, C, HW, bpc, slope, da);
  return check_launch("bn_bwd_apply_kernel");
}

int ms_dropout_advance(int32_t* state, void* stream) {
  if (!state) return set_error("ms_dropout_advance: the dropout state is NULL");
  TimingScope ts((hipStream_t)stream, 0, 16.0, "bn_finalize advance dropout");
  if (ts.skip()) return 0;
  hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
  return check_launch("dropout_advance_kernel");
}

int ms_dropout_mask(float* out, size_t n, int inner, double p, uint32_t site, const int32_t* state, void* stream) {
  DropoutArgs da;
  int rc = dropout_args("ms_dropout_mask", p, site, state, 0, &da);
  if (rc) return rc;
  if (!out || n < 1 || inner < 1 || n / (size_t)inner > ((size_t)1 << 34)) return set_error("ms_dropout_mask: out=%p n=%zu inner=%d", (void*)out, n, inner);
  TimingScope ts((hipStream_t)stream, 0, 4.0 * n, "bn_apply mask n%zu inner%d dropout", n, inner);
  if (ts.skip()) return 0;
  const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, n, inner, da);
  return check_launch("dropout_mask_kernel");
}

}  // extern "C"
