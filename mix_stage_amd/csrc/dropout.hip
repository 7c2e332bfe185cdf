// Dropout inside the ConvNormRelu block (layers.py:32-78 with p > 0): conv (+bias) -> dropout(p) -> BatchNorm -> (Leaky)ReLU.
// The conv runs as the block's MS_BARE launch and leaves y_raw UNDROPPED; the kernels here are the BatchNorm passes of the block
// with the mask regenerated wherever a value of y_raw is read (dropout_mask.h: a counter-based generator, no mask tensor in
// memory): the batch statistics are those of the dropped values x = m * y_raw, m = 0 or 1 / (1 - p).
//   forward   x -> (sum, M2) -> save = mean | invstd | scale | shift, running statistics -> y = lrelu(x * scale + shift)
//   backward  dz = dy * lrelu'(x * scale + shift), x_hat = (x - mean) * invstd,
//             dy_raw = m * gamma * invstd * (dz - mean(dz) - x_hat * mean(dz * x_hat));  dgamma = sum dz * x_hat, dbeta = sum dz
// FZ (frozen BatchNorm, layers.freeze_batchnorm): scale / shift come from the running statistics, which are only read, and the
// backward drops the two batch-mean terms, as the FZ kernels of elementwise.hip do.
// One workgroup owns a channel of at most 256 * 16 values and keeps them in registers (the forms of splitk_fwd_epilogue_kernel<NE>
// and bn_bwd_fused_kernel<NE>); larger channels take two passes over chunks of batch items.  No workgroup waits for another; every
// reduction runs in a fixed order (no float atomics): the same bits run to run, captured or eager.
#include <algorithm>

#include <stdint.h>

#include "kernels.h"
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

// block-wide sum in double for 256-thread blocks, in a fixed order; result valid in every thread.  `red` = 4 doubles of LDS.
__device__ inline double block_sum_256_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

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
  const DropoutSeed sd = dropout_seed(da);
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
    const float f = dropout_of(da, sd, off[i], fdHW.div(e), C, c);
    v[i] = t + i * 256 < N ? dropped(v[i], f) : 0.f;
    s1 += v[i];
  }
  float mean, invstd, sc, sh;
  if (FZ) {
    const FrozenBN f = frozen_bn(gamma, beta, rm, rv, eps, c);
    mean = f.mean; invstd = f.invstd; sc = f.sc; sh = f.sh;
    if (t == 0) { save[c] = mean; save[C + c] = invstd; save[2 * C + c] = sc; save[3 * C + c] = sh; }
  } else {
    // (sum, M2 about the mean) in the order of splitk_fwd_epilogue_kernel
    mean = block_sum_256(s1, red) / (float)N;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const float d = v[i] - mean;
      q += (t + i * 256 < N) ? d * d : 0.f;
    }
    const float m2 = block_sum_256(q, red);
    const float var = m2 / (float)N;
    invstd = 1.0f / sqrtf(var + eps);
    sc = gamma[c] * invstd;
    sh = beta[c] - mean * sc;
    if (t == 0) {
      save[c] = mean; save[C + c] = invstd; save[2 * C + c] = sc; save[3 * C + c] = sh;
      const float unbiased = N > 1 ? m2 / (float)(N - 1) : var;
      running_stats_update(&rm[c], &rv[c], rm[c], rv[c], momentum, mean, unbiased);
    }
  }
#pragma unroll
  for (int i = 0; i < NE; ++i)
    if (t + i * 256 < N) y[off[i]] = lrelu(fmaf(v[i], sc, sh), slope);
}

// ----------------------------------------------------------------------------------------------
// forward, two passes.  grid (C, nchunk); chunk = contiguous range of b_per_chunk batch items.
// pass 1: stats[chunk][C][2] = (sum, M2 about the chunk's mean) of the dropped values -- the per-tile format bn_finalize_kernel combines
__global__ __launch_bounds__(256) void dropout_bn_stats_kernel(const float* __restrict__ y_raw, float* __restrict__ stats, int B, int C,
                                                               int HW, int b_per_chunk, const DropoutArgs da) {
  prefetch_kernargs<128>();
  __shared__ float red[4];
  const int c = blockIdx.x, ch = blockIdx.y, t = threadIdx.x;
  const int b0 = ch * b_per_chunk, nb = min(b_per_chunk, B - b0);
  const int n = nb * HW;
  const DropoutSeed sd = dropout_seed(da);
  float s = 0.f;
  PlaneFactor pf = {-1, 0.f};
  for (int e = t; e < n; e += 256) {
    const int b = b0 + e / HW, pix = e % HW;
    const size_t off = ((size_t)b * C + c) * HW + pix;
    s += dropped(y_raw[off], dropout_in_loop(da, sd, pf, off, b, C, c));
  }
  s = block_sum_256(s, red);
  const float mean = s / (float)n;
  float q = 0.f;
  for (int e = t; e < n; e += 256) {
    const int b = b0 + e / HW, pix = e % HW;
    const size_t off = ((size_t)b * C + c) * HW + pix;
    const float d = dropped(y_raw[off], dropout_in_loop(da, sd, pf, off, b, C, c)) - mean;
    q += d * d;
  }
  q = block_sum_256(q, red);
  if (t == 0) {
    stats[((size_t)ch * C + c) * 2] = s;
    stats[((size_t)ch * C + c) * 2 + 1] = q;
  }
}

// pass 2: every workgroup combines the chunk partials of its channel itself, with the operations of bn_finalize_kernel in its order
// (thread t takes chunks t, t + 256, ...); chunk 0 records `save` and moves the running statistics; all normalise their chunk.
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
  float fmean, invstd, sc, sh;
  if (FZ) {
    const FrozenBN f = frozen_bn(gamma, beta, rm, rv, eps, c);
    fmean = f.mean; invstd = f.invstd; sc = f.sc; sh = f.sh;
    if (t == 0 && ch == 0) { save[c] = fmean; save[C + c] = invstd; save[2 * C + c] = sc; save[3 * C + c] = sh; }
  } else {
    const int tile_n = b_per_chunk * HW;
    double s = 0.0;
    for (int i = t; i < nchunk; i += 256) s += (double)stats[((size_t)i * C + c) * 2];
    s = wave_sum_d(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    const double mean = (red[0] + red[1] + red[2] + red[3]) / (double)N;
    __syncthreads();
    double q = 0.0;
    for (int i = t; i < nchunk; i += 256) {
      const float* st = stats + ((size_t)i * C + c) * 2;
      const int cnt = min(tile_n, N - i * tile_n);
      const double d = (double)st[0] / (double)cnt - mean;
      q += (double)st[1] + (double)cnt * d * d;
    }
    q = wave_sum_d(q);
    if ((t & 63) == 0) red[t >> 6] = q;
    __syncthreads();
    const double m2 = red[0] + red[1] + red[2] + red[3];
    const float var = (float)(m2 / (double)N);
    invstd = 1.0f / sqrtf(var + eps);
    fmean = (float)mean;
    sc = gamma[c] * invstd;
    sh = beta[c] - fmean * sc;
    if (t == 0 && ch == 0) {
      save[c] = fmean; save[C + c] = invstd; save[2 * C + c] = sc; save[3 * C + c] = sh;
      const float unbiased = N > 1 ? (float)(m2 / (double)(N - 1)) : var;
      running_stats_update(&rm[c], &rv[c], rm[c], rv[c], momentum, fmean, unbiased);
    }
  }
  const int b0 = ch * b_per_chunk, nb = min(b_per_chunk, B - b0);
  const int n = nb * HW;
  const DropoutSeed sd = dropout_seed(da);
  PlaneFactor pf = {-1, 0.f};
  for (int e = t; e < n; e += 256) {
    const int b = b0 + e / HW, pix = e % HW;
    const size_t off = ((size_t)b * C + c) * HW + pix;
    const float x = dropped(y_raw[off], dropout_in_loop(da, sd, pf, off, b, C, c));
    y[off] = lrelu(fmaf(x, sc, sh), slope);
  }
}

// ----------------------------------------------------------------------------------------------
// backward, one launch: channels of at most 256 * NE values (bn_bwd_fused_kernel on the dropped values; the bias gradient is left
// to the bare conv's backward, which sums dy_raw)
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
  const DropoutSeed sd = dropout_seed(da);
  const float mean = save[c], invstd = save[C + c], sc = save[2 * C + c], sh = save[3 * C + c], gm = gamma[c];
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
      fm[i] = dropout_of(da, sd, ofs[i], fdHW.div(e), C, c);
      ry[i] = ok ? dropped(ry[i], fm[i]) : 0.f;                  // (x from here on)
      dz[i] = ok ? rg[i] * (fmaf(ry[i], sc, sh) > 0.f ? 1.f : slope) : 0.f;
      xs += (double)ry[i];
    }
    const double mean_d = block_sum_256_d(xs, redd) / (double)n;
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const double d = (double)ry[i] - mean_d;
      q += (t + i * 256 < n) ? d * d : 0.0;
    }
    const double invstd_d = 1.0 / sqrt(block_sum_256_d(q, redd) / (double)n + (double)eps);
    double xhd[NE], d1 = 0.0, d2 = 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      xhd[i] = (t + i * 256 < n) ? ((double)ry[i] - mean_d) * invstd_d : 0.0;
      d1 += (double)dz[i];
      d2 += (double)dz[i] * xhd[i];
    }
    d1 = block_sum_256_d(d1, redd);
    d2 = block_sum_256_d(d2, redd);
    const double gid = (double)gm * invstd_d, m1d = d1 / (double)n, m2d = d2 / (double)n;
#pragma unroll
    for (int i = 0; i < NE; ++i)
      if (t + i * 256 < n) dyr[ofs[i]] = dropped((float)(gid * ((double)dz[i] - m1d - xhd[i] * m2d)), fm[i]);
    if (t == 0 && dgamma) { dgamma[c] = (float)d2; dbeta[c] = (float)d1; }
    return;
  }
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const bool ok = t + i * 256 < n;
    const int e = min(t + i * 256, n - 1);
    fm[i] = dropout_of(da, sd, ofs[i], fdHW.div(e), C, c);
    const float x = dropped(ry[i], fm[i]);
    const bool pos = fmaf(x, sc, sh) > 0.f;                 // (bit-identical to the forward pass)
    dz[i] = ok ? rg[i] * (pos ? 1.f : slope) : 0.f;
    xh[i] = ok ? (x - mean) * invstd : 0.f;
    s1 += dz[i];
    s2 += dz[i] * xh[i];
  }
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  const float invN = 1.0f / (float)n;
  const float gi = gm * invstd, m1 = s1 * invN, m2 = s2 * invN;
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    if (t + i * 256 < n) {
      const float v = FZ ? gi * dz[i] : gi * (dz[i] - m1 - xh[i] * m2);
      dyr[ofs[i]] = dropped(v, fm[i]);
    }
  }
  if (t == 0 && dgamma) { dgamma[c] = s2; dbeta[c] = s1; }
}

// backward, two passes (bn_bwd_reduce_kernel / bn_bwd_apply_kernel on the dropped values): partial[c][chunk] = (sum dz, sum dz * x_hat)
__global__ __launch_bounds__(256) void dropout_bn_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ y_raw,
                                                                    const float* __restrict__ save, float* __restrict__ partial, int B,
                                                                    int C, int HW, int b_per_chunk, float slope, const DropoutArgs da) {
  prefetch_kernargs<128>();
  __shared__ float red[4];
  const int c = blockIdx.x, ch = blockIdx.y, t = threadIdx.x;
  const int b0 = ch * b_per_chunk, nb = min(b_per_chunk, B - b0);
  const float mean = save[c], invstd = save[C + c], sc = save[2 * C + c], sh = save[3 * C + c];
  const DropoutSeed sd = dropout_seed(da);
  float s1 = 0.f, s2 = 0.f;
  const int n = nb * HW;
  PlaneFactor pf = {-1, 0.f};
  for (int e = t; e < n; e += 256) {
    const int b = b0 + e / HW, pix = e % HW;
    const size_t off = ((size_t)b * C + c) * HW + pix;
    const float x = dropped(y_raw[off], dropout_in_loop(da, sd, pf, off, b, C, c));
    const float dz = dy[off] * (fmaf(x, sc, sh) > 0.f ? 1.f : slope);
    s1 += dz;
    s2 += dz * ((x - mean) * invstd);
  }
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  if (t == 0) {
    partial[((size_t)c * gridDim.y + ch) * 2] = s1;
    partial[((size_t)c * gridDim.y + ch) * 2 + 1] = s2;
  }
}

template <bool FZ>
__global__ __launch_bounds__(256) void dropout_bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y_raw,
                                                                   const float* __restrict__ save, const float* __restrict__ gamma,
                                                                   const float* __restrict__ partial, float* __restrict__ dyr,
                                                                   float* dgamma, float* dbeta, int B, int C, int HW, int b_per_chunk,
                                                                   float slope, const DropoutArgs da) {
  prefetch_kernargs<128>();
  const int c = blockIdx.x, ch = blockIdx.y, t = threadIdx.x, nchunk = gridDim.y;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < nchunk; ++k) {
    s1 += partial[((size_t)c * nchunk + k) * 2];
    s2 += partial[((size_t)c * nchunk + k) * 2 + 1];
  }
  const float invN = 1.0f / (float)((size_t)B * HW);
  const float mean = save[c], invstd = save[C + c], sc = save[2 * C + c], sh = save[3 * C + c];
  const float gi = gamma[c] * invstd, m1 = s1 * invN, m2 = s2 * invN;
  const int b0 = ch * b_per_chunk, nb = min(b_per_chunk, B - b0);
  const int n = nb * HW;
  const DropoutSeed sd = dropout_seed(da);
  PlaneFactor pf = {-1, 0.f};
  for (int e = t; e < n; e += 256) {
    const int b = b0 + e / HW, pix = e % HW;
    const size_t off = ((size_t)b * C + c) * HW + pix;
    const float f = dropout_in_loop(da, sd, pf, off, b, C, c);
    const float x = dropped(y_raw[off], f);
    const float dz = dy[off] * (fmaf(x, sc, sh) > 0.f ? 1.f : slope);
    const float xh = (x - mean) * invstd;
    dyr[off] = dropped(FZ ? gi * dz : gi * (dz - m1 - xh * m2), f);
  }
  if (t == 0 && ch == 0 && dgamma) { dgamma[c] = s2; dbeta[c] = s1; }
}

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

#define MS_DROPOUT_FWD(N)                                                                                                        \
  do {                                                                                                                           \
    if (frozen) hipLaunchKernelGGL((dropout_bn_fwd_fused_kernel<N, true>), dim3(C), dim3(256), 0, s, y_raw, gamma, beta, running_mean, running_var, y, save, B, C, HW, slope, eps, momentum, da); \
    else hipLaunchKernelGGL((dropout_bn_fwd_fused_kernel<N, false>), dim3(C), dim3(256), 0, s, y_raw, gamma, beta, running_mean, running_var, y, save, B, C, HW, slope, eps, momentum, da);      \
  } while (0)
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
    const int ne = n <= 256 * 4 ? 4 : n <= 256 * 8 ? 8 : 16;
    // (a frozen block's forward is a bn_apply, a batch-statistics block's a bn_finalize_apply: the families of the forms without dropout)
    TimingScope ts(s, 0, 8.0 * n * C, frozen ? "bn_apply fused<%d> C%d HW%d B%d frozen dropout" : "bn_finalize_apply<%d> C%d HW%d B%d fused dropout",
                   ne, C, HW, B);
    if (ts.skip()) return 0;
    if (ne == 4) MS_DROPOUT_FWD(4);
    else if (ne == 8) MS_DROPOUT_FWD(8);
    else MS_DROPOUT_FWD(16);
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
  hipLaunchKernelGGL(dropout_bn_stats_kernel, dim3(C, nchunk), dim3(256), 0, s, y_raw, (float*)workspace, B, C, HW, bpc, da);
  if ((rc = check_launch("dropout_bn_stats_kernel"))) return rc;
  hipLaunchKernelGGL(dropout_bn_apply_kernel<false>, dim3(C, nchunk), dim3(256), 0, s, y_raw, (const float*)workspace, gamma, beta, running_mean,
                     running_var, y, save, B, C, HW, bpc, slope, eps, momentum, da);
  return check_launch("dropout_bn_apply_kernel");
}
#undef MS_DROPOUT_FWD

#define MS_DROPOUT_BWD(N)                                                                                                        \
  do {                                                                                                                           \
    if (frozen) hipLaunchKernelGGL((dropout_bn_bwd_fused_kernel<N, true>), dim3(C), dim3(256), 0, s, dy, y_raw, save, gamma, dyr, dgamma, dbeta, B, C, HW, slope, eps, da); \
    else hipLaunchKernelGGL((dropout_bn_bwd_fused_kernel<N, false>), dim3(C), dim3(256), 0, s, dy, y_raw, save, gamma, dyr, dgamma, dbeta, B, C, HW, slope, eps, da);      \
  } while (0)
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
    const int ne = n <= 256 * 4 ? 4 : n <= 256 * 8 ? 8 : 16;
    TimingScope ts(s, 0, 12.0 * n * C, "bn_bwd_fused<%d> C%d HW%d B%d%s dropout", ne, C, HW, B, frozen ? " frozen" : "");
    if (ts.skip()) return 0;
    if (ne == 4) MS_DROPOUT_BWD(4);
    else if (ne == 8) MS_DROPOUT_BWD(8);
    else MS_DROPOUT_BWD(16);
    return check_launch("dropout_bn_bwd_fused_kernel");
  }
  int bpc;
  const int nchunk = bwd_chunks(B, C, &bpc);
  TimingScope ts(s, 0, 20.0 * n * C, "bn_bwd(reduce+apply) C%d HW%d B%d%s dropout", C, HW, B, frozen ? " frozen" : "");
  if (ts.skip()) return 0;
  hipLaunchKernelGGL(dropout_bn_bwd_reduce_kernel, dim3(C, nchunk), dim3(256), 0, s, dy, y_raw, save, (float*)workspace, B, C, HW, bpc, slope, da);
  if ((rc = check_launch("dropout_bn_bwd_reduce_kernel"))) return rc;
  if (frozen)
    hipLaunchKernelGGL(dropout_bn_bwd_apply_kernel<true>, dim3(C, nchunk), dim3(256), 0, s, dy, y_raw, save, gamma, (const float*)workspace, dyr,
                       dgamma, dbeta, B, C, HW, bpc, slope, da);
  else
    hipLaunchKernelGGL(dropout_bn_bwd_apply_kernel<false>, dim3(C, nchunk), dim3(256), 0, s, dy, y_raw, save, gamma, (const float*)workspace, dyr,
                       dgamma, dbeta, B, C, HW, bpc, slope, da);
  return check_launch("dropout_bn_bwd_apply_kernel");
}
#undef MS_DROPOUT_BWD

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
