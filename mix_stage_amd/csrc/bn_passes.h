// The fp32 stand-alone BatchNorm passes' channel arithmetic, once: elementwise.hip (the passes of a block), dropout.hip (the same
// passes on the dropped values) and conv_igemm.hip (the split-K epilogues that own a channel) all compute with the functions here,
// so the statistics of the one-launch and two-launch forms, and the activation mask of forward and backward, agree bit for bit by
// construction.  Blocks of 256 threads; every reduction in a fixed order.
//   tiles / chunks:  stats[tile][C][2] = (sum, M2 about the tile's mean) -> bn_combine_tiles -> (mean, M2) in double
//   registers:       NE values per thread                                -> bn_reg_moments   -> (mean, M2) in fp32
//   channel:         (mean, M2) -> bn_var -> bn_channel -> save = mean | invstd | scale | shift (BNChannel);  bn_unbiased_var for the
//                    running statistics
//   backward:        bn_bwd_elem: (x, dy) -> (dz, x_hat);  bn_bwd_out<FZ>: dy_raw
// Mask policy: the kernels here read y_raw through a Mask.  NoMask is the plain block; dropout.hip's DropMask regenerates the
// block's dropout mask wherever a value is read (x = m * y_raw) and masks dy_raw again.
#pragma once
#include "common.h"

namespace ms {

// the four-word record of `save`: BNChannel (common.h)
__device__ __forceinline__ void bn_save_store(float* save, int C, int c, const BNChannel& ch) {
  save[c] = ch.mean;
  save[C + c] = ch.invstd;
  save[2 * C + c] = ch.sc;
  save[3 * C + c] = ch.sh;
}
__device__ __forceinline__ BNChannel bn_save_load(const float* save, int C, int c) {
  return {save[c], save[C + c], save[2 * C + c], save[3 * C + c]};
}

template <typename T> struct BNMoments { T mean, m2; };
// (mean, M2) of N values -> the biased variance, the channel's record, and the variance the running statistics take.
// T = double: the finalize family (tile partials); T = float: the kernels that hold a channel in registers or re-read it.
template <typename T>
__device__ __forceinline__ float bn_var(const BNMoments<T>& m, int N) { return (float)(m.m2 / (T)N); }
// (gamma[c], beta[c] are read here, behind the square root, where every kernel has always read them: the kernels' code stays as it was)
template <typename T>
__device__ __forceinline__ BNChannel bn_channel(const BNMoments<T>& m, float var, const float* gamma, const float* beta, int c, float eps) {
  BNChannel ch;
  ch.invstd = 1.0f / sqrtf(var + eps);
  ch.mean = (float)m.mean;
  ch.sc = gamma[c] * ch.invstd;
  ch.sh = beta[c] - ch.mean * ch.sc;
  return ch;
}
// ... for a kernel that holds the channel's two parameters in registers
template <typename T>
__device__ __forceinline__ BNChannel bn_channel(const BNMoments<T>& m, float var, float gamma_c, float beta_c, float eps) {
  return bn_channel(m, var, &gamma_c, &beta_c, 0, eps);
}
template <typename T>
__device__ __forceinline__ float bn_unbiased_var(const BNMoments<T>& m, int N, float var) {
  return N > 1 ? (float)(m.m2 / (T)(N - 1)) : var;
}

// ---- tile partials -> (mean, M2) in double
// a tile's term of M2 about the global mean; st = the tile's (sum, M2 about its own mean) of cnt values
__device__ __forceinline__ double bn_tile_m2(float2 st, int cnt, double mean) {
  const double d = (double)st.x / (double)cnt - mean;
  return (double)st.y + (double)cnt * d * d;
}
// the finalize family's block sum, left to right; the caller separates two uses of `red` (4 doubles of LDS) with a barrier
__device__ __forceinline__ double bn_finalize_sum(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
// thread t takes tiles t, t + 256, ...; tile i holds counts[i] values, or min(tile_n, N - i * tile_n) where counts == NULL
__device__ __forceinline__ BNMoments<double> bn_combine_tiles(const float* __restrict__ stats, const float* __restrict__ counts, int n_tiles,
                                                              int tile_n, int N, int C, int c, double* red) {
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n_tiles; i += 256) s += (double)stats[((size_t)i * C + c) * 2];
  const double mean = bn_finalize_sum(s, red) / (double)N;
  __syncthreads();
  double q = 0.0;
  for (int i = t; i < n_tiles; i += 256) {
    const float* st = stats + ((size_t)i * C + c) * 2;
    const int cnt = counts ? (int)counts[i] : min(tile_n, N - i * tile_n);
    q += bn_tile_m2(float2{st[0], st[1]}, cnt, mean);
  }
  return {mean, bn_finalize_sum(q, red)};
}

// ---- NE values per thread (value i of thread t is element t + 256 * i; entries past N hold 0) -> two-pass (mean, M2) in fp32
template <int NE>
__device__ __forceinline__ BNMoments<float> bn_reg_moments(const float (&v)[NE], float thread_sum, int N, float* red) {
  const int t = threadIdx.x;
  const float mean = block_sum_256(thread_sum, red) / (float)N;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const float d = v[i] - mean;
    q += (t + i * 256 < N) ? d * d : 0.f;
  }
  return {mean, block_sum_256(q, red)};
}

// ---- backward element math.  The activation mask comes from the fp32 z = fma(x, scale, shift), bit-identical to the forward pass,
// whatever Acc carries dz and x_hat.
__device__ __forceinline__ bool bn_act_pos(float x, const BNChannel& ch) { return fmaf(x, ch.sc, ch.sh) > 0.f; }
template <typename Acc = float>
__device__ __forceinline__ Acc bn_dz(float dy, bool pos, float slope) { return (Acc)dy * (pos ? (Acc)1 : (Acc)slope); }
template <typename Acc = float>
__device__ __forceinline__ Acc bn_xhat(float x, const BNChannel& ch) { return ((Acc)x - (Acc)ch.mean) * (Acc)ch.invstd; }
template <typename Acc> struct BNBwdElem { Acc dz, xh; };
template <typename Acc = float>
__device__ __forceinline__ BNBwdElem<Acc> bn_bwd_elem(float x, float dy, const BNChannel& ch, float slope) {
  return {bn_dz<Acc>(dy, bn_act_pos(x, ch), slope), bn_xhat<Acc>(x, ch)};
}
// dy_raw from gi = gamma * invstd and the channel means m1 = mean(dz), m2 = mean(dz * x_hat).  FZ (frozen BatchNorm: the statistics
// do not depend on the batch): without the two mean terms, which are the derivative of the batch statistics.
template <bool FZ>
__device__ __forceinline__ float bn_bwd_out(float gi, float dz, float m1, float xh, float m2) {
  return FZ ? gi * dz : gi * (dz - m1 - xh * m2);
}

// ---- the mask policy of a plain block: every factor is the constant 1
struct NoMask {
  struct Args {};
  __device__ __forceinline__ explicit NoMask(const Args&) {}
  __device__ __forceinline__ float factor(size_t, int, int, int) { return 1.f; }      // of the value at `off`, plane (b, c), in a loop over b
  __device__ static __forceinline__ float apply(float v, float) { return v; }
};

// ----------------------------------------------------------------------------------------------
// The chunked two-pass kernels.  grid (C, nchunk); chunk = contiguous range of b_per_chunk batch items.

// stats[chunk][C][2] = (sum, M2 about the chunk's mean) of x -- the per-tile format bn_combine_tiles takes
template <class Mask>
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ y_raw, float* __restrict__ stats, int B, int C, int HW,
                                                       int b_per_chunk, const typename Mask::Args ma) {
  prefetch_kernargs<128>();
  __shared__ float red[4];
  const int c = blockIdx.x, ch = blockIdx.y, t = threadIdx.x;
  const int b0 = ch * b_per_chunk, nb = min(b_per_chunk, B - b0);
  const int n = nb * HW;
  Mask mask(ma);
  auto x_at = [&](int e) {
    const int b = b0 + e / HW, pix = e % HW;
    const size_t off = ((size_t)b * C + c) * HW + pix;
    return Mask::apply(y_raw[off], mask.factor(off, b, C, c));
  };
  float s = 0.f;
  for (int e = t; e < n; e += 256) s += x_at(e);
  s = block_sum_256(s, red);
  const float mean = s / (float)n;
  float q = 0.f;
  for (int e = t; e < n; e += 256) {
    const float d = x_at(e) - mean;
    q += d * d;
  }
  q = block_sum_256(q, red);
  if (t == 0) {
    stats[((size_t)ch * C + c) * 2] = s;
    stats[((size_t)ch * C + c) * 2 + 1] = q;
  }
}

// BatchNorm + LeakyReLU backward, pass 1: partial[c][chunk] = (sum dz, sum dz * x_hat).
// Acc = double (the stand-alone sums of the cross-rank BatchNorm, ms_bn_bwd_sums): the terms and every partial sum in double.  sum dz *
// x_hat cancels (about sqrt(n) of n terms of size 1 remain): with fp32 terms and fp32 partials a single channel of 2047 values came
// out 9e-7 off, more than four times what an fp32 evaluation on the host loses.
template <class Mask, typename Acc>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ y_raw,
                                                            const float* __restrict__ save, Acc* __restrict__ partial, int B, int C, int HW,
                                                            int b_per_chunk, float slope, const typename Mask::Args ma) {
  prefetch_kernargs<128>();
  __shared__ Acc red[4];
  const int c = blockIdx.x, ch = blockIdx.y, t = threadIdx.x;
  const int b0 = ch * b_per_chunk, nb = min(b_per_chunk, B - b0);
  const BNChannel bn = bn_save_load(save, C, c);
  Mask mask(ma);
  Acc s1 = 0, s2 = 0;
  const int n = nb * HW;
  for (int e = t; e < n; e += 256) {
    const int b = b0 + e / HW, pix = e % HW;
    const size_t off = ((size_t)b * C + c) * HW + pix;
    const float x = Mask::apply(y_raw[off], mask.factor(off, b, C, c));
    const BNBwdElem<Acc> el = bn_bwd_elem<Acc>(x, dy[off], bn, slope);
    s1 += el.dz;
    s2 += el.dz * el.xh;
  }
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  if (t == 0) {
    partial[((size_t)c * gridDim.y + ch) * 2] = s1;
    partial[((size_t)c * gridDim.y + ch) * 2 + 1] = s2;
  }
}

// pass 2: dy_raw = m * bn_bwd_out(...) with the chunk partials summed in chunk order; dgamma = sum dz * x_hat, dbeta = sum dz.
// COLSUM: colpart[c][chunk] = the chunk's sum of dy_raw (the bias gradient's partials).
template <bool FZ, class Mask, bool COLSUM>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y_raw,
                                                           const float* __restrict__ save, const float* __restrict__ gamma,
                                                           const float* __restrict__ partial, float* __restrict__ dyr,
                                                           float* __restrict__ colpart, float* dgamma, float* dbeta, int B, int C, int HW,
                                                           int b_per_chunk, float slope, const typename Mask::Args ma) {
  prefetch_kernargs<128>();
  __shared__ float red[4];
  const int c = blockIdx.x, ch = blockIdx.y, t = threadIdx.x, nchunk = gridDim.y;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < nchunk; ++k) {
    s1 += partial[((size_t)c * nchunk + k) * 2];
    s2 += partial[((size_t)c * nchunk + k) * 2 + 1];
  }
  const float invN = 1.0f / (float)((size_t)B * HW);
  const BNChannel bn = bn_save_load(save, C, c);
  const float gi = gamma[c] * bn.invstd, m1 = s1 * invN, m2 = s2 * invN;
  const int b0 = ch * b_per_chunk, nb = min(b_per_chunk, B - b0);
  const int n = nb * HW;
  Mask mask(ma);
  float cs = 0.f;
  for (int e = t; e < n; e += 256) {
    const int b = b0 + e / HW, pix = e % HW;
    const size_t off = ((size_t)b * C + c) * HW + pix;
    const float f = mask.factor(off, b, C, c);
    const BNBwdElem<float> el = bn_bwd_elem(Mask::apply(y_raw[off], f), dy[off], bn, slope);
    const float v = Mask::apply(bn_bwd_out<FZ>(gi, el.dz, m1, el.xh, m2), f);
    dyr[off] = v;
    cs += v;
  }
  if (COLSUM) cs = block_sum_256(cs, red);
  if (t == 0) {
    if (COLSUM) colpart[(size_t)c * nchunk + ch] = cs;
    if (ch == 0 && dgamma) { dgamma[c] = s2; dbeta[c] = s1; }
  }
}

}  // namespace ms
