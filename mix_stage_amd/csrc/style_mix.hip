// Style mixing: the float twin of the content || style concat (elementwise.hip: ms_concat_style_fwd/bwd).  EmbLin's 'lin' mode
// (layers.py:659-663, JL:159-180) gives every frame a weighted mix of embedding rows, x.matmul(emb.weight); here the mix, the
// transpose and the cat are one launch in the channel-major layout of the id kernel:
//   out[b,c,t] = x[b,c,t] (c < C),   out[b,C+j,t] = sum_s w[b,t,s] * E[s][j]
// fp32, from zero, ascending s, one fma per term: a one-hot row returns the embedding row bit for bit, and nothing depends on
// the grid.  w is addressed as w[b*w_sb + t*w_st + s] (w_st = 0: one row per clip, the training branch's softmax of the style
// encoder's (B,S) scores); rows are used as given, not normalised.  The backward sums in fixed order, without atomics.
// The launches run under the id twin's labels: one call of a launcher here stands for one call of its twin (as the lr-word forms
// of adam.hip do for the Adam prep).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace ms {

// Every loop below requests a group of U values per operand before the first use (clamped indices, so no load sits behind a
// branch): one round trip per group instead of one per term (the rule of DESIGN 4d; softmax_mix_bwd_kernel has the pattern).
constexpr int MIX_US = 8;    // terms of the sum over styles in flight
constexpr int MIX_UD = 16;   // terms of the sum over the embedding dimension in flight
constexpr int MIX_UR = 4;    // terms per thread in flight in the block reductions

__global__ __launch_bounds__(256) void style_mix_fwd_kernel(const float* __restrict__ x, const float* __restrict__ emb,
                                                            const float* __restrict__ w, int w_sb, int w_st,
                                                            float* __restrict__ out, int C, int D, int T, int S, size_t total) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int t = (int)(i % T);
    const size_t bc = i / T;
    const int c = (int)(bc % (C + D)), b = (int)(bc / (C + D));
    if (c < C) {
      out[i] = x[((size_t)b * C + c) * T + t];
      continue;
    }
    const float* wr = w + (size_t)b * w_sb + (size_t)t * w_st;
    const float* er = emb + (c - C);
    float acc = 0.f;
    for (int s0 = 0; s0 < S; s0 += MIX_US) {
      float wv[MIX_US], ev[MIX_US];
#pragma unroll
      for (int u = 0; u < MIX_US; ++u) {
        const int s = min(s0 + u, S - 1);
        wv[u] = wr[s];
        ev[u] = er[(size_t)s * D];
      }
#pragma unroll
      for (int u = 0; u < MIX_US; ++u)
        if (s0 + u < S) acc = fmaf(wv[u], ev[u], acc);
    }
    out[i] = acc;
  }
}

// dx = dout[:, :C]
__global__ __launch_bounds__(256) void style_mix_bwd_x_kernel(const float* __restrict__ dout, float* __restrict__ dx, int C, int D,
                                                              int T, size_t total) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int t = (int)(i % T);
    const size_t bc = i / T;
    const int c = (int)(bc % C), b = (int)(bc / C);
    dx[i] = dout[((size_t)b * (C + D) + c) * T + t];
  }
}

// dE[s][j] = sum over (b,t) of w[b,t,s] * dout[b,C+j,t]: one workgroup per (j, s), thread-strided partial sums in ascending
// (b,t), then the fixed tree of block_sum_256.  A style whose weight is 0 everywhere gets a row of exact zeros.
__global__ __launch_bounds__(256) void style_mix_bwd_emb_kernel(const float* __restrict__ dout, const float* __restrict__ w,
                                                                int w_sb, int w_st, float* __restrict__ demb, int B, int C, int D,
                                                                int T) {
  __shared__ float red[4];
  const int j = blockIdx.x, sidx = blockIdx.y;
  const int n = B * T;
  const float* g = dout + (size_t)(C + j) * T;
  const float* ws = w + sidx;
  float acc = 0.f;
  for (int e0 = threadIdx.x; e0 < n; e0 += 256 * MIX_UR) {
    float wv[MIX_UR], gv[MIX_UR];
#pragma unroll
    for (int u = 0; u < MIX_UR; ++u) {
      const int e = min(e0 + u * 256, n - 1);
      const int b = e / T, t = e - b * T;
      wv[u] = ws[(size_t)b * w_sb + (size_t)t * w_st];
      gv[u] = g[(size_t)b * (C + D) * T + t];
    }
#pragma unroll
    for (int u = 0; u < MIX_UR; ++u)
      if (e0 + u * 256 < n) acc = fmaf(wv[u], gv[u], acc);
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) demb[(size_t)sidx * D + j] = acc;
}

// per-frame weights: dw[b,t,s] = sum_j dout[b,C+j,t] * E[s][j], ascending j, contiguous (B,T,S)
__global__ __launch_bounds__(256) void style_mix_bwd_w_frame_kernel(const float* __restrict__ dout, const float* __restrict__ emb,
                                                                    float* __restrict__ dw, int C, int D, int T, int S,
                                                                    size_t total) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int s = (int)(i % S);
    const size_t bt = i / S;
    const int t = (int)(bt % T), b = (int)(bt / T);
    const float* g = dout + ((size_t)b * (C + D) + C) * T + t;
    const float* er = emb + (size_t)s * D;
    float acc = 0.f;
    for (int j0 = 0; j0 < D; j0 += MIX_UD) {
      float gv[MIX_UD], ev[MIX_UD];
#pragma unroll
      for (int u = 0; u < MIX_UD; ++u) {
        const int j = min(j0 + u, D - 1);
        gv[u] = g[(size_t)j * T];
        ev[u] = er[j];
      }
#pragma unroll
      for (int u = 0; u < MIX_UD; ++u)
        if (j0 + u < D) acc = fmaf(gv[u], ev[u], acc);
    }
    dw[i] = acc;
  }
}

// per-clip weights: dw[b,s] = sum over (j,t) of dout[b,C+j,t] * E[s][j]: one workgroup per (b, s); the clip's D*T style
// gradients are contiguous in dout, thread-strided in ascending (j,t), then the fixed tree of block_sum_256
__global__ __launch_bounds__(256) void style_mix_bwd_w_clip_kernel(const float* __restrict__ dout, const float* __restrict__ emb,
                                                                   float* __restrict__ dw, int C, int D, int T, int S) {
  __shared__ float red[4];
  const int b = blockIdx.x / S, s = blockIdx.x - b * S;
  const int n = D * T;
  const float* g = dout + ((size_t)b * (C + D) + C) * T;
  const float* er = emb + (size_t)s * D;
  float acc = 0.f;
  for (int e0 = threadIdx.x; e0 < n; e0 += 256 * MIX_UR) {
    float gv[MIX_UR], ev[MIX_UR];
#pragma unroll
    for (int u = 0; u < MIX_UR; ++u) {
      const int e = min(e0 + u * 256, n - 1);
      gv[u] = g[e];
      ev[u] = er[e / T];
    }
#pragma unroll
    for (int u = 0; u < MIX_UR; ++u)
      if (e0 + u * 256 < n) acc = fmaf(gv[u], ev[u], acc);
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) dw[blockIdx.x] = acc;
}

static int style_mix_dims(const char* who, int B, int C, int D, int T, int S, int w_stride_b, int w_stride_t) {
  if (S < 1 || D < 1) return set_error("%s: S=%d D=%d (at least one style and one embedding column)", who, S, D);
  if (B < 1 || C < 0 || T < 1) return set_error("%s: B=%d C=%d T=%d", who, B, C, T);
  if (w_stride_b < 0 || w_stride_t < 0) return set_error("%s: negative weight strides (%d, %d)", who, w_stride_b, w_stride_t);
  if (S > 65535) return set_error("%s: S=%d (one grid row per style)", who, S);
  if ((long long)B * T > 0x7fffffffLL || (long long)D * T > 0x7fffffffLL || (long long)B * S > 0x7fffffffLL)
    return set_error("%s: B=%d T=%d D=%d S=%d exceed the 32-bit row counts of the reductions", who, B, T, D, S);
  return 0;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_concat_style_soft_fwd(const float* x, const float* emb, const float* w, int w_stride_b, int w_stride_t, float* out, int B,
                             int C, int D, int T, int S, void* stream) {
  if (int rc = style_mix_dims("ms_concat_style_soft_fwd", B, C, D, T, S, w_stride_b, w_stride_t)) return rc;
  if (!emb || !w || !out || (C > 0 && !x)) return set_error("ms_concat_style_soft_fwd: x, emb, w and out are required");
  TimingScope ts((hipStream_t)stream, 0, 0, "ew|ew_concat_style_fwd");
  if (ts.skip()) return 0;
  const size_t total = (size_t)B * (C + D) * T;
  int blocks = (int)std::min<size_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(style_mix_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, emb, w, w_stride_b, w_stride_t, out,
                     C, D, T, S, total);
  return check_launch("style_mix_fwd_kernel");
}

int ms_concat_style_soft_bwd(const float* dout, const float* emb, const float* w, int w_stride_b, int w_stride_t, float* dx,
                             float* demb, float* dw, int B, int C, int D, int T, int S, void* stream) {
  if (int rc = style_mix_dims("ms_concat_style_soft_bwd", B, C, D, T, S, w_stride_b, w_stride_t)) return rc;
  if (!dout || (demb && !w) || (dw && !emb)) return set_error("ms_concat_style_soft_bwd: dout, w (for demb) and emb (for dw) are required");
  TimingScope ts((hipStream_t)stream, 0, 0, "ew|ew_concat_style_bwd");
  if (ts.skip()) return 0;
  if (dx && C > 0) {
    const size_t total = (size_t)B * C * T;
    int blocks = (int)std::min<size_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(style_mix_bwd_x_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dout, dx, C, D, T, total);
    int rc = check_launch("style_mix_bwd_x_kernel");
    if (rc) return rc;
  }
  if (demb) {
    hipLaunchKernelGGL(style_mix_bwd_emb_kernel, dim3(D, S), dim3(256), 0, (hipStream_t)stream, dout, w, w_stride_b, w_stride_t,
                       demb, B, C, D, T);
    int rc = check_launch("style_mix_bwd_emb_kernel");
    if (rc) return rc;
  }
  if (dw && w_stride_t != 0) {
    const size_t total = (size_t)B * T * S;
    int blocks = (int)std::min<size_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(style_mix_bwd_w_frame_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dout, emb, dw, C, D, T, S,
                       total);
    return check_launch("style_mix_bwd_w_frame_kernel");
  }
  if (dw) {
    hipLaunchKernelGGL(style_mix_bwd_w_clip_kernel, dim3(B * S), dim3(256), 0, (hipStream_t)stream, dout, emb, dw, C, D, T, S);
    return check_launch("style_mix_bwd_w_clip_kernel");
  }
  return 0;
}

}  // extern "C"
