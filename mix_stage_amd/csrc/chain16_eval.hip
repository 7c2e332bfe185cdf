// Chained pose decoder, eval mode, 16-bit arithmetic (bf16 / fp16 operands, fp32 accumulate, BatchNorm from the running
// statistics in the fp32 epilogue): the wait-free form of chain16.hip for any batch size and sequence length.  Decomposition,
// tile plan, masking and mixture: chain32_eval.hip / chain_eval.h; weight streaming and LDS image: chain16.hip (the prepared
// streams are the same ones -- unfolded weights: blocks marked for BatchNorm folding are served with the scale applied in fp32).
#include "conv16_kernel.h"
#include "chain_eval.h"

namespace ms {

// (the geometry of chain16.hip: the prepared streams are shared)
constexpr int E16_C = 256, E16_NL = 4;
constexpr int E16_PITCH = 68;
constexpr int E16_CB0 = 34;
constexpr int E16_IMG0 = E16_CB0 * E16_PITCH, E16_IMG1 = 32 * E16_PITCH;
constexpr int E16_SPL = 516;
constexpr int E16_SCR = 32 * E16_SPL;
constexpr int E16_RING = 24;
constexpr int E16_UNITS_X = 3, E16_UNITS_L = 48, E16_UNITS_LOGIT = 8, E16_UNITS_SLACK = 16;
constexpr int E16_UNITS = E16_UNITS_X + E16_NL * E16_UNITS_L + E16_UNITS_LOGIT + E16_UNITS_SLACK;
constexpr size_t E16_WAVE_STREAM = (size_t)E16_UNITS * 128;
constexpr int E16_MAXM = 32;
constexpr int E16_LDS_BYTES = (E16_IMG0 + E16_IMG1) * 16 + E16_SCR * 4 + (3 * E16_NL * 256 + 64 + 8) * 4;
static_assert(CE_PPAD * CE_MT_PITCH <= E16_SCR, "the mixture tile lives in the epilogue scratch");

struct Chain16EvalArgs {
  const u32x4* x;             // cb8 (B, 34, T)
  const u32x4* wp;            // prepared weight streams [M][4][E16_WAVE_STREAM]
  const float* bias[E16_NL];
  const float* gamma[E16_NL];
  const float* beta[E16_NL];
  const float* rm[E16_NL];
  const float* rv[E16_NL];
  const float* bias_l;
  float* z;                   // (B, M*P, T) fp32 or null
  const float* score;         // (B, M, T)
  float* soft;                // (B, T, M) or null
  float* out;                 // (B, T, P)
  float* part;
  int* cnt;
  int B, M, P, T, n_tiles, gpw, ngw;
  float slope, eps;
};

// (an instance of the chain16_kernel family -- the launch labels and the profiles group the decoder chain's kernels by that name --
// told apart by the second template argument)
enum Chain16Form { CHAIN16_FORM_EVAL = 1 };
template <typename DT, Chain16Form FORM>
__global__ __launch_bounds__(256, 1) void chain16_kernel(const Chain16EvalArgs p) {
  prefetch_kernargs<sizeof(Chain16EvalArgs)>();
  extern __shared__ u32x4 smem16e[];
  u32x4* imgA = smem16e;
  u32x4* imgB = imgA + E16_IMG0;
  float* scr = reinterpret_cast<float*>(imgB + E16_IMG1);
  float* tb0 = scr + E16_SCR;               // [NL][256] bias
  float* tb1 = tb0 + E16_NL * 256;          // scale
  float* tb2 = tb1 + E16_NL * 256;          // shift
  float* sg = tb2 + E16_NL * 256;           // [64] the current group's softmax weight per frame of the tile
  int* lflag = reinterpret_cast<int*>(sg + 64);

  const int t = threadIdx.x, lane = t & 63, w = t >> 6, n0 = lane & 31, h = lane >> 5;
  const ChainEvalTileId tl = chain_eval_tile(p.B, p.n_tiles, p.T);
  const int b = tl.b, s0 = tl.s0, nv = tl.nv, own_lo = tl.own_lo, own_hi = tl.own_hi;
  const int g_lo = tl.jc * p.gpw, g_hi = min(p.M, g_lo + p.gpw);

  // halos (vector slots 0 and 65..67 of every plane): written once, nothing else touches them
  for (int e = t; e < (E16_CB0 + 32) * 4; e += 256) {
    const int plane = e >> 2, s = e & 3;
    u32x4* pl = plane < E16_CB0 ? imgA + plane * E16_PITCH : imgB + (plane - E16_CB0) * E16_PITCH;
    pl[s == 0 ? 0 : 64 + s] = u32x4{0u, 0u, 0u, 0u};
  }

  float oacc[2][16];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int q = 0; q < 16; ++q) oacc[nb][q] = 0.f;

  for (int g = g_lo; g < g_hi; ++g) {
    // this wave's weight stream through a buffer descriptor: the lane in the vector offset, the stream position in the scalar
    // offset -- no 64-bit address register per load in flight (the group loop's accumulators need the room)
    const __amdgpu_buffer_rsrc_t rsW = buf_rsrc(p.wp + ((size_t)g * 4 + __builtin_amdgcn_readfirstlane(w)) * E16_WAVE_STREAM);
    const unsigned wlane = 16u * (unsigned)lane;
    auto ld_w = [&](unsigned vec) {         // vector `vec` (uniform) + lane of the stream
      return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsW, (int)wlane, (int)(16u * vec), 0));
    };
    u32x4 rx[E16_UNITS_X][2], ra[E16_RING][2];
    {
      // (an opaque zero per group: the load addresses below are computed HERE in every pass instead of being hoisted out of the
      // group loop and kept alive across the K loops, where the register file is full)
      int opq = 0;
      asm volatile("" : "+s"(opq));
      const int tp = t + opq, lp = lane + opq;
      // the input image is staged again for every group (block 1 overwrites it; 35 KB from L2)
      constexpr int NX = (E16_CB0 * CE_T + 255) / 256;
      const u32x4* xb = p.x + (size_t)b * E16_CB0 * p.T + s0;
      u32x4 xv[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int e = min(tp + 256 * i, E16_CB0 * CE_T - 1);
        xv[i] = xb[(size_t)(e >> 6) * p.T + min(e & 63, nv - 1)];
      }
      float q0[E16_NL], q1[E16_NL], q2[E16_NL], q3[E16_NL], q4[E16_NL];
      const int cgp = g * E16_C + tp;
#pragma unroll
      for (int l = 0; l < E16_NL; ++l) {
        q0[l] = p.bias[l] ? p.bias[l][cgp] : 0.f;
        q1[l] = p.gamma[l][cgp];
        q2[l] = p.beta[l][cgp];
        q3[l] = p.rm[l][cgp];
        q4[l] = p.rv[l][cgp];
      }
      float sv[E16_MAXM];
      {
        const __amdgpu_buffer_rsrc_t rsS = buf_rsrc(p.score + (size_t)b * p.M * p.T + opq);
        const unsigned fo = 4u * (unsigned)(s0 + min(lp, nv - 1));
#pragma unroll
        for (int m = 0; m < E16_MAXM; ++m) sv[m] = buf_load(rsS, fo, 4u * (unsigned)(min(m, p.M - 1) * p.T));
      }
      // the weight ring's first fill, behind the loads above
#pragma unroll
      for (int j = 0; j < E16_UNITS_X; ++j)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) rx[j][mb] = ld_w((unsigned)(j * 128 + mb * 64));
#pragma unroll
      for (int j = 0; j < E16_RING; ++j)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) ra[j][mb] = ld_w((unsigned)((E16_UNITS_X + j) * 128 + mb * 64));

#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int e = tp + 256 * i;
        if (e < E16_CB0 * CE_T) imgA[(e >> 6) * E16_PITCH + 1 + (e & 63)] = (e & 63) < nv ? xv[i] : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int l = 0; l < E16_NL; ++l) {
        const float sc = q1[l] * (1.0f / sqrtf(q4[l] + p.eps));
        tb0[l * 256 + tp] = q0[l];
        tb1[l * 256 + tp] = sc;
        tb2[l * 256 + tp] = q2[l] - q3[l] * sc;
      }
      if (tp < CE_T) {
        // softmax over the M cluster scores of frame s0 + t (JL:186-187); the first workgroup of the tile writes the monitor tensor
        float mx = sv[0];
#pragma unroll
        for (int m = 1; m < E16_MAXM; ++m) mx = m < p.M ? fmaxf(mx, sv[m]) : mx;
        float den = 0.f, mine = 0.f;
#pragma unroll
        for (int m = 0; m < E16_MAXM; ++m) {
          sv[m] = m < p.M ? __expf(sv[m] - mx) : 0.f;
          den += sv[m];
          mine = m == g ? sv[m] : mine;
        }
        sg[tp] = mine / den;
        if (g == 0 && p.soft && tp >= own_lo && tp < own_hi) {
#pragma unroll
          for (int m = 0; m < E16_MAXM; ++m)
            if (m < p.M) p.soft[((size_t)b * p.T + s0 + tp) * p.M + m] = sv[m] / den;
        }
      }
    }

    f32x16 acc[2][2];
    unsigned pos = E16_UNITS_X;             // stream position of ring slot 0's current unit
    u32x4* bin = imgA;
    u32x4* bout = imgB;

    // 24 units = k-steps ks0 .. ks0+7 x 3 taps against the resident image; every slot is refilled with the unit 24 positions on
    // (branch-free and identical for every half, the stream's last one included: chain16.hip)
    auto run_half = [&](const u32x4* img, int ks0) {
      u32x4 bf[4][2];
      auto fetch_b = [&](int j, u32x4 (&dst)[2]) {
        const int ks = j / 3, tap = j - 3 * ks;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) dst[nb] = img[(2 * (ks0 + ks) + h) * E16_PITCH + 32 * nb + n0 + tap];
      };
      fetch_b(0, bf[0]);
      fetch_b(1, bf[1]);
      fetch_b(2, bf[2]);
#pragma unroll
      for (int j = 0; j < E16_RING; ++j) {
        if (j + 3 < E16_RING) fetch_b(j + 3, bf[(j + 3) & 3]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = DT::mfma(ra[j][mb], bf[j & 3][nb], acc[mb][nb]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) ra[j][mb] = ld_w((pos + E16_RING + j) * 128 + mb * 64);
      }
      pos += E16_RING;
    };

    for (int l = 0; l < E16_NL; ++l) {
      const float* pb = tb0 + l * 256;
      const float* psc = tb1 + l * 256;
      const float* psh = tb2 + l * 256;
      if (l == 0) __syncthreads();          // the input image, the tables and sg are complete
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[mb][nb][q] = 0.f;

      if (l == 0) {
        // block 0's 17th k-step (the style channels 256..271): its three units came first in the stream
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
          u32x4 bfx[2];
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) bfx[nb] = bin[(32 + h) * E16_PITCH + 32 * nb + n0 + tap];
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = DT::mfma(rx[tap][mb], bfx[nb], acc[mb][nb]);
        }
      }
      run_half(bin, 0);
      run_half(bin, 8);
      __syncthreads();                      // the scratch is free (the previous block's epilogue, the previous group's logits tile)

      // ---- epilogue: conv + bias (fp32) through the scratch [channel block][frame][8]; thread (cb, pq) then owns frames 8*k + pq
      {
        const int cb0 = 8 * w;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const int c0 = 64 * w + 32 * mb + 8 * rq + 4 * h;
            const float4 bs = *reinterpret_cast<const float4*>(pb + c0);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
              const float4 v = {acc[mb][nb][4 * rq] + bs.x, acc[mb][nb][4 * rq + 1] + bs.y, acc[mb][nb][4 * rq + 2] + bs.z,
                                acc[mb][nb][4 * rq + 3] + bs.w};
              *reinterpret_cast<float4*>(scr + (cb0 + 4 * mb + rq) * E16_SPL + (32 * nb + n0) * 8 + 4 * h) = v;
            }
          }
      }
      __syncthreads();
      {
        // BatchNorm (running statistics) + LeakyReLU: 8 frames x 8 channels per thread -> cb8 vectors of the next block's input
        // image; frames outside the sequence are zero (they are the next conv's zero padding)
        const int cb = t >> 3, pq = t & 7;
        const float4 sc0 = *reinterpret_cast<const float4*>(psc + 8 * cb), sc1 = *reinterpret_cast<const float4*>(psc + 8 * cb + 4);
        const float4 sh0 = *reinterpret_cast<const float4*>(psh + 8 * cb), sh1 = *reinterpret_cast<const float4*>(psh + 8 * cb + 4);
        const float scv[8] = {sc0.x, sc0.y, sc0.z, sc0.w, sc1.x, sc1.y, sc1.z, sc1.w};
        const float shv[8] = {sh0.x, sh0.y, sh0.z, sh0.w, sh1.x, sh1.y, sh1.z, sh1.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int px = 8 * k + pq;
          const float4 lo = *reinterpret_cast<const float4*>(scr + cb * E16_SPL + px * 8);
          const float4 hi = *reinterpret_cast<const float4*>(scr + cb * E16_SPL + px * 8 + 4);
          const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
          float yv[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) yv[j] = lrelu(fmaf(v[j], scv[j], shv[j]), p.slope);
          bout[cb * E16_PITCH + 1 + px] = px < nv ? pack8<DT>(yv) : u32x4{0u, 0u, 0u, 0u};
        }
      }
      __syncthreads();
      u32x4* tmp = bin; bin = bout; bout = tmp;
      if (l == 0) bout = imgA;
    }

    // ---- logits (1x1; this wave's 32 of the P rows) + the group's mixture term; the 8 logits units sit in ring slots 0..7
    {
      f32x16 za[2];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int q = 0; q < 16; ++q) za[nb][q] = 0.f;
#pragma unroll
      for (int u = 0; u < E16_UNITS_LOGIT; ++u)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int ks = 2 * u + e;
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
            const u32x4 bv = bin[(2 * ks + h) * E16_PITCH + 1 + 32 * nb + n0];
            za[nb] = DT::mfma(ra[u][e], bv, za[nb]);
          }
        }
      const float sw0 = sg[n0], sw1 = sg[32 + n0];
      // (an opaque zero again: z's row offsets are formed here, not carried through the group loop)
      int opz = 0;
      asm volatile("" : "+s"(opz));
      const int Tz = p.T + opz;
      float* zb = p.z ? p.z + ((size_t)b * p.M + g) * p.P * p.T + s0 : nullptr;
      const bool own0 = n0 >= own_lo && n0 < own_hi, own1 = 32 + n0 >= own_lo && 32 + n0 < own_hi;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int prow = 32 * w + 8 * (q >> 2) + 4 * h + (q & 3);
        const float bl = prow < p.P ? p.bias_l[g * p.P + prow] : 0.f;
        const float z0 = za[0][q] + bl, z1 = za[1][q] + bl;
        oacc[0][q] += sw0 * z0;
        oacc[1][q] += sw1 * z1;
        if (zb && prow < p.P) {               // the owned frames of this row: 32 consecutive floats per half wave
          if (own0) zb[prow * Tz + n0] = z0;
          if (own1) zb[prow * Tz + 32 + n0] = z1;
        }
      }
    }
    __syncthreads();                        // every read of the images, the tables, sg and the tile is done: the next group may stage
  }

  chain_eval_mix_out(scr, lflag, oacc, p.part, p.cnt, p.out, p.P, p.T, p.ngw, tl);
}

int chain16_eval_fwd(const ms_chain_desc* d, const ms_chain_tensors* tn, void* workspace, size_t workspace_bytes, hipStream_t s) {
  const ChainEvalPlan pl = chain_eval_plan(d);
  Chain16EvalArgs a = {};
  a.x = (const u32x4*)tn->x; a.wp = (const u32x4*)tn->prepared;
  for (int l = 0; l < E16_NL; ++l) {
    a.bias[l] = tn->bias[l]; a.gamma[l] = tn->gamma[l]; a.beta[l] = tn->beta[l]; a.rm[l] = tn->running_mean[l]; a.rv[l] = tn->running_var[l];
  }
  a.bias_l = tn->bias_logits; a.z = tn->z; a.score = tn->score; a.soft = tn->soft; a.out = tn->out;
  a.part = (float*)workspace;
  a.cnt = pl.ngw > 1 ? tn->sync + d->sync_first_word : nullptr;
  a.B = d->B; a.M = d->M; a.P = d->P; a.T = d->T; a.n_tiles = pl.n_tiles; a.gpw = pl.gpw; a.ngw = pl.ngw;
  a.slope = d->slope; a.eps = d->eps;
  static unsigned long long lds_done = 0;
  if (first_time_on_device(lds_done)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(chain16_kernel<BF16, CHAIN16_FORM_EVAL>), hipFuncAttributeMaxDynamicSharedMemorySize, E16_LDS_BYTES) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(chain16_kernel<F16, CHAIN16_FORM_EVAL>), hipFuncAttributeMaxDynamicSharedMemorySize, E16_LDS_BYTES) != hipSuccess)
      return set_error("ms_decoder_chain_eval_fwd: cannot raise the dynamic LDS limit");
    done_on_device(lds_done);
  }
  const char* dn = d->dtype == MS_BF16 ? "bf16" : "f16";
  // algorithmic work of the useful frames (the 8 of 64 recomputed ones are not counted)
  const double bt = (double)d->B * d->T;
  const double flops = 2.0 * bt * d->M * (E16_C * 3.0 * (d->cin0 + 3.0 * E16_C) + (double)d->P * E16_C);
  const double bytes = bt * (2.0 * 8 * E16_CB0 + 4.0 * (d->M + d->P)) + 2.0 * d->M * (E16_C * 3.0 * (d->cin0 + 3.0 * E16_C) + (double)d->P * E16_C);
  TimingScope ts(s, flops, bytes, "chain16_kernel<%s,eval>|decoder_chain_eval_fwd %s M%d B%d T%d P%d cin%d gpw%d", dn, dn, d->M, d->B, d->T, d->P,
                 d->cin0, pl.gpw);
  if (ts.skip()) return 0;
  if (d->dtype == MS_BF16) hipLaunchKernelGGL((chain16_kernel<BF16, CHAIN16_FORM_EVAL>), dim3((unsigned)(pl.units * pl.ngw)), dim3(256), E16_LDS_BYTES, s, a);
  else hipLaunchKernelGGL((chain16_kernel<F16, CHAIN16_FORM_EVAL>), dim3((unsigned)(pl.units * pl.ngw)), dim3(256), E16_LDS_BYTES, s, a);
  return check_launch("chain16_kernel<eval>");
}

}  // namespace ms
