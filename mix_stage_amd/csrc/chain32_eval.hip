// Chained pose decoder, eval mode, fp32: decoder.0-3 + logits + softmax mixture (JL:69-83,106-115,186-194) in one launch for ANY
// batch size and sequence length.  The recipe of chain32.hip (activations of a 64-frame image resident in LDS through the four
// blocks, every wave's weight rows streamed global -> registers in MFMA operand order from the SAME prepared streams, no barrier
// in a K loop), with what eval mode allows:
//
//  * BatchNorm uses the running statistics, so no layer needs the other workgroups: NO workgroup of this launch ever waits for
//    another one.  There is no residency condition and no error word.
//  * work unit = (sequence b, time tile k, chunk j of the groups).  Tile k computes frames [56k, 56k + 64) and owns
//    [56k + 4, 56k + 60) of them (the first tile from frame 0, the last one up to T): four k3 / pad 1 layers contaminate 4 frames
//    from a zero halo, so the 4 frames on an interior edge are recomputed by the neighbour (chain_eval_plan).
//  * frames outside [0, T) are zero at the input of EVERY layer (the reference zero-pads each conv's input; a block's output
//    beyond T is bias + BatchNorm shift, not zero): masked when a layer's output is written into the image.
//  * mixture: a workgroup carries `gpw` groups of its tile one after the other and accumulates softmax_m * z_m in the logits'
//    accumulator layout (32 registers).  gpw == M (many work units): the workgroup writes `out` itself.  gpw < M (few work units:
//    the groups spread over workgroups so that the chip fills): each workgroup stores its partial sum (sc1), and the one whose
//    agent-scope counter add came LAST -- told by the value the add returned, no poll -- sums the ceil(M / gpw) partials in
//    ascending order (MI355X hand-off: sc1 stores, every storing wave's s_waitcnt vmcnt(0), workgroup barrier, one atomic add by
//    one lane, workgroup barrier, sc1 loads).  The summation order is a function of the shape alone.  Counters are monotonic.
#include <algorithm>

#include "kernels.h"
#include "conv16.h"
#include "chain_eval.h"

namespace ms {

// (the geometry of chain32.hip: the prepared streams are shared)
constexpr int CE_C = 256;
constexpr int CE_NL = 4;
constexpr int CE_PITCH = 68;
constexpr int CE_PLANE = CE_PITCH * 4;
constexpr int CE_K8_0 = 34;
constexpr int CE_BUF0 = CE_K8_0 * 2 * CE_PLANE;
constexpr int CE_BUF1 = 32 * 2 * CE_PLANE;
constexpr int CE_BLK = 6;
constexpr int CE_NBLK0 = 17, CE_NBLK = 16;
constexpr int CE_CONV_BLOCKS = CE_NBLK0 + 3 * CE_NBLK;
constexpr int CE_LOGIT_Q = 32;
constexpr size_t CE_WAVE_STREAM = (size_t)CE_CONV_BLOCKS * CE_BLK * 2 * 256 + (size_t)CE_LOGIT_Q * 256 + 2 * CE_BLK * 2 * 256;
constexpr int CE_MAXM = 32;
constexpr int CE_LDS_FLOATS = CE_BUF0 + CE_BUF1 + 3 * CE_NL * 256 + 64 + 8;

// ---- the tile plan (host arithmetic only; shared with chain16_eval.hip)
ChainEvalPlan chain_eval_plan(const ms_chain_desc* d) {
  ChainEvalPlan pl;
  pl.n_tiles = d->T <= CHAIN_EVAL_TILE ? 1 : 1 + (d->T - CHAIN_EVAL_TILE + CHAIN_EVAL_STEP - 1) / CHAIN_EVAL_STEP;
  pl.units = (long)d->B * pl.n_tiles;
  // groups per workgroup from the shape alone.  A workgroup's time is ~gpw group passes and the launch runs in
  // ceil(workgroups / CHAIN_EVAL_FILL) rounds of one workgroup per compute unit: take the gpw with the fewest group passes end to
  // end, the larger one on a tie (fewer partial sums to exchange; gpw == M exchanges nothing), among those whose partial sums
  // stay within CHAIN_EVAL_MAX_PARTS tiles.  Few units (B = 1, 12 tiles): one group per workgroup, the chip fills; thousands of
  // units (B = 1024): all M groups in one workgroup.
  long best = 0;
  pl.gpw = d->M;
  for (int gpw = d->M; gpw >= 1; --gpw) {
    const int ngw = (d->M + gpw - 1) / gpw;
    if ((d->M + ngw - 1) / ngw != gpw) continue;            // (the smallest gpw of every ngw only)
    if (ngw > 1 && pl.units * ngw > CHAIN_EVAL_MAX_PARTS) continue;
    const long cost = ((pl.units * ngw + CHAIN_EVAL_FILL - 1) / CHAIN_EVAL_FILL) * gpw;
    if (!best || cost < best) { best = cost; pl.gpw = gpw; }
  }
  pl.ngw = (d->M + pl.gpw - 1) / pl.gpw;
  return pl;
}

int chain_eval_shape_ok(const ms_chain_desc* d) {
  return d && d->T >= 1 && d->C == CE_C && d->n_blocks == CE_NL && d->cin0 > CE_C && d->cin0 <= 8 * CE_K8_0 && d->P >= 1 &&
         d->P <= CE_PPAD && d->B >= 1 && d->M >= 1 && d->M <= CE_MAXM && d->mode == MS_BN_EVAL &&
         (d->dtype == MS_F32 || ((d->dtype == MS_BF16 || d->dtype == MS_F16) && d->cin0 > 8 * (CE_K8_0 - 1))) &&   // (16-bit x: 34 channel blocks)
         d->T <= (1 << 20) && (long)d->B * d->T <= (1l << 28);
}

size_t chain_eval_workspace(const ms_chain_desc* d) {
  const ChainEvalPlan pl = chain_eval_plan(d);
  return pl.ngw > 1 ? (size_t)pl.units * pl.ngw * CE_PPAD * CE_T * sizeof(float) + 256 : 256;
}

int chain_eval_sync_words(const ms_chain_desc* d) {
  const ChainEvalPlan pl = chain_eval_plan(d);
  return pl.ngw > 1 ? (int)(32 * pl.units) : 0;       // (a counter per (sequence, tile), each on a line of its own)
}

struct Chain32EvalArgs {
  const float* x;             // (B, cin0, T)
  const float* wp;            // prepared weight streams [M][4][CE_WAVE_STREAM]
  const float* bias[CE_NL];
  const float* gamma[CE_NL];
  const float* beta[CE_NL];
  const float* rm[CE_NL];
  const float* rv[CE_NL];
  const float* bias_l;        // (M*P)
  float* z;                   // (B, M*P, T) or null
  const float* score;         // (B, M, T)
  float* soft;                // (B, T, M) or null
  float* out;                 // (B, T, P)
  float* part;                // ngw > 1: [unit][ngw][128][64]
  int* cnt;                   // ngw > 1: [unit] counters, stride 32 words
  int B, M, P, cin0, T, n_tiles, gpw, ngw;
  float slope, eps;
};

__device__ __forceinline__ float ce_f4e(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// (an instance of the chain32_kernel family -- the launch labels and the profiles group the decoder chain's kernels by that name --
// told apart by the template argument)
enum ChainForm { CHAIN_FORM_EVAL = 1 };
template <ChainForm FORM>
__global__ __launch_bounds__(256, 1) void chain32_kernel(const Chain32EvalArgs p) {
  prefetch_kernargs<sizeof(Chain32EvalArgs)>();
  extern __shared__ float smem[];
  float* bufA = smem;
  float* bufB = bufA + CE_BUF0;
  float* tb0 = bufB + CE_BUF1;              // [NL][256] bias
  float* tb1 = tb0 + CE_NL * 256;           // scale
  float* tb2 = tb1 + CE_NL * 256;           // shift
  float* sg = tb2 + CE_NL * 256;            // [64] the current group's softmax weight per frame of the tile
  int* lflag = reinterpret_cast<int*>(sg + 64);

  const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 31, h = lane >> 5;
  const ChainEvalTileId tl = chain_eval_tile(p.B, p.n_tiles, p.T);
  const int b = tl.b, s0 = tl.s0, nv = tl.nv, own_lo = tl.own_lo, own_hi = tl.own_hi, jc = tl.jc;
  const int g_lo = jc * p.gpw, g_hi = min(p.M, g_lo + p.gpw);
  const int n0 = r;

  // halos (pixel slots 0 and 65..67 of every plane): written once, no layer touches them
  for (int e = t; e < (CE_K8_0 + 32) * 2 * 4; e += 256) {
    const int plane = e >> 2, s = e & 3;
    float* pl = (plane < CE_K8_0 * 2 ? bufA + plane * CE_PLANE : bufB + (plane - CE_K8_0 * 2) * CE_PLANE);
    *reinterpret_cast<float4*>(pl + (s == 0 ? 0 : 64 + s) * 4) = float4{0.f, 0.f, 0.f, 0.f};
  }

  float oacc[2][16];                        // sum over this workgroup's groups of softmax weight x logits, logits' MFMA layout
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int q = 0; q < 16; ++q) oacc[nb][q] = 0.f;

  for (int g = g_lo; g < g_hi; ++g) {
    const float4* ws = reinterpret_cast<const float4*>(p.wp + ((size_t)g * 4 + w) * CE_WAVE_STREAM) + lane;
    float4 ra0[CE_BLK][2], ra1[CE_BLK][2];
    {
      // every global load of the prologue goes out before the first LDS store.  The input image is staged again for every group
      // (block 1 overwrites it; 70 KB from L2 against 3.2 MB of weights per group)
      // (an opaque zero per group: the 68 + 32 load addresses below are computed HERE in every pass instead of being hoisted out of
      // the group loop and kept alive -- spilled -- across the K loops, where the register file is full)
      int opq = 0;
      asm volatile("" : "+s"(opq));
      constexpr int NPL = (CE_K8_0 * 2 + 3) / 4;
      // (buffer loads: the frame in the vector offset, the channel row in the scalar offset -- no 64-bit address per load)
      const __amdgpu_buffer_rsrc_t rsX = buf_rsrc(p.x + (size_t)b * p.cin0 * p.T + opq);
      const unsigned fo = 4u * (unsigned)(s0 + min(lane, nv - 1));
      float xv[NPL][4];
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const int pl = __builtin_amdgcn_readfirstlane(w) + 4 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = 4 * pl + j;
          xv[i][j] = buf_load(rsX, fo, 4u * (unsigned)(min(c, p.cin0 - 1) * p.T));
        }
      }
      float q0[CE_NL], q1[CE_NL], q2[CE_NL], q3[CE_NL], q4[CE_NL];
      const int cgp = g * CE_C + t + opq;
#pragma unroll
      for (int l = 0; l < CE_NL; ++l) {
        q0[l] = p.bias[l] ? p.bias[l][cgp] : 0.f;
        q1[l] = p.gamma[l][cgp];
        q2[l] = p.beta[l][cgp];
        q3[l] = p.rm[l][cgp];
        q4[l] = p.rv[l][cgp];
      }
      float sv[CE_MAXM];
      {
        const __amdgpu_buffer_rsrc_t rsS = buf_rsrc(p.score + (size_t)b * p.M * p.T + opq);
#pragma unroll
        for (int m = 0; m < CE_MAXM; ++m) sv[m] = buf_load(rsS, fo, 4u * (unsigned)(min(m, p.M - 1) * p.T));
      }
      // the weight ring's first fill, behind the loads above
#pragma unroll
      for (int uu = 0; uu < CE_BLK; ++uu)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
          ra0[uu][mb] = ws[((0 * CE_BLK + uu) * 2 + mb) * 64];
          ra1[uu][mb] = ws[((1 * CE_BLK + uu) * 2 + mb) * 64];
        }
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const int pl = w + 4 * i;
        if (pl < CE_K8_0 * 2) {
          const bool in = lane < nv;
          float4 v;
          v.x = in && 4 * pl < p.cin0 ? xv[i][0] : 0.f;
          v.y = in && 4 * pl + 1 < p.cin0 ? xv[i][1] : 0.f;
          v.z = in && 4 * pl + 2 < p.cin0 ? xv[i][2] : 0.f;
          v.w = in && 4 * pl + 3 < p.cin0 ? xv[i][3] : 0.f;
          *reinterpret_cast<float4*>(bufA + pl * CE_PLANE + (1 + lane) * 4) = v;
        }
      }
#pragma unroll
      for (int l = 0; l < CE_NL; ++l) {
        const float sc = q1[l] * (1.0f / sqrtf(q4[l] + p.eps));
        tb0[l * 256 + t] = q0[l];
        tb1[l * 256 + t] = sc;
        tb2[l * 256 + t] = q2[l] - q3[l] * sc;
      }
      if (t < CE_T) {
        // softmax over the M cluster scores of frame s0 + t (JL:186-187); the first workgroup of the tile writes the monitor tensor
        float mx = sv[0];
#pragma unroll
        for (int m = 1; m < CE_MAXM; ++m) mx = m < p.M ? fmaxf(mx, sv[m]) : mx;
        float den = 0.f, mine = 0.f;
#pragma unroll
        for (int m = 0; m < CE_MAXM; ++m) {
          sv[m] = m < p.M ? __expf(sv[m] - mx) : 0.f;
          den += sv[m];
          mine = m == g ? sv[m] : mine;
        }
        sg[t] = mine / den;
        if (g == 0 && p.soft && t >= own_lo && t < own_hi) {
#pragma unroll
          for (int m = 0; m < CE_MAXM; ++m)
            if (m < p.M) p.soft[((size_t)b * p.T + s0 + t) * p.M + m] = sv[m] / den;
        }
      }
    }

    f32x16 acc[2][2];
    size_t blk = 0;
    float* bin = bufA;
    float* bout = bufB;

    auto run_block = [&](float4 (&ra)[CE_BLK][2], const float* bb, size_t refill) {
      float4 bf[2][2];
      auto fetch_b = [&](int uu, float4 (&dst)[2]) {
        const int k8s = uu / 3, tap = uu - 3 * k8s;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          dst[nb] = *reinterpret_cast<const float4*>(bb + (k8s * 2 + h) * CE_PLANE + (32 * nb + n0 + tap) * 4);
      };
      fetch_b(0, bf[0]);
#pragma unroll
      for (int uu = 0; uu < CE_BLK; ++uu) {
        if (uu + 1 < CE_BLK) fetch_b(uu + 1, bf[(uu + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
              acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ce_f4e(ra[uu][mb], j), ce_f4e(bf[uu & 1][nb], j), acc[mb][nb], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) ra[uu][mb] = ws[((refill * CE_BLK + uu) * 2 + mb) * 64];
      }
    };

    for (int l = 0; l < CE_NL; ++l) {
      const float* pb = tb0 + l * 256;
      const float* psc = tb1 + l * 256;
      const float* psh = tb2 + l * 256;
      if (l == 0) __syncthreads();           // the input image, the tables and sg are complete
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[mb][nb][q] = 0.f;

      const float* bb = bin;
      if (l == 0) {                          // block 0 has 17 stream blocks: the odd one first
        run_block(ra0, bb, blk + 2);
        ++blk; bb += 4 * CE_PLANE;
      }
      for (int dd = 0; dd < CE_NBLK / 2; ++dd) {
        run_block(ra1, bb, blk + 2);
        run_block(ra0, bb + 4 * CE_PLANE, blk + 3);
        blk += 2; bb += 8 * CE_PLANE;
      }

      // ---- epilogue: conv + bias into the output image, then BatchNorm (running statistics) + LeakyReLU in place, frames
      // outside the sequence zeroed (they are the next conv's zero padding)
      const int wc = 64 * w;
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int c0 = wc + 32 * mb + 8 * rq + 4 * h;
          const float4 bs = *reinterpret_cast<const float4*>(pb + c0);
          const float4 sc = *reinterpret_cast<const float4*>(psc + c0);
          const float4 sh = *reinterpret_cast<const float4*>(psh + c0);
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
            const bool in = 32 * nb + n0 < nv;
            float4 v = {lrelu(fmaf(acc[mb][nb][4 * rq] + bs.x, sc.x, sh.x), p.slope),
                        lrelu(fmaf(acc[mb][nb][4 * rq + 1] + bs.y, sc.y, sh.y), p.slope),
                        lrelu(fmaf(acc[mb][nb][4 * rq + 2] + bs.z, sc.z, sh.z), p.slope),
                        lrelu(fmaf(acc[mb][nb][4 * rq + 3] + bs.w, sc.w, sh.w), p.slope)};
            if (!in) v = float4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<float4*>(bout + ((c0 >> 3) * 2 + h) * CE_PLANE + (1 + 32 * nb + n0) * 4) = v;
          }
        }
      __syncthreads();                       // the next block's input image is complete
      float* tmp = bin; bin = bout; bout = tmp;
      if (l == 0) bout = bufA;
    }

    // ---- logits (1x1, P rows of this group) and this group's term of the mixture
    {
      const float4* wl = ws + (size_t)CE_CONV_BLOCKS * CE_BLK * 2 * 64;
      f32x16 za[2];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int q = 0; q < 16; ++q) za[nb][q] = 0.f;
      float4 wv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) wv[i] = wl[i * 64];
      for (int q0 = 0; q0 < CE_LOGIT_Q; q0 += 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float4 bfr[2];
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
            bfr[nb] = *reinterpret_cast<const float4*>(bin + ((q0 + i) * 2 + h) * CE_PLANE + (1 + 32 * nb + n0) * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) za[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ce_f4e(wv[i], j), ce_f4e(bfr[nb], j), za[nb], 0, 0, 0);
          wv[i] = wl[(size_t)(min(q0 + 8 + i, CE_LOGIT_Q - 1)) * 64];
        }
      }
      // rows prow = 32*w + 8*(q>>2) + 4*h + (q&3); this lane's frames are 32*nb + n0
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
    __syncthreads();                         // every read of the images, the tables and sg is done: the next group may stage
  }

  chain_eval_mix_out(bufB, lflag, oacc, p.part, p.cnt, p.out, p.P, p.T, p.ngw, tl);
}

static int chain32_eval_fwd(const ms_chain_desc* d, const ms_chain_tensors* tn, void* workspace, size_t workspace_bytes, hipStream_t s) {
  const ChainEvalPlan pl = chain_eval_plan(d);
  Chain32EvalArgs a = {};
  a.x = (const float*)tn->x; a.wp = (const float*)tn->prepared;
  for (int l = 0; l < CE_NL; ++l) {
    a.bias[l] = tn->bias[l]; a.gamma[l] = tn->gamma[l]; a.beta[l] = tn->beta[l]; a.rm[l] = tn->running_mean[l]; a.rv[l] = tn->running_var[l];
  }
  a.bias_l = tn->bias_logits; a.z = tn->z; a.score = tn->score; a.soft = tn->soft; a.out = tn->out;
  a.part = (float*)workspace;
  a.cnt = pl.ngw > 1 ? tn->sync + d->sync_first_word : nullptr;
  a.B = d->B; a.M = d->M; a.P = d->P; a.cin0 = d->cin0; a.T = d->T; a.n_tiles = pl.n_tiles; a.gpw = pl.gpw; a.ngw = pl.ngw;
  a.slope = d->slope; a.eps = d->eps;
  static unsigned long long lds_done = 0;
  if (first_time_on_device(lds_done)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(chain32_kernel<CHAIN_FORM_EVAL>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            CE_LDS_FLOATS * (int)sizeof(float)) != hipSuccess)
      return set_error("ms_decoder_chain_eval_fwd: cannot raise the dynamic LDS limit");
    done_on_device(lds_done);
  }
  // algorithmic work of the useful frames (the 8 of 64 recomputed ones are not counted)
  const double bt = (double)d->B * d->T;
  const double flops = 2.0 * bt * d->M * (CE_C * 3.0 * (d->cin0 + 3.0 * CE_C) + (double)d->P * CE_C);
  const double bytes = 4.0 * (bt * (d->cin0 + d->M + d->P) + (double)d->M * (CE_C * 3.0 * (d->cin0 + 3.0 * CE_C) + (double)d->P * CE_C));
  TimingScope ts(s, flops, bytes, "chain32_kernel<eval>|decoder_chain_eval_fwd f32 M%d B%d T%d P%d cin%d gpw%d", d->M, d->B, d->T, d->P, d->cin0, pl.gpw);
  if (ts.skip()) return 0;
  hipLaunchKernelGGL(chain32_kernel<CHAIN_FORM_EVAL>, dim3((unsigned)(pl.units * pl.ngw)), dim3(256), CE_LDS_FLOATS * sizeof(float), s, a);
  return check_launch("chain32_kernel<eval>");
}

}  // namespace ms

using namespace ms;
extern "C" {
int ms_decoder_chain_eval_supported(const ms_chain_desc* d) { return chain_eval_shape_ok(d); }
size_t ms_decoder_chain_eval_workspace(const ms_chain_desc* d) { return chain_eval_shape_ok(d) ? chain_eval_workspace(d) : 256; }
int ms_decoder_chain_eval_sync_words(const ms_chain_desc* d) { return chain_eval_shape_ok(d) ? chain_eval_sync_words(d) : 0; }
int ms_decoder_chain_eval_plan(const ms_chain_desc* d, int32_t* n_tiles, int32_t* groups_per_workgroup, int32_t* tile_first,
                               int32_t* own_lo, int32_t* own_hi, int32_t cap) {
  if (!d || d->mode != MS_BN_EVAL) return set_error("ms_decoder_chain_eval_plan: the eval form serves MS_BN_EVAL only");
  if (!chain_eval_shape_ok(d)) return set_error("ms_decoder_chain_eval_plan: unsupported shape (ms_decoder_chain_eval_supported)");
  const ChainEvalPlan pl = chain_eval_plan(d);
  if (n_tiles) *n_tiles = pl.n_tiles;
  if (groups_per_workgroup) *groups_per_workgroup = pl.gpw;
  if (tile_first || own_lo || own_hi) {
    if (cap < pl.n_tiles) return set_error("ms_decoder_chain_eval_plan: %d tiles, room for %d", pl.n_tiles, cap);
    for (int k = 0; k < pl.n_tiles; ++k) {
      const int s0 = CHAIN_EVAL_STEP * k;
      if (tile_first) tile_first[k] = s0;
      if (own_lo) own_lo[k] = k == 0 ? 0 : s0 + CHAIN_EVAL_HALO;
      if (own_hi) own_hi[k] = s0 + CHAIN_EVAL_TILE >= d->T ? d->T : s0 + CHAIN_EVAL_TILE - CHAIN_EVAL_HALO;
    }
  }
  return 0;
}
int ms_decoder_chain_eval_fwd(const ms_chain_desc* d, const ms_chain_tensors* t, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !t) return set_error("ms_decoder_chain_eval_fwd: null argument");
  if (d->mode != MS_BN_EVAL) return set_error("ms_decoder_chain_eval_fwd: the eval form serves MS_BN_EVAL only (train mode: ms_decoder_chain_fwd)");
  if (!chain_eval_shape_ok(d)) return set_error("ms_decoder_chain_eval_fwd: unsupported shape (ms_decoder_chain_eval_supported)");
  if (!t->x || !t->score || !t->out || !t->prepared || !t->bias_logits) return set_error("ms_decoder_chain_eval_fwd: null tensor");
  for (int l = 0; l < CE_NL; ++l)
    if (!t->gamma[l] || !t->beta[l] || !t->running_mean[l] || !t->running_var[l]) return set_error("ms_decoder_chain_eval_fwd: BN tensors missing");
  if (workspace_bytes < chain_eval_workspace(d) || !workspace) return set_error("ms_decoder_chain_eval_fwd: workspace too small");
  const int words = chain_eval_sync_words(d);
  if (words && (!t->sync || t->sync_words < d->sync_first_word + words)) return set_error("ms_decoder_chain_eval_fwd: sync buffer too small");
  return d->dtype == MS_F32 ? chain32_eval_fwd(d, t, workspace, workspace_bytes, (hipStream_t)stream)
                            : chain16_eval_fwd(d, t, workspace, workspace_bytes, (hipStream_t)stream);
}
}
