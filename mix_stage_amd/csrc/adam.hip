// The trainer's Adam step (torch.optim.Adam defaults: no amsgrad, no weight decay) with clip_grad_norm_ folded in: the
// unsegmented step, and the segmented step of FlatAdam with its three optional features.  Every form of the segmented step is TWO
// launches under one label (`ew|ew_adam_step_segmented`): a one-workgroup prep kernel -- one template, instantiated per form -- and
// the element pass.  No feature adds a launch or a pass over the parameters:
//   * Loss scale (fp16 training; the backward pass was seeded with the scale S instead of 1).  The prep kernel un-scales the
//     gradient norm, folds 1/S into the clip coefficient the element pass multiplies every gradient with anyway, decides whether
//     the step is applied, and moves S -- so a captured step follows the scale from replay to replay: the prep kernel at the end
//     of step k writes the word the loss kernels of step k+1 read their incoming gradient from.
//   * Learning rate in a device word.  The prep kernel READS lr when it runs instead of receiving it as a kernel argument.  A step
//     captured into a HIP graph then follows a learning-rate schedule from replay to replay (the reference steps ExponentialLR
//     once per epoch, TR:311-313, 499-500): the host writes the word between steps, on the stream the replays run on.  The same
//     bits as lr by value for the same lr.
//   * An exponential moving average (EMA) of the weights.  The EMA instance of the element pass reads and writes `ema` next to p,
//     m and v.  An element the pass leaves alone -- a refused step (step_state word 2: non-finite norm, overflow skip, bad lr
//     word), a segment that never had a gradient or whose first step is still ahead -- keeps its average.
#include <algorithm>
#include <type_traits>

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.h"

namespace ms {

// state words: [0] step (int32), [1] clip coef (NaN: the gradient norm was not finite, the update is skipped), [2] step_size = lr/bc1, [3] sqrt(bc2)
__global__ void adam_prep_kernel(int32_t* state, const float* norm, float max_norm, float lr, float beta1, float beta2) {
  const int step = state[0] + 1;
  state[0] = step;
  float* f = reinterpret_cast<float*>(state);
  float coef = 1.f;
  if (norm) {
    coef = max_norm / (norm[0] + 1e-6f);
    if (coef > 1.f) coef = 1.f;
    if (!(fabsf(norm[0]) <= 3.0e38f)) coef = __builtin_nanf("");   // non-finite gradient: adam_kernel leaves p, m, v untouched
  }
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  f[1] = coef;
  f[2] = (float)((double)lr / bc1);
  f[3] = (float)sqrt(bc2);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, size_t n, const int32_t* __restrict__ state,
                                                   float beta1, float beta2, float eps) {
  const float* f = reinterpret_cast<const float*>(state);
  const float coef = f[1], step_size = f[2], bc2s = f[3];
  if (coef != coef) return;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float gi = g[i] * coef;
    const float mi = m[i] + (1.f - beta1) * (gi - m[i]);
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= step_size * (mi / (sqrtf(vi) / bc2s + eps));
  }
}

// ---- device code of the segmented step's prep kernel.  One definition of each formula: every form gives the same bits for the
// same inputs.
// (lr / bias correction 1, in fp64 and rounded once) of a segment at its step count t >= 1 ...
__device__ inline float adam_seg_step_size(float lr, float beta1, double t) { return (float)((double)lr / (1.0 - pow((double)beta1, t))); }
// ... and sqrt(bias correction 2)
__device__ inline float adam_seg_bc2(float beta2, double t) { return (float)sqrt(1.0 - pow((double)beta2, t)); }
// clip_grad_norm_'s coefficient for the true gradient norm n
__device__ inline float adam_clip_coef(float max_norm, float n) {
  const float coef = max_norm / (n + 1e-6f);
  return coef > 1.f ? 1.f : coef;
}
__device__ inline bool adam_norm_finite(float n) { return fabsf(n) <= 3.0e38f; }
// a learning-rate word no step may be taken with: NaN, infinite, negative or zero
__device__ inline bool adam_lr_bad(float lr) { return !(lr > 0.f && lr <= 3.0e38f); }
// health words of step_state: [2] = the step is refused (adam_seg_kernel returns on it), [3] counts refused steps
__device__ inline void adam_flag_step(int32_t* state, bool bad) {
  state[2] = bad ? 1 : 0;
  if (bad) state[3] += 1;
}
// loss scaling: did an in-launch meeting behind this step raise its error word?  Scanned by the whole workgroup and only when the
// step is not finite; the caller combines the result over the workgroup (__syncthreads_or)
__device__ inline int adam_meeting_raised(bool finite, const int32_t* const* __restrict__ meeting_words, int n_meeting_words) {
  int raised = 0;
  if (!finite)
    for (int i = threadIdx.x; i < n_meeting_words; i += blockDim.x)
      if (meeting_words[i] && meeting_words[i][0] != 0) raised = 1;
  return raised;
}
// loss scaling: thread 0's tail of the prep kernel.  state words of `ls` (include/mixstage.h): [0] S, [1] 1/S, [2] consecutive
// finite steps since S last changed, [3] overflow skips, [4] the last step was an overflow skip.  S moves by factors of 2 only:
// every rescaling below is exact.  raw: norm of the SCALED gradients; bad_lr: the learning-rate word cannot be used (false where
// lr is a kernel argument) -- a bad step whatever the gradients are, and not the scale's doing: S and its counters stay
__device__ inline void adam_scaled_tail(int32_t* state, float* norm, float raw, bool finite, bool meeting, bool bad_lr, int step,
                                        float max_norm, int32_t* ls, int growth_interval, float min_scale, float max_scale) {
  float* lf = reinterpret_cast<float*>(ls);
  float S = lf[0];
  const float inv_S = lf[1];
  int good = ls[2];
  state[0] = step;
  const float n = raw * inv_S;
  norm[0] = n;                                     // the caller reads the true norm
  reinterpret_cast<float*>(state)[1] = adam_clip_coef(max_norm, n) * inv_S;
  int skipped = 0;
  if (bad_lr) {
    state[2] = 1;
    state[3] += 1;
  } else if (finite) {
    state[2] = 0;
    if (good < 0x7fffffff) good += 1;
    if (growth_interval > 0 && good >= growth_interval && S < max_scale) { S *= 2.f; good = 0; }
  } else {
    // the update is skipped either way (adam_seg_kernel returns on word 2).  Above the floor it is the scale's doing -- halve it
    // and try again, normal operation; AT the floor, or behind a meeting that timed out, the gradients themselves are not finite: a
    // bad step, counted in word 3 as the unscaled path counts it
    state[2] = 1;
    good = 0;
    if (S > min_scale && !meeting) { S *= 0.5f; ls[3] += 1; skipped = 1; }
    else state[3] += 1;
  }
  lf[0] = S;
  lf[1] = 1.f / S;                                 // (a power of two: exact)
  ls[2] = good;
  ls[4] = skipped;
}

// the loss-scale arguments of the prep kernel: the scale's state words, the rule that moves S, and the table of error words of the
// in-launch meetings (word 0 of a sync buffer; sticky: every later launch on those counters yields NaN).  Empty without a scale
template <bool SCALED>
struct AdamScale {};
template <>
struct AdamScale<true> {
  int32_t* ls;
  int growth_interval;
  float min_scale, max_scale;
  const int32_t* const* meeting_words;
  int n_meeting_words;
};

// Segmented form: torch.optim.Adam keeps one step count PER PARAMETER, started when the parameter first receives a
// gradient, and skips parameters that never had one.  seg_first[s] = global step (1-based) of the segment's first
// gradient, or -1; seg_scratch[2s..2s+1] = (lr/bc1, sqrt(bc2)) of the segment for this step (0,0 = inactive).
// The prep kernel sits on the step's latency chain, the last thing between the backward pass and the next step's first kernel.
// LR_DEV: `lr` is one fp32 word on the device instead of a value; its load is issued at the top, next to state[0], and both loads
// are in flight before the first dependent instruction.  A word that is NaN, infinite, negative or zero refuses the step as a
// non-finite gradient norm does (with or without `norm`).
// SCALED: `norm` holds the norm of the SCALED gradients on entry (thread 0 overwrites it behind the barrier with the true one);
// `scale` are the members of AdamScale<true>, one kernel argument each (the compiler fetches each where it is first needed; a
// struct argument is fetched whole at the top, in front of the load of state[0]); no such arguments without a scale.
template <bool SCALED, bool LR_DEV, typename... Scale>
__global__ void adam_prep_seg_kernel(int32_t* state, std::conditional_t<SCALED, float*, const float*> norm, float max_norm,
                                     std::conditional_t<LR_DEV, const float* __restrict__, float> lr_arg, float beta1, float beta2,
                                     const int32_t* __restrict__ seg_first, float* __restrict__ seg_scratch, int n_seg,
                                     Scale... scale) {
  const AdamScale<SCALED> sc = {scale...};
  float lr;
  if constexpr (LR_DEV) lr = lr_arg[0];
  else lr = lr_arg;
  const int step = state[0] + 1;
  float raw = 0.f;
  bool finite = true;
  int raised = 0;
  if constexpr (SCALED) {
    raw = norm[0];
    finite = adam_norm_finite(raw);
    // a raised error word of a meeting is the cause of a non-finite step, not the scale: a bad step that leaves S where it is, at
    // any scale
    raised = adam_meeting_raised(finite, sc.meeting_words, sc.n_meeting_words);
  }
  for (int sidx = threadIdx.x; sidx < n_seg; sidx += blockDim.x) {
    const int first = seg_first[sidx];
    float ss = 0.f, b2 = 0.f;
    if (first >= 1 && first <= step) {
      const double t = (double)(step - first + 1);
      ss = adam_seg_step_size(lr, beta1, t);
      b2 = adam_seg_bc2(beta2, t);
    }
    seg_scratch[2 * sidx] = ss;
    seg_scratch[2 * sidx + 1] = b2;
  }
  if constexpr (SCALED) {
    const bool meeting = __syncthreads_or(raised) != 0;
    // a bad lr word is a bad step that leaves the loss scale and its counters where they are
    if (threadIdx.x == 0)
      adam_scaled_tail(state, norm, raw, finite, meeting, LR_DEV ? adam_lr_bad(lr) : false, step, max_norm, sc.ls, sc.growth_interval,
                       sc.min_scale, sc.max_scale);
  } else {
    __syncthreads();
    if (threadIdx.x == 0) {
      state[0] = step;
      float coef = 1.f;
      // A non-finite gradient norm (a launch whose in-launch meeting timed out poisons its output with NaN, and the NaN reaches
      // every gradient behind it) must not reach the weights or the moments: the update of this step is SKIPPED on the device --
      // word 2 flags the step, word 3 counts such steps (MixStageTrainStep reads both with the losses); the step clocks advance
      // as if the step had had a zero gradient and frozen moments.
      if constexpr (LR_DEV) {
        bool bad = adam_lr_bad(lr);
        if (norm) {
          coef = adam_clip_coef(max_norm, norm[0]);
          bad = bad || !adam_norm_finite(norm[0]);
        }
        adam_flag_step(state, bad);
      } else if (norm) {                           // (lr by value and no norm: nothing can refuse the step, words 2 and 3 stay)
        coef = adam_clip_coef(max_norm, norm[0]);
        adam_flag_step(state, !adam_norm_finite(norm[0]));
      }
      reinterpret_cast<float*>(state)[1] = coef;
    }
  }
}

// The element pass is written once and instantiated twice: adam_seg_kernel<false> is the pass as it always was (`e` and `om` are
// passed as NULL / 0 and never read: every statement that names them is compiled out), adam_seg_kernel<true> also moves an
// exponential moving average of the weights: e' = fma(om, pn - e, e), om = 1 - decay, one more 16-byte load and store per lane
// next to the seven of the pass.  An element the pass skips (refused step, inactive segment) keeps its `e`.
template <bool EMA>
__global__ __launch_bounds__(256) void adam_seg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, size_t n, const int32_t* __restrict__ state,
                                                       const int32_t* __restrict__ seg_of_chunk,
                                                       const float* __restrict__ seg_scratch, float beta1, float beta2,
                                                       float eps, float* __restrict__ e, float om) {
  const float coef = reinterpret_cast<const float*>(state)[1];
  if (state[2]) return;                        // non-finite gradient norm: no update (adam_prep_seg_kernel)
  // 16 bytes per lane and stream, two vectors per thread in flight (7 streams over the 60 MB of live parameters: dword accesses
  // ran at 5.4 TB/s); a 64-element chunk belongs to one segment, so a vector does too.  n is a multiple of 64 (FlatAdam's layout);
  // the buffers are 256-byte aligned
  // the roundings are spelled out (explicit fma, contraction off): the vector path and the scalar fallback below give the same bits
  // for the same element -- left to the compiler, the fallback rounded the products of mn and vn separately and the vector path did not
  auto upd = [&](float pi, float gr, float mo, float vo, float step_size, float bc2s, float& mn, float& vn) {
#pragma clang fp contract(off)
    const float gi = gr * coef;
    mn = fmaf(1.f - beta1, fmaf(gr, coef, -mo), mo);
    vn = fmaf(beta2, vo, gi * ((1.f - beta2) * gi));
    return fmaf(-step_size, mn / (sqrtf(vn) / bc2s + eps), pi);
  };
  // the average: the difference is rounded, then one fma (contraction off, as above: both paths give the same bits)
  auto avg = [&](float pn, float eo) {
#pragma clang fp contract(off)
    const float t = pn - eo;
    return fmaf(om, t, eo);
  };
  if ((n & 3) == 0 && ((((size_t)p | (size_t)g | (size_t)m | (size_t)v | (EMA ? (size_t)e : (size_t)0)) & 15) == 0)) {
    const size_t n4 = n >> 2, stride = (size_t)gridDim.x * 256;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(e);
    for (size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += 2 * stride) {
      float4 pv[2], gv[2], mv[2], vv[2], ev[2];
      float ss[2], bc[2];
      bool on[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const size_t i = i0 + u * stride;
        on[u] = i < n4;
        const int sidx = seg_of_chunk[min(i, n4 - 1) >> 4];
        ss[u] = seg_scratch[2 * sidx]; bc[u] = seg_scratch[2 * sidx + 1];
        on[u] = on[u] && bc[u] != 0.f;         // never received a gradient: torch.optim.Adam skips it
        if (on[u]) {
          pv[u] = p4[i]; gv[u] = g4[i]; mv[u] = m4[i]; vv[u] = v4[i];
          if constexpr (EMA) ev[u] = e4[i];
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (!on[u]) continue;
        const size_t i = i0 + u * stride;
        float4 mn, vn, pn;
        pn.x = upd(pv[u].x, gv[u].x, mv[u].x, vv[u].x, ss[u], bc[u], mn.x, vn.x);
        pn.y = upd(pv[u].y, gv[u].y, mv[u].y, vv[u].y, ss[u], bc[u], mn.y, vn.y);
        pn.z = upd(pv[u].z, gv[u].z, mv[u].z, vv[u].z, ss[u], bc[u], mn.z, vn.z);
        pn.w = upd(pv[u].w, gv[u].w, mv[u].w, vv[u].w, ss[u], bc[u], mn.w, vn.w);
        m4[i] = mn; v4[i] = vn; p4[i] = pn;
        if constexpr (EMA) {
          float4 en;
          en.x = avg(pn.x, ev[u].x); en.y = avg(pn.y, ev[u].y); en.z = avg(pn.z, ev[u].z); en.w = avg(pn.w, ev[u].w);
          e4[i] = en;
        }
      }
    }
    return;
  }
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int sidx = seg_of_chunk[i >> 6];
    const float step_size = seg_scratch[2 * sidx], bc2s = seg_scratch[2 * sidx + 1];
    if (bc2s == 0.f) continue;                 // never received a gradient: torch.optim.Adam skips it
    float mn, vn;
    const float pn = upd(p[i], g[i], m[i], v[i], step_size, bc2s, mn, vn);
    m[i] = mn;
    v[i] = vn;
    p[i] = pn;
    if constexpr (EMA) e[i] = avg(pn, e[i]);
  }
}

// grid of both element passes
static inline int adam_blocks(size_t n) {
  const int blocks = (int)std::min<size_t>((n + 1023) / 1024, 2048);
  return blocks < 1 ? 1 : blocks;
}

// One call of the segmented step as an entry point states it: the arguments every form has, then the form.  who: the entry point,
// for its refusals; lr_word: lr is read from lr_dev; scaled: the gradients carry the loss scale of `sc`; with_ema: the element pass
// also moves `ema`
struct AdamSegArgs {
  const char* who;
  float* p;
  const float* g;
  float *m, *v;
  size_t n;
  float* norm;                                     // (only the scaled forms write through it)
  float max_norm, beta1, beta2, eps;
  int32_t* step_state;
  const int32_t *seg_of_chunk, *seg_first;
  float* seg_scratch;
  int n_seg;
  float lr = 0.f;
  bool lr_word = false;
  const float* lr_dev = nullptr;
  bool scaled = false;
  AdamScale<true> sc = {};
  bool with_ema = false;
  float* ema = nullptr;
  float ema_decay = 0.f;
};

template <bool SCALED, bool LR_DEV>
static int adam_prep_seg(const AdamSegArgs& a, hipStream_t s) {
  std::conditional_t<LR_DEV, const float*, float> lr;
  if constexpr (LR_DEV) lr = a.lr_dev;
  else lr = a.lr;
  if constexpr (SCALED)
    hipLaunchKernelGGL((adam_prep_seg_kernel<true, LR_DEV>), dim3(1), dim3(256), 0, s, a.step_state, a.norm, a.max_norm, lr, a.beta1,
                       a.beta2, a.seg_first, a.seg_scratch, a.n_seg, a.sc.ls, a.sc.growth_interval, a.sc.min_scale, a.sc.max_scale,
                       a.sc.meeting_words, a.sc.n_meeting_words);
  else
    hipLaunchKernelGGL((adam_prep_seg_kernel<false, LR_DEV>), dim3(1), dim3(256), 0, s, a.step_state, a.norm, a.max_norm, lr, a.beta1,
                       a.beta2, a.seg_first, a.seg_scratch, a.n_seg);
  // (one name per form: an error message tells the four apart)
  return check_launch(SCALED ? (LR_DEV ? "adam_prep_seg_scaled_lr_kernel" : "adam_prep_seg_scaled_kernel")
                             : (LR_DEV ? "adam_prep_seg_lr_kernel" : "adam_prep_seg_kernel"));
}

// every entry point of the segmented step: the refusals (nothing is launched or written), the prep kernel of the form, the element pass
static int adam_segmented(const AdamSegArgs& a, hipStream_t s) {
  if (a.with_ema) {
    if (!a.ema) return set_error("%s: ema is required (n fp32 values, the layout of p)", a.who);
    if (!(a.ema_decay >= 0.f && a.ema_decay < 1.f)) return set_error("%s: ema_decay must be finite and in [0, 1)", a.who);
  }
  if (a.lr_word && !a.lr_dev) return set_error("%s: lr_dev is required (one fp32 word on the device)", a.who);
  if (a.scaled) {
    // (the EMA entry point takes its form from the pointers it is given: its scaled form is the one WITH loss_scale_state)
    if (!a.norm || !a.sc.ls)
      return set_error(a.with_ema ? "%s: the scaled form needs norm" : "%s: norm and loss_scale_state are required", a.who);
    if (!(a.sc.min_scale > 0.f) || !(a.sc.max_scale >= a.sc.min_scale)) return set_error("%s: 0 < min_scale <= max_scale", a.who);
    if (a.sc.n_meeting_words < 0 || (a.sc.n_meeting_words > 0 && !a.sc.meeting_words)) return set_error("%s: meeting_words table", a.who);
  }
  TimingScope ts(s, 0, 0, "ew|ew_adam_step_segmented");
  if (ts.skip()) return 0;
  const int rc = a.scaled ? (a.lr_word ? adam_prep_seg<true, true>(a, s) : adam_prep_seg<true, false>(a, s))
                          : (a.lr_word ? adam_prep_seg<false, true>(a, s) : adam_prep_seg<false, false>(a, s));
  if (rc) return rc;
  const int blocks = adam_blocks(a.n);
  if (a.with_ema) {
    // om = 1.0f - decay is exact for decay >= 0.5 (Sterbenz); below that it is one rounding of a constant
    hipLaunchKernelGGL(adam_seg_kernel<true>, dim3(blocks), dim3(256), 0, s, a.p, a.g, a.m, a.v, a.n, a.step_state, a.seg_of_chunk,
                       a.seg_scratch, a.beta1, a.beta2, a.eps, a.ema, 1.0f - a.ema_decay);
    return check_launch("adam_seg_kernel<ema>");
  }
  hipLaunchKernelGGL(adam_seg_kernel<false>, dim3(blocks), dim3(256), 0, s, a.p, a.g, a.m, a.v, a.n, a.step_state, a.seg_of_chunk,
                     a.seg_scratch, a.beta1, a.beta2, a.eps, (float*)nullptr, 0.f);
  return check_launch("adam_seg_kernel");
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_adam_step(float* p, const float* g, float* m, float* v, size_t n, const float* norm, float max_norm, float lr,
                 float beta1, float beta2, float eps, int32_t* step_state, void* stream) {
  TimingScope ts((hipStream_t)stream, 0, 0, "ew|ew_adam_step");
  if (ts.skip()) return 0;
  hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_state, norm, max_norm, lr, beta1, beta2);
  int rc = check_launch("adam_prep_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(adam_kernel, dim3(adam_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, step_state, beta1, beta2, eps);
  return check_launch("adam_kernel");
}

// The entry points of the segmented step pack their arguments.  The form is fixed by the entry point, except for _ema, which takes
// it from lr_dev and loss_scale_state (NULL: by value / unscaled)
int ms_adam_step_segmented(float* p, const float* g, float* m, float* v, size_t n, const float* norm, float max_norm, float lr,
                           float beta1, float beta2, float eps, int32_t* step_state, const int32_t* seg_of_chunk,
                           const int32_t* seg_first_step, float* seg_scratch, int n_seg, void* stream) {
  AdamSegArgs a = {"ms_adam_step_segmented", p, g, m, v, n, const_cast<float*>(norm), max_norm, beta1, beta2, eps, step_state,
                   seg_of_chunk, seg_first_step, seg_scratch, n_seg};
  a.lr = lr;
  return adam_segmented(a, (hipStream_t)stream);
}

int ms_adam_step_segmented_scaled(float* p, const float* g, float* m, float* v, size_t n, float* norm, float max_norm, float lr,
                                  float beta1, float beta2, float eps, int32_t* step_state, const int32_t* seg_of_chunk,
                                  const int32_t* seg_first_step, float* seg_scratch, int n_seg, int32_t* loss_scale_state,
                                  int32_t growth_interval, float min_scale, float max_scale,
                                  const int32_t* const* meeting_words, int n_meeting_words, void* stream) {
  AdamSegArgs a = {"ms_adam_step_segmented_scaled", p, g, m, v, n, norm, max_norm, beta1, beta2, eps, step_state,
                   seg_of_chunk, seg_first_step, seg_scratch, n_seg};
  a.lr = lr;
  a.scaled = true;
  a.sc = {loss_scale_state, (int)growth_interval, min_scale, max_scale, meeting_words, n_meeting_words};
  return adam_segmented(a, (hipStream_t)stream);
}

int ms_adam_step_segmented_lr(float* p, const float* g, float* m, float* v, size_t n, const float* norm, float max_norm,
                              const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_state,
                              const int32_t* seg_of_chunk, const int32_t* seg_first_step, float* seg_scratch, int n_seg, void* stream) {
  AdamSegArgs a = {"ms_adam_step_segmented_lr", p, g, m, v, n, const_cast<float*>(norm), max_norm, beta1, beta2, eps, step_state,
                   seg_of_chunk, seg_first_step, seg_scratch, n_seg};
  a.lr_word = true;
  a.lr_dev = lr_dev;
  return adam_segmented(a, (hipStream_t)stream);
}

int ms_adam_step_segmented_scaled_lr(float* p, const float* g, float* m, float* v, size_t n, float* norm, float max_norm,
                                     const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_state,
                                     const int32_t* seg_of_chunk, const int32_t* seg_first_step, float* seg_scratch, int n_seg,
                                     int32_t* loss_scale_state, int32_t growth_interval, float min_scale, float max_scale,
                                     const int32_t* const* meeting_words, int n_meeting_words, void* stream) {
  AdamSegArgs a = {"ms_adam_step_segmented_scaled_lr", p, g, m, v, n, norm, max_norm, beta1, beta2, eps, step_state,
                   seg_of_chunk, seg_first_step, seg_scratch, n_seg};
  a.lr_word = true;
  a.lr_dev = lr_dev;
  a.scaled = true;
  a.sc = {loss_scale_state, (int)growth_interval, min_scale, max_scale, meeting_words, n_meeting_words};
  return adam_segmented(a, (hipStream_t)stream);
}

int ms_adam_step_segmented_ema(float* p, const float* g, float* m, float* v, size_t n, float* norm, float max_norm, float lr,
                               const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_state,
                               const int32_t* seg_of_chunk, const int32_t* seg_first_step, float* seg_scratch, int n_seg,
                               int32_t* loss_scale_state, int32_t growth_interval, float min_scale, float max_scale,
                               const int32_t* const* meeting_words, int n_meeting_words, float* ema, float ema_decay, void* stream) {
  AdamSegArgs a = {"ms_adam_step_segmented_ema", p, g, m, v, n, norm, max_norm, beta1, beta2, eps, step_state,
                   seg_of_chunk, seg_first_step, seg_scratch, n_seg};
  a.lr = lr;
  a.lr_word = lr_dev != nullptr;
  a.lr_dev = lr_dev;
  a.scaled = loss_scale_state != nullptr;
  a.sc = {loss_scale_state, (int)growth_interval, min_scale, max_scale, meeting_words, n_meeting_words};
  a.with_ema = true;
  a.ema = ema;
  a.ema_decay = ema_decay;
  return adam_segmented(a, (hipStream_t)stream);
}

}  // extern "C"
