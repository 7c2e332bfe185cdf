// The learning rate as a device word: the twins of ms_adam_step_segmented (elementwise.hip) and ms_adam_step_segmented_scaled
// (loss_scale.hip) whose prep kernel READS lr when it runs instead of receiving it as a kernel argument.  A step captured into a HIP
// graph then follows a learning-rate schedule from replay to replay (the reference steps ExponentialLR once per epoch, TR:311-313,
// 499-500): the host writes the word between steps, on the stream the replays run on.  One prep launch in place of one prep launch,
// the element pass is launch_adam_seg's: the launch count of a step does not change.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace ms {

// adam_prep_seg_kernel with lr from `lr_dev`.  The load of the word is issued at the top, next to state[0]: the prep kernel sits on
// the step's latency chain, and both loads are in flight before the first dependent instruction.  The step sizes, the clip
// coefficient and the health words are kernels.h's, shared with the by-value kernel: the same bits for the same lr.
// A word that is NaN, infinite, negative or zero refuses the step as a non-finite gradient norm does (with or without `norm`).
__global__ void adam_prep_seg_lr_kernel(int32_t* state, const float* norm, float max_norm, const float* __restrict__ lr_dev,
                                        float beta1, float beta2, const int32_t* __restrict__ seg_first,
                                        float* __restrict__ seg_scratch, int n_seg) {
  const float lr = lr_dev[0];
  const int step = state[0] + 1;
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
  __syncthreads();
  if (threadIdx.x == 0) {
    state[0] = step;
    float coef = 1.f;
    bool bad = adam_lr_bad(lr);
    if (norm) {
      coef = adam_clip_coef(max_norm, norm[0]);
      bad = bad || !adam_norm_finite(norm[0]);
    }
    adam_flag_step(state, bad);
    reinterpret_cast<float*>(state)[1] = coef;
  }
}

// adam_prep_seg_scaled_kernel with lr from `lr_dev`: same order of loads, same shared tail.  A bad lr word is a bad step that leaves
// the loss scale and its counters where they are (adam_scaled_tail).
__global__ void adam_prep_seg_scaled_lr_kernel(int32_t* state, float* norm, float max_norm, const float* __restrict__ lr_dev,
                                               float beta1, float beta2, const int32_t* __restrict__ seg_first,
                                               float* __restrict__ seg_scratch, int n_seg, int32_t* ls, int growth_interval,
                                               float min_scale, float max_scale,
                                               const int32_t* const* __restrict__ meeting_words, int n_meeting_words) {
  const float lr = lr_dev[0];
  const int step = state[0] + 1;
  const float raw = norm[0];                         // norm of the SCALED gradients (thread 0 overwrites it behind the barrier)
  const bool finite = adam_norm_finite(raw);
  const int raised = adam_meeting_raised(finite, meeting_words, n_meeting_words);
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
  const bool meeting = __syncthreads_or(raised) != 0;
  if (threadIdx.x == 0)
    adam_scaled_tail(state, norm, raw, finite, meeting, adam_lr_bad(lr), step, max_norm, ls, growth_interval, min_scale, max_scale);
}

// the two prep kernels on their own (ema.hip)
int launch_adam_prep_seg_lr(int32_t* step_state, const float* norm, float max_norm, const float* lr_dev, float beta1, float beta2,
                            const int32_t* seg_first, float* seg_scratch, int n_seg, hipStream_t s) {
  hipLaunchKernelGGL(adam_prep_seg_lr_kernel, dim3(1), dim3(256), 0, s, step_state, norm, max_norm, lr_dev, beta1, beta2, seg_first,
                     seg_scratch, n_seg);
  return check_launch("adam_prep_seg_lr_kernel");
}

int launch_adam_prep_seg_scaled_lr(int32_t* step_state, float* norm, float max_norm, const float* lr_dev, float beta1, float beta2,
                                   const int32_t* seg_first, float* seg_scratch, int n_seg, int32_t* ls, int growth_interval,
                                   float min_scale, float max_scale, const int32_t* const* meeting_words, int n_meeting_words,
                                   hipStream_t s) {
  hipLaunchKernelGGL(adam_prep_seg_scaled_lr_kernel, dim3(1), dim3(256), 0, s, step_state, norm, max_norm, lr_dev, beta1, beta2, seg_first,
                     seg_scratch, n_seg, ls, growth_interval, min_scale, max_scale, meeting_words, n_meeting_words);
  return check_launch("adam_prep_seg_scaled_lr_kernel");
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_adam_step_segmented_lr(float* p, const float* g, float* m, float* v, size_t n, const float* norm, float max_norm,
                              const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_state,
                              const int32_t* seg_of_chunk, const int32_t* seg_first_step, float* seg_scratch, int n_seg, void* stream) {
  if (!lr_dev) return set_error("ms_adam_step_segmented_lr: lr_dev is required (one fp32 word on the device)");
  TimingScope ts((hipStream_t)stream, 0, 0, "ew|ew_adam_step_segmented");
  if (ts.skip()) return 0;
  hipLaunchKernelGGL(adam_prep_seg_lr_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, step_state, norm, max_norm, lr_dev, beta1,
                     beta2, seg_first_step, seg_scratch, n_seg);
  int rc = check_launch("adam_prep_seg_lr_kernel");
  if (rc) return rc;
  return launch_adam_seg(p, g, m, v, n, step_state, seg_of_chunk, seg_scratch, beta1, beta2, eps, (hipStream_t)stream);
}

int ms_adam_step_segmented_scaled_lr(float* p, const float* g, float* m, float* v, size_t n, float* norm, float max_norm,
                                     const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_state,
                                     const int32_t* seg_of_chunk, const int32_t* seg_first_step, float* seg_scratch, int n_seg,
                                     int32_t* loss_scale_state, int32_t growth_interval, float min_scale, float max_scale,
                                     const int32_t* const* meeting_words, int n_meeting_words, void* stream) {
  if (!lr_dev) return set_error("ms_adam_step_segmented_scaled_lr: lr_dev is required (one fp32 word on the device)");
  if (!norm || !loss_scale_state) return set_error("ms_adam_step_segmented_scaled_lr: norm and loss_scale_state are required");
  if (!(min_scale > 0.f) || !(max_scale >= min_scale)) return set_error("ms_adam_step_segmented_scaled_lr: 0 < min_scale <= max_scale");
  if (n_meeting_words < 0 || (n_meeting_words > 0 && !meeting_words)) return set_error("ms_adam_step_segmented_scaled_lr: meeting_words table");
  TimingScope ts((hipStream_t)stream, 0, 0, "ew|ew_adam_step_segmented");
  if (ts.skip()) return 0;
  hipLaunchKernelGGL(adam_prep_seg_scaled_lr_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, step_state, norm, max_norm, lr_dev,
                     beta1, beta2, seg_first_step, seg_scratch, n_seg, loss_scale_state, (int)growth_interval, min_scale, max_scale,
                     meeting_words, n_meeting_words);
  int rc = check_launch("adam_prep_seg_scaled_lr_kernel");
  if (rc) return rc;
  return launch_adam_seg(p, g, m, v, n, step_state, seg_of_chunk, seg_scratch, beta1, beta2, eps, (hipStream_t)stream);
}

}  // extern "C"
