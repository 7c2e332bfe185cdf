// Dynamic loss scaling for fp16 training, on the device: the tail of a step whose backward pass was seeded with the scale S
// instead of 1.  One prep launch un-scales the gradient norm, folds 1/S into the clip coefficient the element pass multiplies
// every gradient with anyway (no extra pass over the gradients), decides whether the step is applied, and moves S -- so a
// captured step follows the scale from replay to replay: the prep kernel at the end of step k writes the word the loss kernels
// of step k+1 read their incoming gradient from.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace ms {

// The per-segment step sizes, the clip coefficient and thread 0's tail (state words of `ls`, the rule that moves S) are device code
// shared with adam_prep_seg_kernel (elementwise.hip) and the twins that read lr from a device word (lr_device.hip): kernels.h.
__global__ void adam_prep_seg_scaled_kernel(int32_t* state, float* norm, float max_norm, float lr, float beta1, float beta2,
                                            const int32_t* __restrict__ seg_first, float* __restrict__ seg_scratch, int n_seg,
                                            int32_t* ls, int growth_interval, float min_scale, float max_scale,
                                            const int32_t* const* __restrict__ meeting_words, int n_meeting_words) {
  const int step = state[0] + 1;
  const float raw = norm[0];                         // norm of the SCALED gradients (thread 0 overwrites it behind the barrier)
  const bool finite = adam_norm_finite(raw);
  // a raised error word of an in-launch meeting (word 0 of a sync buffer; sticky: every later launch on those counters yields NaN)
  // is the cause of a non-finite step, not the scale: a bad step that leaves S where it is, at any scale.  The table is scanned by
  // the whole workgroup, and only when the step is not finite
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
    adam_scaled_tail(state, norm, raw, finite, meeting, false, step, max_norm, ls, growth_interval, min_scale, max_scale);
}

// the prep kernel on its own (ema.hip)
int launch_adam_prep_seg_scaled(int32_t* step_state, float* norm, float max_norm, float lr, float beta1, float beta2,
                                const int32_t* seg_first, float* seg_scratch, int n_seg, int32_t* ls, int growth_interval,
                                float min_scale, float max_scale, const int32_t* const* meeting_words, int n_meeting_words,
                                hipStream_t s) {
  hipLaunchKernelGGL(adam_prep_seg_scaled_kernel, dim3(1), dim3(256), 0, s, step_state, norm, max_norm, lr, beta1, beta2, seg_first,
                     seg_scratch, n_seg, ls, growth_interval, min_scale, max_scale, meeting_words, n_meeting_words);
  return check_launch("adam_prep_seg_scaled_kernel");
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_adam_step_segmented_scaled(float* p, const float* g, float* m, float* v, size_t n, float* norm, float max_norm, float lr,
                                  float beta1, float beta2, float eps, int32_t* step_state, const int32_t* seg_of_chunk,
                                  const int32_t* seg_first_step, float* seg_scratch, int n_seg, int32_t* loss_scale_state,
                                  int32_t growth_interval, float min_scale, float max_scale,
                                  const int32_t* const* meeting_words, int n_meeting_words, void* stream) {
  if (!norm || !loss_scale_state) return set_error("ms_adam_step_segmented_scaled: norm and loss_scale_state are required");
  if (!(min_scale > 0.f) || !(max_scale >= min_scale)) return set_error("ms_adam_step_segmented_scaled: 0 < min_scale <= max_scale");
  if (n_meeting_words < 0 || (n_meeting_words > 0 && !meeting_words)) return set_error("ms_adam_step_segmented_scaled: meeting_words table");
  TimingScope ts((hipStream_t)stream, 0, 0, "ew|ew_adam_step_segmented");
  if (ts.skip()) return 0;
  hipLaunchKernelGGL(adam_prep_seg_scaled_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, step_state, norm, max_norm, lr, beta1,
                     beta2, seg_first_step, seg_scratch, n_seg, loss_scale_state, (int)growth_interval, min_scale, max_scale,
                     meeting_words, n_meeting_words);
  int rc = check_launch("adam_prep_seg_scaled_kernel");
  if (rc) return rc;
  return launch_adam_seg(p, g, m, v, n, step_state, seg_of_chunk, seg_scratch, beta1, beta2, eps, (hipStream_t)stream);
}

}  // extern "C"
