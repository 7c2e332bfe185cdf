// An exponential moving average (EMA) of the weights inside the segmented Adam step: ONE entry point for the four forms of the step
// (lr by value or from a device word, with or without dynamic loss scaling).  It launches the unchanged prep kernel of the form
// (elementwise.hip, lr_device.hip, loss_scale.hip) and the EMA instance of the element pass (elementwise.hip: adam_seg_kernel<true>),
// which reads and writes `ema` next to p, m and v: two launches, as every other form, and no extra pass over the parameters.
// An element the pass leaves alone -- a refused step (step_state word 2: non-finite norm, overflow skip, bad lr word), a segment
// that never had a gradient or whose first step is still ahead -- keeps its average.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.h"

using namespace ms;

extern "C" {

int ms_adam_step_segmented_ema(float* p, const float* g, float* m, float* v, size_t n, float* norm, float max_norm, float lr,
                               const float* lr_dev, float beta1, float beta2, float eps, int32_t* step_state,
                               const int32_t* seg_of_chunk, const int32_t* seg_first_step, float* seg_scratch, int n_seg,
                               int32_t* loss_scale_state, int32_t growth_interval, float min_scale, float max_scale,
                               const int32_t* const* meeting_words, int n_meeting_words, float* ema, float ema_decay, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ema) return set_error("ms_adam_step_segmented_ema: ema is required (n fp32 values, the layout of p)");
  if (!(ema_decay >= 0.f && ema_decay < 1.f)) return set_error("ms_adam_step_segmented_ema: ema_decay must be finite and in [0, 1)");
  if (loss_scale_state) {
    if (!norm) return set_error("ms_adam_step_segmented_ema: the scaled form needs norm");
    if (!(min_scale > 0.f) || !(max_scale >= min_scale)) return set_error("ms_adam_step_segmented_ema: 0 < min_scale <= max_scale");
    if (n_meeting_words < 0 || (n_meeting_words > 0 && !meeting_words)) return set_error("ms_adam_step_segmented_ema: meeting_words table");
  }
  TimingScope ts(s, 0, 0, "ew|ew_adam_step_segmented");
  if (ts.skip()) return 0;
  int rc;
  if (loss_scale_state && lr_dev)
    rc = launch_adam_prep_seg_scaled_lr(step_state, norm, max_norm, lr_dev, beta1, beta2, seg_first_step, seg_scratch, n_seg,
                                        loss_scale_state, (int)growth_interval, min_scale, max_scale, meeting_words, n_meeting_words, s);
  else if (loss_scale_state)
    rc = launch_adam_prep_seg_scaled(step_state, norm, max_norm, lr, beta1, beta2, seg_first_step, seg_scratch, n_seg, loss_scale_state,
                                     (int)growth_interval, min_scale, max_scale, meeting_words, n_meeting_words, s);
  else if (lr_dev)
    rc = launch_adam_prep_seg_lr(step_state, norm, max_norm, lr_dev, beta1, beta2, seg_first_step, seg_scratch, n_seg, s);
  else
    rc = launch_adam_prep_seg(step_state, norm, max_norm, lr, beta1, beta2, seg_first_step, seg_scratch, n_seg, s);
  if (rc) return rc;
  // 1.0f - decay is exact for decay >= 0.5 (Sterbenz); below that it is one rounding of a constant
  return launch_adam_seg_ema(p, g, m, v, n, step_state, seg_of_chunk, seg_scratch, beta1, beta2, eps, ema, 1.0f - ema_decay, s);
}

}  // extern "C"
