// Dynamic loss scaling for fp16 training, on the device: the tail of a step whose backward pass was seeded with the scale S
// instead of 1.  One prep launch un-scales the gradient norm, folds 1/S into the clip coefficient the element pass multiplies
// every gradient with anyway (no extra pass over the gradients), decides whether the step is applied, and moves S -- so a
// captured step follows the scale from replay to replay: the prep kernel at the end of step k writes the word the loss kernels
// of step k+1 read their incoming gradient from.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace ms {

// state words of `ls` (include/mixstage.h): [0] S, [1] 1/S, [2] consecutive finite steps since S last changed, [3] overflow
// skips, [4] the last step was an overflow skip.  S moves by factors of 2 only: every rescaling below is exact.
// The per-segment step sizes are adam_prep_seg_kernel's (elementwise.hip), same fp64 pow path: same bits.
__global__ void adam_prep_seg_scaled_kernel(int32_t* state, float* norm, float max_norm, float lr, float beta1, float beta2,
                                            const int32_t* __restrict__ seg_first, float* __restrict__ seg_scratch, int n_seg,
                                            int32_t* ls, int growth_interval, float min_scale, float max_scale,
                                            const int32_t* const* __restrict__ meeting_words, int n_meeting_words) {
  const int step = state[0] + 1;
  const float raw = norm[0];                         // norm of the SCALED gradients (thread 0 overwrites it behind the barrier)
  const bool finite = fabsf(raw) <= 3.0e38f;
  // a raised error word of an in-launch meeting (word 0 of a sync buffer; sticky: every later launch on those counters yields NaN)
  // is the cause of a non-finite step, not the scale: a bad step that leaves S where it is, at any scale.  The table is scanned by
  // the whole workgroup, and only when the step is not finite
  int raised = 0;
  if (!finite)
    for (int i = threadIdx.x; i < n_meeting_words; i += blockDim.x)
      if (meeting_words[i] && meeting_words[i][0] != 0) raised = 1;
  for (int sidx = threadIdx.x; sidx < n_seg; sidx += blockDim.x) {
    const int first = seg_first[sidx];
    float ss = 0.f, b2 = 0.f;
    if (first >= 1 && first <= step) {
      const double t = (double)(step - first + 1);
      ss = (float)((double)lr / (1.0 - pow((double)beta1, t)));
      b2 = (float)sqrt(1.0 - pow((double)beta2, t));
    }
    seg_scratch[2 * sidx] = ss;
    seg_scratch[2 * sidx + 1] = b2;
  }
  const bool meeting = __syncthreads_or(raised) != 0;
  if (threadIdx.x == 0) {
    float* lf = reinterpret_cast<float*>(ls);
    float S = lf[0];
    const float inv_S = lf[1];
    int good = ls[2];
    state[0] = step;
    const float n = raw * inv_S;
    norm[0] = n;                                     // the caller reads the true norm
    float coef = max_norm / (n + 1e-6f);
    if (coef > 1.f) coef = 1.f;
    reinterpret_cast<float*>(state)[1] = coef * inv_S;
    int skipped = 0;
    if (finite) {
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
