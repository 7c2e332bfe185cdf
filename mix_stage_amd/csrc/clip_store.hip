// Device-resident clip store: the batch itself drawn on the device.  The raw frames of a whole speaker set stay in HBM as
// two row stores, pose_rows (R, P) and audio_rows (R, F); one launch picks this step's B windows from the epoch's order, gathers them
// and runs the pre-step on them (the labels of ms_kmeans_labels, the z-norm of ms_znorm_select -- km_nearest_wave and znorm_value of
// prestep_feat.h, so the bits are those of DevicePreStep on the gathered clips by construction), writing straight into the caller's
// buffers -- the static inputs of a captured training step.  A second, one-thread launch moves the cursor, so a replayed graph walks
// through the epoch without the host.
//   one wave per frame (b, t): clip b = window order[cursor + rank * B + b], its frame t = store row win_row[window] + t
//   velocity  t is the frame WITHIN THE WINDOW: at t == 0 the velocity is 0 although the interval's previous row sits right in front
//             of the window in the store (km_velocity reads xr[col - P] for t > 0 only)
//   offsets   the stores are larger than 2 GiB (and than the 4 GiB a 32-bit byte offset reaches): rows are addressed as
//             base + (size_t)row * width from plain global pointers, no buffer descriptor
//   guard     a position >= n_order, an order entry outside [0, W) or a window outside [0, R) is "no window": the clip is zeros with
//             label 0, style 0, index -1, state word 0 goes up, and nothing is read through the entry
// Rows whose width is a multiple of 4 floats (P = 104, PK = 96, F = 128) move as 16-byte accesses; any other width takes the scalar loop.
#include <stdint.h>

#include "kernels.h"
#include "prestep_feat.h"

namespace ms {

enum { CLIP_VEC_AUDIO = 1, CLIP_VEC_Y = 2, CLIP_VEC_FULL = 4 };

struct ClipDrawArgs {
  const float *pose_rows, *audio_rows;
  const int64_t* win_row;
  const int32_t *win_style, *order, *keep;
  int32_t* state;
  const double *centers, *pose_mean, *pose_inv, *audio_mean, *audio_inv;
  float *audio, *y, *full;
  int64_t *labels, *style;
  int32_t* indices;
  int64_t R;
  int W, n_order, B, T, rank, M, feats, P, PK, F, vec;
};

// out[d] = znorm(xr[keep ? keep[d] : d]) for d < n, by one wave.  VEC: n % 4 == 0 and the rows are 16-byte aligned -- four columns
// per lane, one 16-byte store (and, without keep, one 16-byte load); the values are those of the scalar loop.
__device__ __forceinline__ void clip_znorm_row(const float* __restrict__ xr, const int32_t* __restrict__ keep, const double* __restrict__ mean,
                                               const double* __restrict__ inv, float* __restrict__ out, int n, int lane, bool vec) {
  if (vec) {
    for (int d = lane * 4; d < n; d += 256) {
      int c[4];
      float x[4];
      if (keep) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { c[k] = keep[d + k]; x[k] = xr[c[k]]; }
      } else {
        const float4 v = *reinterpret_cast<const float4*>(xr + d);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = d + k;
      }
      float4 o;
      o.x = znorm_value(x[0], mean[c[0]], inv[c[0]]);
      o.y = znorm_value(x[1], mean[c[1]], inv[c[1]]);
      o.z = znorm_value(x[2], mean[c[2]], inv[c[2]]);
      o.w = znorm_value(x[3], mean[c[3]], inv[c[3]]);
      *reinterpret_cast<float4*>(out + d) = o;
    }
    return;
  }
  for (int d = lane; d < n; d += 64) {          // scalar tail path: any width, any alignment
    const int col = keep ? keep[d] : d;
    out[d] = znorm_value(xr[col], mean[col], inv[col]);
  }
}

__global__ __launch_bounds__(256) void clip_draw_kernel(const ClipDrawArgs a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);          // frame (b, t) of the batch: one wave
  if (r >= a.B * a.T) return;
  const int b = r / a.T, t = r - b * a.T;
  // the window: every step of the way is checked before the next index is used (wave-uniform: all lanes take the same branch)
  const int64_t pos = (int64_t)a.state[1] + (int64_t)a.rank * a.B + b;
  int w = -1;
  int64_t row0 = 0;
  if (pos >= 0 && pos < (int64_t)a.n_order) {
    w = a.order[pos];
    if (w >= a.W) w = -1;
  }
  if (w >= 0) {
    row0 = a.win_row[w];
    if (row0 < 0 || row0 + (int64_t)a.T > a.R) w = -1;
  }
  float* ao = a.audio + (size_t)r * a.F;
  float* yo = a.y + (size_t)r * a.PK;
  float* fo = a.full ? a.full + (size_t)r * a.P : nullptr;
  if (w < 0) {                                                // no window: zeros, and the sticky flag
    for (int d = lane; d < a.F; d += 64) ao[d] = 0.f;
    for (int d = lane; d < a.PK; d += 64) yo[d] = 0.f;
    if (fo) for (int d = lane; d < a.P; d += 64) fo[d] = 0.f;
    if (lane == 0) {
      a.labels[r] = 0;
      a.style[r] = 0;
      if (t == 0) { a.indices[b] = -1; a.state[0] = 1; }
    }
    return;
  }
  const size_t row = (size_t)row0 + (size_t)t;                // 64-bit: row * P * 4 passes 2^32 in a large store
  const float* xr = a.pose_rows + row * (size_t)a.P;
  const float* ar = a.audio_rows + row * (size_t)a.F;
  const KMFeat f(a.feats, a.PK);
  double bestd;
  const int best = km_nearest_wave(f, xr, a.keep, a.centers, a.M, lane, t, a.P, a.PK, &bestd);
  clip_znorm_row(ar, nullptr, a.audio_mean, a.audio_inv, ao, a.F, lane, a.vec & CLIP_VEC_AUDIO);
  clip_znorm_row(xr, a.keep, a.pose_mean, a.pose_inv, yo, a.PK, lane, a.vec & CLIP_VEC_Y);
  if (fo) clip_znorm_row(xr, nullptr, a.pose_mean, a.pose_inv, fo, a.P, lane, a.vec & CLIP_VEC_FULL);
  if (lane == 0) {
    a.labels[r] = best;
    a.style[r] = (int64_t)a.win_style[w];
    if (t == 0) a.indices[b] = w;
  }
}

// the cursor moves once per draw (one thread, stream-ordered behind the draw's reads: eager or captured)
__global__ void clip_advance_kernel(int32_t* state, int step) {
  if (blockIdx.x == 0 && threadIdx.x == 0) state[1] = (int32_t)((uint32_t)state[1] + (uint32_t)step);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace ms

using namespace ms;

extern "C" {

int ms_clip_draw(const float* pose_rows, const float* audio_rows, int64_t R, const int64_t* win_row, const int32_t* win_style, int W,
                 const int32_t* order, int n_order, int32_t* state, int B, int T, int rank, int world, const int32_t* keep,
                 const double* centers, int M, int feats, const double* pose_mean, const double* pose_inv_std, const double* audio_mean,
                 const double* audio_inv_std, int P, int PK, int F, float* audio, int64_t* labels, float* y, int64_t* style,
                 float* pose_full_norm, int32_t* indices, void* stream) {
  if (!pose_rows || !audio_rows || !win_row || !win_style || !order || !state || !keep || !centers || !pose_mean || !pose_inv_std ||
      !audio_mean || !audio_inv_std || !audio || !labels || !y || !style || !indices)
    return set_error("ms_clip_draw: a NULL tensor");
  if (B < 1 || T < 1 || P < 1 || PK < 1 || PK > P || F < 1 || M < 1 || R < 0 || W < 0 || n_order < 0)
    return set_error("ms_clip_draw: B=%d T=%d P=%d PK=%d F=%d M=%d R=%lld W=%d n_order=%d", B, T, P, PK, F, M, (long long)R, W, n_order);
  if (world < 1 || rank < 0 || rank >= world) return set_error("ms_clip_draw: rank %d of world %d", rank, world);
  if (!(feats & 7) || (feats & ~7) || ((feats & 4) && (PK & 1))) return set_error("ms_clip_draw: feats must be a subset of pose|velocity|speed (1|2|4)");
  if ((long long)B * T * (P > F ? P : F) > 0x7fffffffLL || (long long)rank * B + B > 0x7fffffffLL)
    return set_error("ms_clip_draw: B=%d T=%d is beyond the batch's index range (2^31 values per output)", B, T);
  ClipDrawArgs a;
  a.pose_rows = pose_rows; a.audio_rows = audio_rows; a.win_row = win_row; a.win_style = win_style; a.order = order; a.keep = keep;
  a.state = state; a.centers = centers; a.pose_mean = pose_mean; a.pose_inv = pose_inv_std; a.audio_mean = audio_mean; a.audio_inv = audio_inv_std;
  a.audio = audio; a.y = y; a.full = pose_full_norm; a.labels = labels; a.style = style; a.indices = indices;
  a.R = R; a.W = W; a.n_order = n_order; a.B = B; a.T = T; a.rank = rank; a.M = M; a.feats = feats; a.P = P; a.PK = PK; a.F = F;
  a.vec = 0;
  if (F % 4 == 0 && aligned16(audio_rows) && aligned16(audio)) a.vec |= CLIP_VEC_AUDIO;
  if (PK % 4 == 0 && aligned16(y)) a.vec |= CLIP_VEC_Y;
  if (P % 4 == 0 && pose_full_norm && aligned16(pose_rows) && aligned16(pose_full_norm)) a.vec |= CLIP_VEC_FULL;
  hipLaunchKernelGGL(clip_draw_kernel, dim3(cdiv(B * T, 4)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("clip_draw_kernel");
}

int ms_clip_advance(int32_t* state, int step, void* stream) {
  if (!state) return set_error("ms_clip_advance: the store's state is NULL");
  if (step < 0) return set_error("ms_clip_advance: step %d", step);
  hipLaunchKernelGGL(clip_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, step);
  return check_launch("clip_advance_kernel");
}

}  // extern "C"
