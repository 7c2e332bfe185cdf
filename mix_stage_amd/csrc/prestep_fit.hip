// Fitting what the pre-step consumes, on device: Lloyd iterations of KMeans.fit (transform.py:247-427, sklearn on the CPU in the
// reference) and the statistics pass of ZNorm (transform.py:99-244).  Everything in fp64; every reduction in a fixed order, no
// floating-point atomics, no workgroup waits for another: a workgroup owns a contiguous slice of rows, writes its partials to
// the workspace, and a second small launch folds them into the running state in workgroup order.  The feature row and the
// distance arithmetic are those of ms_kmeans_labels (prestep_feat.h).
#include <algorithm>

#include <stdint.h>

#include "kernels.h"
#include "prestep_feat.h"

namespace ms {

constexpr int FIT_ROUND = 32;          // rows labelled (one wave per row, 8 per wave) before the 256 threads add them up
constexpr int FIT_PRE = 8;             // rows in flight per thread in the adding phase
constexpr int FIT_SLICE_MIN = 64;      // rows a workgroup takes at least
constexpr int FIT_MAX_WGS = 2048;      // partial records per launch at most
constexpr int FIT_LDS_MAX = 160 * 1024;
constexpr int STATS_SLICE_MIN = 256;
constexpr int STATS_MAX_WGS = 1024;
constexpr double FIT_MAX_ROWS = 1073741824.0;   // 2^30: row indices and r * P stay clear of 2^31 / 2^63

// how a launch cuts `rows` rows into slices: nwg workgroups of `per` rows (the last ones may be short or empty)
struct Slices { int nwg; long long per; };
static Slices slices_of(long long rows, int slice_min, int max_wgs) {
  Slices s;
  s.nwg = (int)std::min<long long>(max_wgs, (rows + slice_min - 1) / slice_min);
  if (s.nwg < 1) s.nwg = 1;
  s.per = (rows + s.nwg - 1) / s.nwg;
  return s;
}

// state / partial record of the Lloyd pass: sums[M][W] | counts[M] | inertia | changed
static size_t fit_record_elems(int M, int W) { return (size_t)M * W + M + 2; }
// LDS of a workgroup: sums and counts as [M][W + 1] doubles, 4 wave inertias, then the round's labels and frame indices and 4
// wave counters as int32
static size_t fit_lds_bytes(int M, int W) { return ((size_t)M * (W + 1) + 4) * sizeof(double) + (2 * FIT_ROUND + 4) * sizeof(int32_t); }

// ----------------------------------------------------------------------------------------------
// Lloyd assignment and partial sums.  Per round of FIT_ROUND rows: wave w labels rows w, w + 4, ... (km_nearest_wave: the
// arithmetic of kmeans_labels_kernel); then thread j adds column j of every row of the round, in row order, into the LDS sum of
// that row's cluster (column W is the count) -- one thread owns a column of the M x (W + 1) block, so nothing races.
__global__ __launch_bounds__(256) void kmeans_fit_accumulate_kernel(const float* __restrict__ pose, const int32_t* __restrict__ keep,
                                                                    const double* __restrict__ centers, int64_t* __restrict__ labels,
                                                                    double* __restrict__ partials, int BT, int T, int P, int PK, int M,
                                                                    int feats, int rows_per_wg) {
  extern __shared__ double sh[];
  const KMFeat f(feats, PK);
  const int W = f.D, W1 = W + 1;
  double* sums = sh;
  double* w_inertia = sh + (size_t)M * W1;
  int32_t* r_label = reinterpret_cast<int32_t*>(w_inertia + 4);
  int32_t* r_t = r_label + FIT_ROUND;
  int32_t* w_changed = r_t + FIT_ROUND;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int e = tid; e < M * W1; e += 256) sums[e] = 0.0;
  __syncthreads();
  const long long r0l = (long long)blockIdx.x * rows_per_wg;
  const int r0 = (int)std::min<long long>(r0l, BT), r1 = (int)std::min<long long>(r0l + rows_per_wg, BT);
  double inertia = 0.0;
  int changed = 0;
  for (int base = r0; base < r1; base += FIT_ROUND) {
    const int n = min(FIT_ROUND, r1 - base);
    for (int i = wv; i < n; i += 4) {
      const int r = base + i, t = r % T;
      double bestd;
      const int best = km_nearest_wave(f, pose + (size_t)r * P, keep, centers, M, lane, t, P, PK, &bestd);
      if (lane == 0) {
        r_label[i] = best;
        r_t[i] = t;
        changed += labels[r] != (int64_t)best;
        labels[r] = best;
        inertia += bestd;
      }
    }
    __syncthreads();
    // (FIT_PRE rows' labels and elements are loaded before the first of their LDS additions: a store to `sums` would otherwise
    // stand between every two loads, and a round would be a chain of FIT_ROUND trips to the L2)
    for (int j = tid; j < W1; j += 256)
      for (int i0 = 0; i0 < n; i0 += FIT_PRE) {
        double v[FIT_PRE];
        int lab[FIT_PRE];
#pragma unroll
        for (int u = 0; u < FIT_PRE; ++u) {
          const int i = min(i0 + u, n - 1);
          lab[u] = r_label[i];
          v[u] = j < W ? km_feature(f, pose + (size_t)(base + i) * P, keep, j, r_t[i], P, PK) : 1.0;
        }
#pragma unroll
        for (int u = 0; u < FIT_PRE; ++u)
          if (i0 + u < n) sums[lab[u] * W1 + j] += v[u];          // row order: the sum's definition
      }
    __syncthreads();
  }
  if (lane == 0) { w_inertia[wv] = inertia; w_changed[wv] = changed; }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ((size_t)M * W + M + 2);
  for (int e = tid; e < M * W; e += 256) {
    const int m = e / W;
    out[e] = sums[m * W1 + (e - m * W)];
  }
  for (int m = tid; m < M; m += 256) out[(size_t)M * W + m] = sums[m * W1 + W];
  if (tid == 0) {
    out[(size_t)M * W + M] = (w_inertia[0] + w_inertia[1]) + (w_inertia[2] + w_inertia[3]);
    out[(size_t)M * W + M + 1] = (double)((w_changed[0] + w_changed[1]) + (w_changed[2] + w_changed[3]));
  }
}

// state[e] += partials[0][e] + partials[1][e] + ..., left to right
__global__ __launch_bounds__(256) void fit_fold_kernel(const double* __restrict__ partials, double* __restrict__ state, int n_rec, int elems) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  double s = state[e];
  for (int g = 0; g < n_rec; ++g) s += partials[(size_t)g * elems + e];
  state[e] = s;
}

// centres_out[m] = sums[m] / counts[m], an empty cluster keeps centres_in[m]; out4 = shift | empties | inertia | changed
__global__ __launch_bounds__(256) void kmeans_fit_update_kernel(const double* __restrict__ state, const double* __restrict__ cin,
                                                                double* __restrict__ cout, double* __restrict__ out4, int M, int W) {
  __shared__ double red[4];
  const double* counts = state + (size_t)M * W;
  double shift = 0.0;
  for (int e = threadIdx.x; e < M * W; e += 256) {
    const double n = counts[e / W], old = cin[e];
    const double c = n > 0.0 ? state[e] / n : old;
    cout[e] = c;
    shift += (c - old) * (c - old);
  }
  shift = block_sum_256(shift, red);
  if (threadIdx.x == 0) {
    int empties = 0;
    for (int m = 0; m < M; ++m) empties += counts[m] == 0.0;
    out4[0] = shift;
    out4[1] = (double)empties;
    out4[2] = counts[M];
    out4[3] = counts[M + 1];
  }
}

// ----------------------------------------------------------------------------------------------
// ZNorm statistics.  A workgroup's slice of rows, per column: two-pass (mean, M2 about that mean) in fp64.  Column blocks of up
// to 256 columns; with C < 256 the threads split into 256 / C row lanes whose partial sums meet in LDS, lane order.
__global__ __launch_bounds__(256) void column_stats_tile_kernel(const float* __restrict__ x, long long rows, int C, long long rows_per_wg,
                                                                double* __restrict__ partials) {
  __shared__ double red[256];
  __shared__ double cmean[256];
  const long long r0 = std::min<long long>((long long)blockIdx.x * rows_per_wg, rows), r1 = std::min<long long>(r0 + rows_per_wg, rows);
  const double n = (double)(r1 - r0);
  double* out = partials + (size_t)blockIdx.x * 2 * C;
  for (int c0 = 0; c0 < C; c0 += 256) {
    const int cb = min(256, C - c0), nl = 256 / cb;
    const int cl = threadIdx.x % cb, rl = threadIdx.x / cb;
    const bool on = rl < nl;
    double s = 0.0;
    if (on)
      for (long long r = r0 + rl; r < r1; r += nl) s += (double)x[(size_t)r * C + c0 + cl];
    __syncthreads();
    if (on) red[rl * cb + cl] = s;
    __syncthreads();
    if (rl == 0) {
      double a = red[cl];
      for (int k = 1; k < nl; ++k) a += red[k * cb + cl];
      cmean[cl] = n > 0.0 ? a / n : 0.0;
    }
    __syncthreads();
    const double mean = cmean[cl];
    double q = 0.0;
    if (on)
      for (long long r = r0 + rl; r < r1; r += nl) {
        const double d = (double)x[(size_t)r * C + c0 + cl] - mean;
        q += d * d;
      }
    if (on) red[rl * cb + cl] = q;
    __syncthreads();
    if (rl == 0) {
      double a = red[cl];
      for (int k = 1; k < nl; ++k) a += red[k * cb + cl];
      out[c0 + cl] = mean;
      out[C + c0 + cl] = a;
    }
  }
}

// state = count[C] | mean[C] | M2[C]; the tiles join it one after the other with Chan's update (no sum x^2 - (sum x)^2 / N)
__global__ __launch_bounds__(256) void column_stats_fold_kernel(const double* __restrict__ partials, double* __restrict__ state, long long rows,
                                                                int C, long long rows_per_wg, int n_rec) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double na = state[c], mean = state[C + c], m2 = state[2 * C + c];
  for (int g = 0; g < n_rec; ++g) {
    const long long r0 = std::min<long long>((long long)g * rows_per_wg, rows), r1 = std::min<long long>(r0 + rows_per_wg, rows);
    const double nb = (double)(r1 - r0);
    if (nb <= 0.0) continue;
    const double mb = partials[(size_t)g * 2 * C + c], qb = partials[(size_t)g * 2 * C + C + c];
    const double nn = na + nb, delta = mb - mean;
    mean += delta * (nb / nn);
    m2 += qb + delta * delta * (na * nb / nn);
    na = nn;
  }
  state[c] = na;
  state[C + c] = mean;
  state[2 * C + c] = m2;
}

// ----------------------------------------------------------------------------------------------
static int fit_geometry(const char* who, long long BT, int PK, int M, int feats, int* W) {
  if (BT < 1 || PK < 1 || M < 1) return set_error("%s: bad argument (rows %lld, PK %d, M %d)", who, BT, PK, M);
  if (feats < 1 || feats > 7 || ((feats & 4) && (PK & 1)))
    return set_error("%s: feats must be a subset of pose|velocity|speed (1|2|4), speed with an even PK", who);
  if ((double)BT > FIT_MAX_ROWS) return set_error("%s: %lld rows in one chunk (at most 2^30: stream the set as several chunks)", who, BT);
  const KMFeat f(feats, PK);
  if ((double)M * (f.D + 1) * sizeof(double) > (double)FIT_LDS_MAX || fit_lds_bytes(M, f.D) > (size_t)FIT_LDS_MAX)
    return set_error("%s: M * (W + 1) = %d * %d cluster sums do not fit the %d bytes of LDS a workgroup may declare", who, M, f.D + 1,
                     FIT_LDS_MAX);
  *W = f.D;
  return 0;
}

}  // namespace ms

using namespace ms;

extern "C" {

size_t ms_kmeans_fit_state_elems(int PK, int M, int feats) {
  int W;
  if (fit_geometry("ms_kmeans_fit_state_elems", 1, PK, M, feats, &W)) return 0;
  return fit_record_elems(M, W);
}

size_t ms_kmeans_fit_workspace(int BT, int PK, int M, int feats) {
  int W;
  if (fit_geometry("ms_kmeans_fit_workspace", BT, PK, M, feats, &W)) return 0;
  return (size_t)slices_of(BT, FIT_SLICE_MIN, FIT_MAX_WGS).nwg * fit_record_elems(M, W) * sizeof(double);
}

int ms_kmeans_fit_accumulate(const float* pose, const int32_t* keep, const double* centres, int64_t* labels, double* state,
                             void* workspace, size_t workspace_bytes, int B, int T, int P, int PK, int M, int feats, void* stream) {
  if (!pose || !keep || !centres || !labels || !state || !workspace) return set_error("ms_kmeans_fit_accumulate: null pointer");
  if (B < 1 || T < 1 || P < 1) return set_error("ms_kmeans_fit_accumulate: bad argument (B %d, T %d, P %d)", B, T, P);
  int W;
  const long long BT = (long long)B * T;
  if (fit_geometry("ms_kmeans_fit_accumulate", BT, PK, M, feats, &W)) return 1;
  if ((double)BT * P >= 2147483648.0) return set_error("ms_kmeans_fit_accumulate: chunk of 2^31 or more elements");
  const Slices s = slices_of(BT, FIT_SLICE_MIN, FIT_MAX_WGS);
  const size_t elems = fit_record_elems(M, W);
  if (workspace_bytes < (size_t)s.nwg * elems * sizeof(double))
    return set_error("ms_kmeans_fit_accumulate: workspace too small (%zu bytes, ms_kmeans_fit_workspace gives %zu)", workspace_bytes,
                     (size_t)s.nwg * elems * sizeof(double));
  const size_t lds = fit_lds_bytes(M, W);
  if (lds > 64 * 1024) {
    static unsigned long long attr_done = 0;          // (per device)
    if (first_time_on_device(attr_done)) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_fit_accumulate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              FIT_LDS_MAX) != hipSuccess)
        return set_error("ms_kmeans_fit_accumulate: cannot raise the dynamic LDS limit");
      done_on_device(attr_done);
    }
  }
  hipLaunchKernelGGL(kmeans_fit_accumulate_kernel, dim3(s.nwg), dim3(256), lds, (hipStream_t)stream, pose, keep, centres, labels,
                     (double*)workspace, (int)BT, T, P, PK, M, feats, (int)s.per);
  if (int rc = check_launch("kmeans_fit_accumulate_kernel")) return rc;
  hipLaunchKernelGGL(fit_fold_kernel, dim3(cdiv((int)elems, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, state,
                     s.nwg, (int)elems);
  return check_launch("fit_fold_kernel");
}

int ms_kmeans_fit_update(const double* state, const double* centres_in, double* centres_out, double* shift_out, int M, int W,
                         void* stream) {
  if (!state || !centres_in || !centres_out || !shift_out) return set_error("ms_kmeans_fit_update: null pointer");
  if (M < 1 || W < 1) return set_error("ms_kmeans_fit_update: bad argument (M %d, W %d)", M, W);
  if (fit_lds_bytes(M, W) > (size_t)FIT_LDS_MAX || (double)M * (W + 1) * sizeof(double) > (double)FIT_LDS_MAX)
    return set_error("ms_kmeans_fit_update: M * (W + 1) = %d * %d is more than ms_kmeans_fit_accumulate takes", M, W + 1);
  hipLaunchKernelGGL(kmeans_fit_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, state, centres_in, centres_out, shift_out, M, W);
  return check_launch("kmeans_fit_update_kernel");
}

size_t ms_column_stats_accumulate_workspace(size_t rows, int C) {
  if (rows < 1 || C < 1 || (double)rows * C > 9.0e15) {
    set_error("ms_column_stats_accumulate_workspace: bad argument (rows %zu, C %d)", rows, C);
    return 0;
  }
  return (size_t)slices_of((long long)rows, STATS_SLICE_MIN, STATS_MAX_WGS).nwg * 2 * C * sizeof(double);
}

int ms_column_stats_accumulate(const float* x, size_t rows, int C, double* state, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !state || !workspace) return set_error("ms_column_stats_accumulate: null pointer");
  if (rows < 1 || C < 1 || (double)rows * C > 9.0e15)
    return set_error("ms_column_stats_accumulate: bad argument (rows %zu, C %d)", rows, C);
  const Slices s = slices_of((long long)rows, STATS_SLICE_MIN, STATS_MAX_WGS);
  const size_t need = (size_t)s.nwg * 2 * C * sizeof(double);
  if (workspace_bytes < need)
    return set_error("ms_column_stats_accumulate: workspace too small (%zu bytes, ms_column_stats_accumulate_workspace gives %zu)",
                     workspace_bytes, need);
  hipLaunchKernelGGL(column_stats_tile_kernel, dim3(s.nwg), dim3(256), 0, (hipStream_t)stream, x, (long long)rows, C, s.per,
                     (double*)workspace);
  if (int rc = check_launch("column_stats_tile_kernel")) return rc;
  hipLaunchKernelGGL(column_stats_fold_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, state,
                     (long long)rows, C, s.per, s.nwg);
  return check_launch("column_stats_fold_kernel");
}

}  // extern "C"
