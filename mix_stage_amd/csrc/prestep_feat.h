// The k-means feature row of the pre-step, once: KMeans.get_feats (transform.py:352-378) on RemoveJoints(pose), in its order
//   pose (PK columns) | velocity (PK) | speed = |(vx, vy)| per kept joint (PK/2),   selected by feats & 1 | 2 | 4.
// ms_kmeans_labels (elementwise.hip) and the fit (prestep_fit.hip) both compute a row's elements and its squared distance to a
// centre with the functions here, so the labels of a fit and of the per-step kernel agree bit for bit by construction.
// Velocity is 0 at t == 0 of each clip; speed pairs kept column d (x block) with kept column PK/2 + d (y block).  All in fp64.
#pragma once
#include <stdint.h>

#include "common.h"

namespace ms {

struct KMFeat {
  bool f_pose, f_vel, f_speed;
  int o_vel, o_speed, D;          // column of the velocity / speed block, width of the row
  __host__ __device__ KMFeat(int feats, int PK)
      : f_pose(feats & 1), f_vel(feats & 2), f_speed(feats & 4), o_vel(f_pose ? PK : 0), o_speed(o_vel + (f_vel ? PK : 0)),
        D(o_speed + (f_speed ? PK / 2 : 0)) {}
};

// xr = the row (b,t) of pose (B,T,P); col = a kept column; the previous frame of the clip is P floats back
__device__ __forceinline__ double km_velocity(const float* __restrict__ xr, int col, int t, int P) {
  return t > 0 ? (double)xr[col] - (double)xr[col - P] : 0.0;
}
// speed of a joint = |(vx, vy)|: the x block and the y block of the kept columns are PK/2 apart
__device__ __forceinline__ double km_speed(const float* __restrict__ xr, const int32_t* __restrict__ keep, int d, int t, int P, int PK) {
  const int cx = keep[d], cy = keep[PK / 2 + d];
  const double vx = t > 0 ? (double)xr[cx] - (double)xr[cx - P] : 0.0;
  const double vy = t > 0 ? (double)xr[cy] - (double)xr[cy - P] : 0.0;
  return sqrt(vx * vx + vy * vy);
}

// element j (0 <= j < f.D) of the feature row
__device__ __forceinline__ double km_feature(const KMFeat& f, const float* __restrict__ xr, const int32_t* __restrict__ keep, int j, int t,
                                             int P, int PK) {
  if (f.f_speed && j >= f.o_speed) return km_speed(xr, keep, j - f.o_speed, t, P, PK);
  if (f.f_vel && j >= f.o_vel) return km_velocity(xr, keep[j - f.o_vel], t, P);
  return (double)xr[keep[j]];
}

// squared distances of the row to G consecutive centres c[g * D + ..], by one wave: lane l takes columns l, l + 64, ... of each
// block, then the butterfly sum -- every lane holds the totals.  Per centre the additions run in the same order whatever G is
// (G only puts independent chains side by side), and that order is the label's definition: first minimum wins.
template <int G>
__device__ __forceinline__ void km_dist2_wave(const KMFeat& f, const float* __restrict__ xr, const int32_t* __restrict__ keep,
                                              const double* __restrict__ c, int lane, int t, int P, int PK, double (&acc)[G]) {
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0.0;
  if (f.f_pose | f.f_vel) {
    for (int d = lane; d < PK; d += 64) {
      const int col = keep[d];
      const double x = (double)xr[col];
      const double v = km_velocity(xr, col, t, P);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const double* cg = c + (size_t)g * f.D;
        if (f.f_pose) { const double dx = cg[d] - x; acc[g] += dx * dx; }
        if (f.f_vel) { const double dv = cg[f.o_vel + d] - v; acc[g] += dv * dv; }
      }
    }
  }
  if (f.f_speed) {
    for (int d = lane; d < PK / 2; d += 64) {
      const double sp = km_speed(xr, keep, d, t, P, PK);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const double ds = c[(size_t)g * f.D + f.o_speed + d] - sp;
        acc[g] += ds * ds;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {          // wave_sum_d, the G exchanges of a step in flight together
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] += __shfl_xor(acc[g], o);
  }
}

// nearest centre of the row, first minimum wins; `bestd` = its squared distance (identical in every lane)
__device__ __forceinline__ int km_nearest_wave(const KMFeat& f, const float* __restrict__ xr, const int32_t* __restrict__ keep,
                                               const double* __restrict__ centers, int M, int lane, int t, int P, int PK, double* bestd_out) {
  int best = 0;
  double bestd = 0.0;
  int m = 0;
  for (; m + 4 <= M; m += 4) {
    double acc[4];
    km_dist2_wave<4>(f, xr, keep, centers + (size_t)m * f.D, lane, t, P, PK, acc);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (m + g == 0 || acc[g] < bestd) { bestd = acc[g]; best = m + g; }
  }
  for (; m < M; ++m) {
    double acc[1];
    km_dist2_wave<1>(f, xr, keep, centers + (size_t)m * f.D, lane, t, P, PK, acc);
    if (m == 0 || acc[0] < bestd) { bestd = acc[0]; best = m; }
  }
  *bestd_out = bestd;
  return best;
}

// ZNorm of one value (transform.py:221-226), in fp64 with the reciprocal of the standard deviation, rounded once to fp32.
// ms_znorm_select (elementwise.hip) and the clip store's draw (clip_store.hip) both call this, so their bits agree by construction.
__device__ __forceinline__ float znorm_value(float x, double mean, double inv_std) { return (float)(((double)x - mean) * inv_std); }

}  // namespace ms
