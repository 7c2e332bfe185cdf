// What the two eval-form chained decoder kernels (chain32_eval.hip, chain16_eval.hip) share: the decoding of a workgroup's
// work unit and the mixture's way out of the workgroup.
#pragma once
#include "kernels.h"

namespace ms {

constexpr int CE_T = CHAIN_EVAL_TILE;     // frames of the LDS image
constexpr int CE_PPAD = 128;              // rows of the logits tile (P <= 128)
constexpr int CE_MT_PITCH = 65;           // floats per row of the logits / mixture tile in LDS [128 rows][64 frames]

struct ChainEvalTileId {
  int u, jc;                  // (sequence, tile) unit; chunk of the groups
  int b, s0, nv;              // sequence; first frame of the image; frames of the image inside the sequence
  int own_lo, own_hi;         // owned frames of the image [own_lo, own_hi)
};

// The group chunk is the slow index of the workgroup id: workgroups that run at the same time stream the same groups' weights
// (speed only: nothing depends on placement or order).
__device__ __forceinline__ ChainEvalTileId chain_eval_tile(int B, int n_tiles, int T) {
  ChainEvalTileId tl;
  const int units = B * n_tiles;
  tl.jc = blockIdx.x / units;
  tl.u = blockIdx.x - tl.jc * units;
  tl.b = tl.u / n_tiles;
  const int k = tl.u - tl.b * n_tiles;
  tl.s0 = CHAIN_EVAL_STEP * k;
  tl.nv = min(CE_T, T - tl.s0);
  tl.own_lo = k == 0 ? 0 : CHAIN_EVAL_HALO;
  tl.own_hi = tl.s0 + CE_T >= T ? tl.nv : CE_T - CHAIN_EVAL_HALO;
  return tl;
}

// oacc: the sum over this workgroup's groups of softmax weight x logits in the logits' MFMA layout (rows 32*wave + 8*(q>>2) +
// 4*(lane>>5) + (q&3), frames 32*nb + (lane&31)).  mt: a free LDS tile of CE_PPAD * CE_MT_PITCH floats; every wave has passed a
// barrier since its last use.  ngw == 1: the owned frames go to out (B, T, P).  ngw > 1: the workgroup stores its partial sum, and
// the one of the unit's ngw workgroups whose counter add came last -- told by the value the add returned: nobody polls, nobody
// waits -- sums the partials in ascending chunk order, its own included (same bits whoever comes last).  Hand-off: sc1 stores,
// every storing wave's s_waitcnt vmcnt(0), workgroup barrier, ONE agent-scope atomic add by one lane, workgroup barrier, sc1 loads.
// The counter is monotonic (a launch adds exactly ngw): nothing to reset, a replayed graph needs nothing from the host.
__device__ __forceinline__ void chain_eval_mix_out(float* mt, int* lflag, const float (&oacc)[2][16], float* part, int* cnt, float* out,
                                                   int P, int T, int ngw, const ChainEvalTileId& tl) {
  typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, n0 = lane & 31, h = lane >> 5;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int prow = 32 * w + 8 * (q >> 2) + 4 * h + (q & 3);
    mt[prow * CE_MT_PITCH + n0] = oacc[0][q];
    mt[prow * CE_MT_PITCH + 32 + n0] = oacc[1][q];
  }
  __syncthreads();
  if (ngw > 1) {
    const __amdgpu_buffer_rsrc_t rsPart = buf_rsrc(part + (size_t)tl.u * ngw * CE_PPAD * CE_T);
    for (int e = t; e < P * (CE_T / 4); e += 256) {
      const int prow = e >> 4, i4 = (e & 15) * 4;
      const float* src = mt + prow * CE_MT_PITCH + i4;
      const float4 v = {src[0], src[1], src[2], src[3]};
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rsPart, (int)(4u * (unsigned)((tl.jc * CE_PPAD + prow) * CE_T + i4)), 0, 16);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every wave: its partial sums have left
    __syncthreads();
    if (t == 0) {
      const unsigned old = (unsigned)__hip_atomic_fetch_add(cnt + 32 * (size_t)tl.u, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      lflag[0] = (old + 1u) % (unsigned)ngw == 0u;
    }
    __syncthreads();
    if (!lflag[0]) return;
    for (int e = t; e < P * (CE_T / 4); e += 256) {
      const int prow = e >> 4, i4 = (e & 15) * 4;
      float4 sum = {0.f, 0.f, 0.f, 0.f};
      for (int j0 = 0; j0 < ngw; j0 += 4) {               // 4 partials in flight, added in ascending order
        float4 v4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const unsigned off = 4u * (unsigned)((min(j0 + i, ngw - 1) * CE_PPAD + prow) * CE_T + i4);
          v4[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsPart, (int)off, 0, 16));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (j0 + i < ngw) { sum.x += v4[i].x; sum.y += v4[i].y; sum.z += v4[i].z; sum.w += v4[i].w; }
      }
      float* dst = mt + prow * CE_MT_PITCH + i4;
      dst[0] = sum.x; dst[1] = sum.y; dst[2] = sum.z; dst[3] = sum.w;
    }
    __syncthreads();
  }
  float* ob = out + ((size_t)tl.b * T + tl.s0) * P;
  const int n_own = tl.own_hi - tl.own_lo;
  for (int e = t; e < n_own * P; e += 256) {
    const int i = tl.own_lo + e / P, pp = e - (e / P) * P;
    ob[(size_t)i * P + pp] = mt[pp * CE_MT_PITCH + i];
  }
}

}  // namespace ms
