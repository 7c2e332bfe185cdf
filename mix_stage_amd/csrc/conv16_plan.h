// 16-bit arithmetic mode: the planners of conv16_kernel (forward / data gradient) and wgrad16_kernel (weight gradient) as plain host
// code.  Nothing here needs HIP: conv16.h includes it for the library, and tests/helpers/conv16_plan_host.cpp builds it with the
// host compiler to ask which kernel instance, ring depth and wait count a block lands in.  The knobs the planners read are
// defined in conv16.hip / wgrad16.hip (the library) or by the stand-alone program, both from the defaults below.
#pragma once
#include <algorithm>

#include "mixstage.h"

#if defined(__HIPCC__)
#define MS_PLAN_HD __host__ __device__
#else
#define MS_PLAN_HD
#endif

namespace ms {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int c8_of(int c) { return (c + 7) >> 3; }
inline int pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// ---- forward / data-gradient conv (conv16_kernel.h)
constexpr int conv16_ck8(int KW) { return KW == 8 ? 2 : 4; }
constexpr int CONV16_NP = 6;      // patch vectors a thread stages per stage at most (plan_conv16 keeps CK8*TH*PC <= 6*256)
constexpr int CONV16_MAX_RING = 8; // LDS-DMA ring depth limit (buffers; one less is in flight)
// The K loop's wait counts (nstg - 2) * (NA + npd) that get a loop of their own with the literal in the instruction (conv16_kernel.h);
// every other count takes the run-time switch.  One list for the kernel, the host program and the tests' table.
#define CONV16_WAIT_LITERALS(X) X(0) X(6) X(8) X(10) X(11) X(13) X(18) X(20) X(24)

struct Conv16Plan {
  int ok, wm, wn, nwn, tw, th, tiles_y, tiles_x, n_tiles, ck8, nchunks, pc, lds_bytes, dma, nstg;
};

// tuning knobs (ms_debug_set_conv16_tile / ms_debug_set_conv16_ring) and their values when nothing is set
constexpr int CONV16_DMA_DEFAULT = 1, CONV16_BIG_STAGES_DEFAULT = 2;
extern int g_conv16_force_wm, g_conv16_force_wn;     // tuning knob (ms_debug_set_conv16_tile)
extern int g_conv16_dma;                             // tuning knob: 0 = register-staged path everywhere
extern int g_conv16_wide8;                           // tuning knob: 8-wave form of the 128 x 128 tile (measured: no gain)
extern int g_conv16_ring;                            // tuning knob: force the LDS-DMA ring depth (0 = planner)
extern int g_conv16_big_stages;                      // tuning knob: 0 = short stages everywhere (ms_debug_set_conv16_ring, bit 8 of the flags)

inline Conv16Plan plan_conv16(int nd, int Mg, int groups, int Kc, int KH, int KW, int SH, int SW, int B, int OH, int OW, int zmul,
                              bool up2) {
  Conv16Plan pl = {};
  if (!(KW == 1 || KW == 2 || KW == 3 || KW == 4 || KW == 8)) return pl;
  if (nd == 2 && SH != SW) return pl;
  if (up2 && !(KW == 3 && SW == 1 && nd == 1)) return pl;
  const int rows = nd == 1 ? B : OH, imgs = nd == 1 ? 1 : B;
  const int S = SW, SV = nd == 1 ? 1 : SH;
  const int ck8 = conv16_ck8(KW);
  // candidate tiles, largest first: the first one that fills the chip (>= 192 workgroups), else the smallest
  const int cand[3][2] = {{2, 2}, {1, 2}, {1, 1}};
  for (int c = 0; c < 3; ++c) {
    int wm = cand[c][0], wn = cand[c][1], nwn = 2;
    const int bm = 64 * wm, bn = 64 * wn;
    // the 128 x 128 tile runs as 8 waves (2 x 4, 64 x 32 each) on the LDS-DMA path: same tile, half the per-wave overhead
    if (c == 0 && g_conv16_wide8 && g_conv16_dma && !up2) { wn = 1; nwn = 4; }
    const int nt = 128 * nwn;
    if (g_conv16_force_wm && (cand[c][0] != g_conv16_force_wm || cand[c][1] != g_conv16_force_wn)) continue;
    if (c == 0 && Mg < 128) continue;          // 128-row tiles only for layers with >= 128 rows per group
    const int tw = std::min(pow2_at_least(OW), bn), th = bn / tw;
    const int pc = (tw - 1) * S + KW;
    const int tiles_y = cdiv(rows, th), tiles_x = cdiv(OW, tw);
    const long nwg = (long)imgs * tiles_y * tiles_x * cdiv(Mg, bm) * groups * zmul;
    const bool fits = ck8 * th * pc <= CONV16_NP * nt;
    if (!fits) continue;
    // the 128 x 128 tile only when it leaves >= 384 workgroups: with 256 (the grouped decoder) every CU would hold ONE
    // workgroup whose LDS reads and MFMAs alternate; 64 x 128 tiles put two on a CU and they overlap (20.2 -> 18.7 us)
    if (nwg >= (c == 0 ? 384 : 192) || c == 2 || g_conv16_force_wm) {
      pl.ok = 1; pl.wm = wm; pl.wn = wn; pl.nwn = nwn; pl.tw = tw; pl.th = th; pl.tiles_y = tiles_y; pl.tiles_x = tiles_x;
      pl.n_tiles = imgs * tiles_y * tiles_x;
      pl.ck8 = ck8; pl.nchunks = cdiv(c8_of(Kc), ck8); pl.pc = pc;
      pl.lds_bytes = 2 * (KW * ck8 * bm + ck8 * th * pc + 1) * 16;
      // 64 x 64 (and 64 x 128) tiles on at most 256 workgroups (one per CU, the small layers): stages of twice the channels.  Measured per
      // launch: 256->256 k3 T=64 12.9 -> 9.9 us, k4 s2 13.9 -> 10.8, 3x3 (8,16) 23.0 -> 16.8, 3x8 38.0 -> 30.2; the tiles that share
      // a CU (decoder, first audio-encoder layers) lose 10 % with it and keep the short stages
      if (g_conv16_dma && !up2 && (c == 2 || c == 1) && nwg <= 256 && g_conv16_big_stages && 2 * ck8 * th * pc <= CONV16_NP * nt &&
          2 * (KW * 2 * ck8 * bm + cdiv(2 * ck8 * th * pc, nt) * nt) * 16 <= 160 * 1024) {
        int mult = 2;
        // four times the channels where two such stages still fit (k <= 3 taps per row) and the reduction has more than 2 of them
        if (g_conv16_big_stages >= 2 && c == 2 && KW <= 3 && 4 * ck8 * th * pc <= CONV16_NP * nt && c8_of(Kc) > 2 * ck8 &&
            2 * (KW * 4 * ck8 * bm + cdiv(4 * ck8 * th * pc, nt) * nt) * 16 <= 160 * 1024)
          mult = 4;
        const int ck8b = mult * ck8;
        pl.ck8 = ck8b; pl.nchunks = cdiv(c8_of(Kc), ck8b);
        const int stage = (KW * ck8b * bm + cdiv(ck8b * th * pc, nt) * nt) * 16;
        const int nstages = pl.nchunks * KH;
        int nstg = std::min(std::min(CONV16_MAX_RING, nstages + 1), 160 * 1024 / stage);
        if (g_conv16_ring >= 2) nstg = std::min(nstg, g_conv16_ring);
        pl.dma = 1; pl.nstg = std::max(2, nstg); pl.lds_bytes = pl.nstg * stage;
        return pl;
      }
      if (g_conv16_dma && !up2) {
        // LDS-DMA ring: up to 4 buffers; when the grid holds more workgroups than CUs the ring is kept below half of the
        // CU's LDS so that two workgroups share a CU (one computes while the other waits for its stage)
        const int stage = (KW * ck8 * bm + cdiv(ck8 * th * pc, nt) * nt) * 16;
        const int budget = nwg > 256 ? 80 * 1024 : 160 * 1024;
        // (depth up to 8: the small layers -- 64 x 64 tiles, a handful of workgroups -- are pure latency chains, and with the
        // whole reduction in flight at once they pay one memory round trip instead of one per 3 stages)
        const int nstages = cdiv(c8_of(Kc), ck8) * KH;
        int nstg = std::min(std::min(CONV16_MAX_RING, nstages + 1), budget / stage);
        if (nstg < 2) nstg = std::min(4, 160 * 1024 / stage);
        if (g_conv16_ring >= 2) nstg = std::min(nstg, g_conv16_ring);   // knob: cap the depth
        if (nstg >= 2) { pl.dma = 1; pl.nstg = nstg; pl.lds_bytes = nstg * stage; }
      }
      (void)SV;
      return pl;
    }
  }
  return pl;
}

// ---- weight gradient (wgrad16.hip)
// LDS pitches (16-byte vectors) of a channel block's pixels.  The transposed reads of one MFMA operand touch FOUR channel blocks
// at once (lanes 0-31 of ds_read_b64_tr_b16: 4 rows x 16 banks each), so the block pitch must be = 16 banks (4 vectors) mod 64
// banks: the natural pitches -- 64 vectors for dy, TH*PCX = 66 for a k3 row -- put the four blocks on the same / overlapping
// banks (SQ_LDS_BANK_CONFLICT was 40 % of SQ_LDS_IDX_ACTIVE on the decoder layer).
constexpr int WG16_DP = 68;   // dy: 64 pixels + 4
MS_PLAN_HD inline int wg16_xpitch(int thpcx) { return ((thpcx + 11) & ~15) + 4; }   // smallest pitch >= thpcx that is 4 mod 16
constexpr int WG16_DYV = 8 * WG16_DP;    // vectors of the dy part of a stage
constexpr int WG16_NPX = 5;   // register-staged form (upsample-add input): input-row vectors a thread stages per tile at most

struct Wgrad16Plan { int tp, tw, th, tiles_y, tiles_x, n_tiles, splits, tiles_per_split, ktg, pcx, lds_bytes, nstg, npx; };

constexpr int WGRAD16_RING_DEFAULT = 2, WGRAD16_TARGET_WGS_DEFAULT = 128;
extern int g_wgrad16_ring;           // LDS-DMA ring depth (ms_debug_set_wgrad16_ring)
extern int g_wgrad16_target_wgs;     // workgroups a layer's launch aims for through pixel splits (ms_debug_set_wgrad16_target)

inline Wgrad16Plan plan_wgrad16(int nd, int Cog, int Cig, int groups, int KH, int KW, int SH, int SW, int B, int OH, int OW, bool up2) {
  Wgrad16Plan pl = {};
  const int rows = nd == 1 ? B : OH, imgs = nd == 1 ? 1 : B;
  pl.tp = KW == 1 ? 1 : KW == 3 ? 3 : (KW % 4 == 0) ? 4 : (KW == 2 ? 2 : 0);
  if (!pl.tp) return pl;
  pl.ktg = KW / pl.tp;
  pl.tw = std::min(pow2_at_least(OW), 64);
  pl.th = 64 / pl.tw;
  pl.pcx = (pl.tw - 1) * SW + pl.tp;
  const int xp = wg16_xpitch(pl.th * pl.pcx), xv = 8 * xp;
  pl.npx = cdiv(xv, 256);                              // 256-vector slabs of input rows per tile
  if (up2 && pl.npx > WG16_NPX) return (pl.tp = 0, pl);
  if (xv > 65535) return (pl.tp = 0, pl);
  pl.tiles_y = cdiv(rows, pl.th); pl.tiles_x = cdiv(OW, pl.tw);
  pl.n_tiles = imgs * pl.tiles_y * pl.tiles_x;
  // pixel splits: fill ~2 workgroups per CU, at least 2 tiles per workgroup
  const long base = (long)cdiv(Cog, 64) * cdiv(Cig, 64) * groups * KH * pl.ktg;
  int splits = (int)std::max<long>(1, std::min<long>((g_wgrad16_target_wgs + base - 1) / base, pl.n_tiles / 2));
  splits = std::min(splits, 64);
  pl.tiles_per_split = cdiv(pl.n_tiles, std::max(1, splits));
  pl.splits = cdiv(pl.n_tiles, pl.tiles_per_split);
  if (Cig == 1 && groups == 1 && KH == 3 && KW == 3 && SW == 1 && !up2) {
    // single-input-channel 3x3 block (wgrad16_c1_3x3_kernel: a 33 MB stream over dy at the headline size): slabs = row splits x
    // 64-column tiles, one 4-wave workgroup each -- enough of them (256) to keep the stream in flight; a slab is Cog x 9 floats
    const int col_tiles = cdiv(OW, 64), total_rows = imgs * rows;
    const int row_splits = std::max(1, std::min(256 / col_tiles, total_rows / 8));
    const int rps = cdiv(total_rows, row_splits);
    pl.splits = cdiv(total_rows, rps) * col_tiles;
    pl.tiles_per_split = cdiv(pl.n_tiles, pl.splits);            // (the MFMA kernel is not used for this block)
  }
  // register-staged form (upsample-add input): two buffers.  LDS-DMA form: a ring of g_wgrad16_ring buffers of whole 64-vector
  // wave slabs (17 KB for a k3 row: two buffers leave room for four workgroups per CU)
  const int stage = (WG16_DYV + cdiv(xv, 64) * 64) * 16;
  pl.nstg = up2 ? 2 : std::max(2, std::min(std::min(g_wgrad16_ring, pl.tiles_per_split + 1), 160 * 1024 / stage));
  pl.lds_bytes = up2 ? 2 * (WG16_DYV + xv + 1) * 16 : pl.nstg * stage;
  if (pl.lds_bytes > 160 * 1024) return (pl.tp = 0, pl);
  (void)SH;
  return pl;
}

// npxt: slots of input rows a thread keeps in registers (3, 5) or 0 = the per-tile loop (layers with a few pixels per row).
// Queued jobs (wgrad16_flush) all take the 5-slot instance up to 5 slots: a slot beyond a job's rows is a wave-uniform skip, and
// the jobs of a backward pass then share ONE launch per number of taps -- with 3- and 5-slot instances apart, a single
// 192-workgroup job ran alone on a corner of the chip for 55 us.  (A universal kernel holding every instance behind a switch was
// tried: the register allocator gives the cases disjoint accumulator ranges -- 168 VGPR + 128 AGPR, 3.7 KB of scratch.)
inline int wg16_npxt(int npx) { return npx <= 3 ? 3 : npx <= 5 ? 5 : 0; }

// single-input-channel block: its own (vector-unit) weight-gradient kernel (wgrad16_c1_kernel), up to WGC1_MAX_TAPS taps
constexpr int WGC1_MAX_TAPS = 9;
inline bool wgrad16_c1_shape(int Cig, int groups, int KH, int KW, bool up2) { return !up2 && Cig == 1 && groups == 1 && KH * KW <= WGC1_MAX_TAPS; }

// ---- a block descriptor's three plans (the dispatch of api16.hip)
// The data gradient as SH*SW dense stride-1 convs of dy_raw, one per output-parity class: groups and reduction channels per group
// (a broadcast input sums all groups into the same channels), taps per class.
struct DgradGeo { int tg, tcog, jh, jw, ncls; };
inline DgradGeo dgrad_geo_of(const ms_conv_desc* d) {
  const bool bcast = d->in_mode == MS_IN_BCAST;
  DgradGeo r;
  r.tg = bcast ? 1 : d->groups;
  r.tcog = bcast ? d->groups * d->Cout : d->Cout;
  r.jh = cdiv(d->KH, d->SH); r.jw = cdiv(d->KW, d->SW);
  r.ncls = d->SH * d->SW;
  return r;
}
inline int plan_nd_of(const ms_conv_desc* d) { return (d->H == 1 && d->KH == 1) ? 1 : 2; }      // (geo_of, block_geom.h, takes nd and up2 from here)
inline bool plan_up2_of(const ms_conv_desc* d) { return d->in_mode == MS_IN_UP2ADD; }
inline Conv16Plan fwd_plan16_of(const ms_conv_desc* d) {
  return plan_conv16(plan_nd_of(d), d->Cout, d->groups, d->Cin, d->KH, d->KW, d->SH, d->SW, d->B, d->OH, d->OW, 1, plan_up2_of(d));
}
inline Conv16Plan dgrad_plan16_of(const ms_conv_desc* d, const DgradGeo& r) {
  return plan_conv16(plan_nd_of(d), d->Cin, r.tg, r.tcog, r.jh, r.jw, 1, 1, d->B, cdiv(d->H, d->SH), cdiv(d->W, d->SW), r.ncls, false);
}
inline Wgrad16Plan wgrad_plan16_of(const ms_conv_desc* d) {
  return plan_wgrad16(plan_nd_of(d), d->Cout, d->Cin, d->groups, d->KH, d->KW, d->SH, d->SW, d->B, d->OH, d->OW, plan_up2_of(d));
}

}  // namespace ms
