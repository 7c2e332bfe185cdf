// Block-level C-ABI entry points: one conv block (conv [+BN] [+LeakyReLU]) forward / backward, fp32 and bf16x6 (the 16-bit modes:
// api16.hip).  Host code only: ONE plan per descriptor and direction -- derived geometry, kernel family with its planner's result,
// scratch layout -- read by the workspace sizes, the weight-preparation entry points and the launch path alike.
#include "block_geom.h"

namespace ms {
extern int g_clip32;

static int validate(const ms_conv_desc* d, const char* who) {
  if (!d) return set_error("%s: null descriptor", who);
  if (d->B < 1 || d->Cin < 1 || d->Cout < 1 || d->groups < 1 || d->H < 1 || d->W < 1 || d->KH < 1 || d->KW < 1 ||
      d->SH < 1 || d->SW < 1 || d->PH < 0 || d->PW < 0)
    return set_error("%s: bad geometry", who);
  const int oh = (d->H + 2 * d->PH - d->KH) / d->SH + 1, ow = (d->W + 2 * d->PW - d->KW) / d->SW + 1;
  if (d->H + 2 * d->PH < d->KH || d->W + 2 * d->PW < d->KW || oh != d->OH || ow != d->OW)
    return set_error("%s: output size (%d,%d) does not match geometry (expected %d,%d)", who, d->OH, d->OW, oh, ow);
  if (d->mode < MS_BARE || d->mode > MS_BN_EVAL) return set_error("%s: bad mode %d", who, d->mode);
  if (d->in_mode < MS_IN_PLAIN || d->in_mode > MS_IN_UP2ADD) return set_error("%s: bad in_mode %d", who, d->in_mode);
  if (d->in_mode == MS_IN_UP2ADD && (d->H != 1 || d->KH != 1 || (d->W & 1)))
    return set_error("%s: UP2ADD needs a 1-D block with even W", who);
  if (dt_of(d) > DT_F16 || (d->dtype & ~(0xff | MS_DT_OUT_F32 | MS_DT_BN_FOLDED | MS_DT_STAT_PAIR | MS_DT_BN_FROZEN))) return set_error("%s: bad dtype 0x%x", who, d->dtype);
  if (dt_of(d) == DT_F32 && (d->dtype & ~(0xff | MS_DT_STAT_PAIR | MS_DT_BN_FROZEN))) return set_error("%s: MS_DT_OUT_F32 is a flag of the 16-bit modes", who);
  if ((d->dtype & MS_DT_BN_FROZEN) && d->mode != MS_BN_EVAL) return set_error("%s: MS_DT_BN_FROZEN is a flag of BN_EVAL blocks", who);
  if ((d->dtype & MS_DT_STAT_PAIR) && (d->B & 1)) return set_error("%s: MS_DT_STAT_PAIR needs an even batch", who);
  const double out_elems = (double)d->B * d->groups * d->Cout * d->OH * d->OW;
  const double in_elems = (double)d->B * d->groups * d->Cin * d->H * d->W;
  // the staging loads address a tensor with 32-bit BYTE offsets against one buffer descriptor: 2 GiB per tensor
  const double lim = dt_of(d) == DT_F32 ? 536870912.0 : 1073741824.0;      // 2^29 fp32 / 2^30 16-bit elements
  if (out_elems >= lim || in_elems >= lim) return set_error("%s: tensor of 2 GiB or more (%.0f elements)", who, std::max(out_elems, in_elems));
  return 0;
}

static inline bool conv_c1_of(const ms_conv_desc* d) {
  return conv_c1_ok(d->groups, d->Cin, d->Cout, d->KH, d->KW, d->SH, d->SW, d->PH, d->PW, d->H, d->in_mode == MS_IN_PLAIN);
}
static inline bool wgrad_c1_of(const ms_conv_desc* d) {
  return dt_of(d) == DT_F32 && g_precision == 0 &&
         wgrad_c1_ok(d->groups, d->Cin, d->Cout, d->KH, d->KW, d->SH, d->SW, d->PH, d->PW, d->H, d->W, d->in_mode == MS_IN_PLAIN);
}

// ---- the forward of block d.  Kernel family: the clip-resident launch first where it applies (it declines at run time, -2, when
// BN_TRAIN has no counters or its grid is not resident at once), then single-channel > patch-staged > gather.
struct FwdPlan {
  BlockGeo g;
  bool clip, c1;
  int c1_tiles;
  PatchPlan pp;            // pp.ok: the patch-staged kernels
  GatherPlan pl;           // else the gather kernel
  bool pair_epilogue;      // MS_DT_STAT_PAIR: the block ends in the register-resident split-K epilogue (one workgroup per channel walks the
                           // two statistics groups) -- the other BatchNorm finishes have no grouped form
  size_t w_bytes;          // prepared weights (ms_fwd_weights_prepare): the clip-resident weight stream / the bf16x6 planes / 0
  // Scratch, byte offsets.  Only one family runs, so statistics | counts, the split-K slab and the clip-resident statistics partials
  // all start at the front; clip_w (the weight stream, when not prepared) follows the partials, planes (bf16x6 weights, when not
  // prepared) follow everything else.  bf16x6 and the clip-resident kernels exclude each other (g_precision).
  struct { size_t stats, part, counts, clip_w, planes, total; } ws;
};
static FwdPlan fwd_plan(const ms_conv_desc* d) {
  FwdPlan p;
  const BlockGeo g = p.g = geo_of(d);
  const bool train = d->mode == MS_BN_TRAIN;
  p.clip = g_precision == 0 && clip32_fwd_ok(d);
  p.c1 = conv_c1_of(d);
  p.c1_tiles = p.c1 ? conv_c1_tiles(d->B, d->H, d->W) : 0;
  p.pp = plan_patch(g.nd, d->Cout, d->groups, d->Cin, d->KH, d->KW, d->SH, d->SW, d->B, d->OH, d->OW, 1, d->W);
  p.pl = plan_gather(d->Cout, g.npix, d->groups, d->Cin * g.khw);
  const PatchPlan& pp = p.pp;
  const bool patch_slab = pp.ok && (pp.splitk > 1 || pp.ksi > 1);
  p.pair_epilogue = !train || ((long)d->B / 2 * g.hw <= 4096 && !p.c1 && (pp.ok ? patch_slab : p.pl.splitk > 1));
  const size_t planes_bytes = (pp.ok && pp.p6) ? (size_t)3 * g.C * patch6_row_elems(d->Cin, d->KH, d->KW) * 2 : 0;
  p.w_bytes = p.clip ? clip32_fwd_weight_bytes(d) : planes_bytes;

  const size_t slab = (size_t)g.npix * g.C * sizeof(float);                // one split-K slice
  auto tile_stats = [&](int n_tiles) { return align_up((size_t)n_tiles * g.C * 2 * sizeof(float), 256); };
  p.ws.stats = p.ws.part = 0;
  p.ws.counts = p.c1 ? tile_stats(p.c1_tiles) : pp.ok ? tile_stats(pp.n_tiles) : 0;
  size_t front = 256;                                                      // (sized for every family, whichever runs)
  if (train) front = std::max(front, (size_t)p.pl.n_tiles * g.C * 2 * sizeof(float));
  if (pp.ok && train) front = std::max(front, tile_stats(pp.n_tiles) + (size_t)pp.n_tiles * sizeof(float));
  if (patch_slab) front = std::max(front, pp.splitk * slab);
  if (p.pl.splitk > 1) front = std::max(front, p.pl.splitk * slab);
  if (p.c1) front = std::max(front, tile_stats(p.c1_tiles) + (size_t)p.c1_tiles * sizeof(float));
  p.ws.total = align_up(front, 256) + 256;
  p.ws.planes = carve(p.ws.total, align_up(planes_bytes, 256));
  p.ws.clip_w = p.clip ? clip32_part_bytes(d->Cout, d->B * d->OW / 32) : 0;
  if (p.clip) p.ws.total = std::max(p.ws.total, p.ws.clip_w + align_up(p.w_bytes, 256) + 256);
  return p;
}

// ---- the backward of block d.  Data gradient: clip-resident (declines at run time when not resident at once) > grouped
// clip-stationary > patch-staged over the output-parity classes > transposed gather.  Weight gradient: single-channel stream >
// patch-staged > gather.
struct BwdPlan {
  BlockGeo g;
  DgradGeo dg;
  int nchunk;              // batch chunks of the BatchNorm / activation backward partials
  bool dg_clip, dg_grouped;
  PatchPlan dpp;           // dpp.ok: the patch-staged kernels
  GatherPlan dpl;          // else the gather kernel
  size_t wt_elems;         // the transposed / parity-class-split copy of w those two read
  size_t dg_planes_bytes;  // bf16x6: the three planes of that copy (0: the fp32 kernels run)
  bool wg_c1;
  WgradPatchPlan wp;       // wp.ok: the patch-staged kernels, else the gather kernel
  int wg_splits;           // pixel splits of the weight gradient as it will run (1: dw is written directly) ...
  int wg_splits_reserved;  // ... and what the scratch holds: the larger of the patch-staged and the gather kernel's
  // Scratch, byte offsets, regions in this order.  dg_part is the split-K slab of whichever data-gradient kernel runs; the total
  // holds the patch-staged slab, the planes and the gather slab one after the other although only one of the two slabs is used.
  struct { size_t fuse_part, bn_part, colpart, wt, wg_part, dg_part, dg_planes, total; } ws;
};
static BwdPlan bwd_plan(const ms_conv_desc* d) {
  BwdPlan p;
  const BlockGeo g = p.g = geo_of(d);
  const DgradGeo dg = p.dg = dgrad_geo_of(d);
  int bpc;
  p.nchunk = bwd_chunks(d->B, g.C, &bpc);
  p.dg_clip = g_precision == 0 && clip32_dgrad_ok(d);
  p.dg_grouped = g_precision == 0 && g_clip32 && gdgrad32_ok(d);
  p.dpp = plan_patch(g.nd, d->Cin, dg.tg, dg.tcog, dg.jh, dg.jw, 1, 1, d->B, cdiv(d->H, d->SH), cdiv(d->W, d->SW), dg.ncls, d->OW);
  p.dpl = plan_gather(d->Cin, d->B * cdiv(d->H, d->SH) * cdiv(d->W, d->SW), dg.tg * dg.ncls, dg.tcog * dg.jh * dg.jw);
  p.wt_elems = dgrad_weight_elems(d->groups, d->Cout, d->Cin, d->KH, d->KW, d->SH, d->SW);
  p.dg_planes_bytes = (p.dpp.ok && p.dpp.p6) ? (size_t)3 * dg.ncls * dg.tg * d->Cin * patch6_row_elems(dg.tcog, dg.jh, dg.jw) * 2 : 0;
  p.wg_c1 = wgrad_c1_of(d);
  p.wp = WgradPatchPlan{};
  if (p.wg_c1) {
    p.wg_splits = p.wg_splits_reserved = wgrad_c1_splits(d->B, d->H);
  } else {
    p.wp = plan_wgrad_patch(g.nd, d->Cout, d->Cin * g.khw, d->groups, d->KH, d->KW, d->SH, d->SW, d->B, d->OH, d->OW, d->W, g.up2 != 0);
    const int gather_splits = wgrad_splits(d->Cout, d->Cin * g.khw, d->groups, g.npix);
    p.wg_splits = p.wp.ok ? p.wp.splits : gather_splits;
    p.wg_splits_reserved = std::max(p.wp.ok ? p.wp.splits : 1, gather_splits);
  }

  const size_t dx_bytes = (size_t)d->B * g.cin_tot * d->H * d->W * sizeof(float);   // one split-K slice of the data gradient
  p.ws.total = 0;
  p.ws.fuse_part = carve(p.ws.total, clip32_dgrad_bn_part_bytes(d));     // partials of a fused producer-BatchNorm backward (ms_bwd_options.prev_*)
  p.ws.bn_part = carve(p.ws.total, align_up((size_t)g.C * p.nchunk * 2 * sizeof(float), 256));
  p.ws.colpart = carve(p.ws.total, align_up((size_t)g.C * p.nchunk * sizeof(float), 256));
  p.ws.wt = carve(p.ws.total, align_up(std::max(p.wt_elems, std::max(clip32_dgrad_weight_floats(d), gdgrad32_weight_floats(d))) * sizeof(float), 256));
  p.ws.wg_part = carve(p.ws.total, align_up(wsize_of(d) * sizeof(float) * (p.wg_splits_reserved > 1 ? p.wg_splits_reserved : 0), 256));
  p.ws.dg_part = carve(p.ws.total, (p.dpp.ok && p.dpp.splitk > 1) ? align_up(p.dpp.splitk * dx_bytes, 256) : 0);
  p.ws.dg_planes = carve(p.ws.total, align_up(p.dg_planes_bytes, 256));
  if (p.dpl.splitk > 1) p.ws.total += align_up(p.dpl.splitk * dx_bytes, 256);
  p.ws.total += 256;
  return p;
}

// The data-gradient weights of block d: none (the patch kernel reads w in place -- stride-1 convs with whole 64-channel tiles), the
// transposed / parity-class-split copy (taps reversed when the patch-staged kernels consume it), or the weight streams of the
// clip-resident / grouped kernels.  Shared by the backward and the prepare entry points so that both take the same decision.
enum { DW_NONE = 0, DW_TRANSPOSED = 1, DW_CLIP = 2, DW_GROUPED = 3 };
static int dgrad_weights_of(const ms_conv_desc* d, const BwdPlan& p, const float* w) {
  if (p.dg_clip) return DW_CLIP;
  if (p.dg_grouped) return DW_GROUPED;
  const bool direct = p.dpp.ok && !p.dpp.p6 && patch_dgrad_direct_ok(w, d->Cin, d->KH, d->KW, d->SH, d->SW, p.g.bcast != 0);
  return direct ? DW_NONE : DW_TRANSPOSED;
}
static size_t dgrad_weights_elems(const ms_conv_desc* d, const BwdPlan& p, int kind) {
  return kind == DW_CLIP ? clip32_dgrad_weight_floats(d) : kind == DW_GROUPED ? gdgrad32_weight_floats(d) : p.wt_elems;
}

}  // namespace ms

using namespace ms;

extern "C" {

size_t ms_conv_block_fwd_workspace(const ms_conv_desc* d) {
  if (!d) return 256;
  return dt_of(d) != DT_F32 ? block_fwd16_workspace(d) : fwd_plan(d).ws.total;
}

size_t ms_conv_block_bwd_workspace(const ms_conv_desc* d) {
  if (!d) return 256;
  return dt_of(d) != DT_F32 ? block_bwd16_workspace(d) : bwd_plan(d).ws.total;
}

int ms_conv_block_fwd(const ms_conv_desc* d, const float* x, const float* x2, const float* w, const float* bias,
                      const float* gamma, const float* beta, float* running_mean, float* running_var, float* y_raw, float* y,
                      float* save, void* workspace, size_t workspace_bytes, void* stream) {
  return ms_conv_block_fwd_ex(d, x, x2, w, bias, gamma, beta, running_mean, running_var, y_raw, y, save, workspace,
                              workspace_bytes, stream, nullptr);
}

static int conv_block_fwd_impl(const ms_conv_desc* d, const float* x, const float* x2, const float* w, const float* bias,
                               const float* gamma, const float* beta, float* running_mean, float* running_var, float* y_raw,
                               float* y, float* save, void* workspace, size_t workspace_bytes, void* stream,
                               const ms_fwd_options* opt);

int ms_conv_block_fwd_ex(const ms_conv_desc* d, const float* x, const float* x2, const float* w, const float* bias,
                         const float* gamma, const float* beta, float* running_mean, float* running_var, float* y_raw,
                         float* y, float* save, void* workspace, size_t workspace_bytes, void* stream,
                         const ms_fwd_options* opt) {
  // the stream's hold (ms_clip_hold): a block held back from an earlier call goes first unless this call can share its launch
  const bool clip_path = d && dt_of(d) == DT_F32 && g_precision == 0 && !validate(d, "ms_conv_block_fwd") && clip32_fwd_ok(d);
  int rc = clip32_call_begin((hipStream_t)stream, clip_path, workspace, workspace_bytes);
  if (!rc) rc = conv_block_fwd_impl(d, x, x2, w, bias, gamma, beta, running_mean, running_var, y_raw, y, save, workspace, workspace_bytes, stream, opt);
  clip32_call_end((hipStream_t)stream);
  return rc;
}

static int conv_block_fwd_impl(const ms_conv_desc* d, const float* x, const float* x2, const float* w, const float* bias,
                               const float* gamma, const float* beta, float* running_mean, float* running_var, float* y_raw,
                               float* y, float* save, void* workspace, size_t workspace_bytes, void* stream,
                               const ms_fwd_options* opt) {
  const unsigned short* w_planes = opt ? (const unsigned short*)opt->w_planes : nullptr;
  int rc = validate(d, "ms_conv_block_fwd");
  if (rc) return rc;
  if (!x || !w || !y) return set_error("ms_conv_block_fwd: null tensor");
  const bool bn = d->mode == MS_BN_TRAIN || d->mode == MS_BN_EVAL;
  if (bn && (!gamma || !beta || !running_mean || !running_var)) return set_error("ms_conv_block_fwd: BN tensors missing");
  if (d->mode == MS_BN_TRAIN && (!y_raw || !save || !workspace)) return set_error("ms_conv_block_fwd: y_raw/save/workspace missing");
  if (d->in_mode == MS_IN_UP2ADD && !x2) return set_error("ms_conv_block_fwd: UP2ADD needs x2");
  // BN_EVAL with MS_DT_BN_FROZEN: the differentiable (frozen-statistics) form -- the conv as its MS_BARE launch into y_raw, then ONE
  // launch that writes `save` from the running statistics, normalises and activates.  The running statistics are only read.
  // (Without the flag a BN_EVAL block is the one-launch eval form whatever y_raw / save point to, as it always was.)
  const bool frozen = d->mode == MS_BN_EVAL && (d->dtype & MS_DT_BN_FROZEN);
  if (frozen && (d->dtype & MS_DT_BN_FOLDED)) return set_error("ms_conv_block_fwd: MS_DT_BN_FOLDED with MS_DT_BN_FROZEN: a folded block has no BatchNorm to differentiate");
  if (frozen && (!y_raw || !save || !workspace)) return set_error("ms_conv_block_fwd: MS_DT_BN_FROZEN (the differentiable BN_EVAL form) needs y_raw/save/workspace");
  if (frozen && dt_of(d) == DT_F32) {
    ms_conv_desc bare = *d;
    bare.mode = MS_BARE;
    bare.dtype &= ~(MS_DT_STAT_PAIR | MS_DT_BN_FROZEN);          // (no statistics groups: a plain batch of B)
    if (workspace_bytes < fwd_plan(d).ws.total) return set_error("ms_conv_block_fwd: workspace too small");
    rc = conv_block_fwd_impl(&bare, x, x2, w, bias, nullptr, nullptr, nullptr, nullptr, nullptr, y_raw, nullptr, workspace, workspace_bytes, stream, opt);
    if (!rc) rc = clip32_hold_flush((hipStream_t)stream);      // (the conv's launch is on the stream before its reader)
    if (rc) return rc;
    const BlockGeo g = geo_of(d);
    return launch_bn_apply_frozen(y_raw, y, save, gamma, beta, running_mean, running_var, d->eps, g.C, g.hw, (size_t)g.npix * g.C, d->slope,
                                  (hipStream_t)stream);
  }
  if (dt_of(d) != DT_F32)     // 16-bit modes: the tensor pointers are cb8 buffers (include/mixstage.h, ms_dtype)
    return block_fwd16(d, x, x2, w, bias, gamma, beta, running_mean, running_var, y_raw, y, save, workspace, workspace_bytes,
                       (hipStream_t)stream, w_planes, opt ? opt->bn_sync : nullptr, opt ? opt->bn_sync_words : 0);
  const FwdPlan p = fwd_plan(d);
  if (workspace_bytes < p.ws.total) return set_error("ms_conv_block_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const BlockGeo& g = p.g;
  const int C = g.C, npix = g.npix, hw = g.hw, Kg = d->Cin * g.khw;
  float* stats = ws_at<float>(workspace, p.ws.stats);
  float* counts = ws_at<float>(workspace, p.ws.counts);
  float* part = ws_at<float>(workspace, p.ws.part);

  if (p.clip) {
    // 1-D blocks whose whole reduction fits a workgroup (clip32.hip): conv, statistics, meeting, normalisation in ONE launch
    const float* wp = (const float*)w_planes;
    if (!wp) {
      float* mine = ws_at<float>(workspace, p.ws.clip_w);
      rc = clip32_prep_queue(w, mine, d->Cout, d->Cin, d->KW, 0, d->Cin, s);
      if (!rc) rc = clip32_prep_flush(s);
      if (rc) return rc;
      wp = mine;
    }
    rc = clip32_block_fwd(d, x, x2, wp, bias, gamma, beta, running_mean, running_var, y_raw, y, save, stats, opt ? opt->bn_sync : nullptr,
                          opt ? opt->bn_sync_words : 0, s);
    if (rc != -2) return rc;          // (-2: BN_TRAIN without counters, or a grid that is not resident at once: the kernels below)
    rc = clip32_hold_flush(s);        // (... in stream order behind a block the stream's hold may still hold)
    if (rc) return rc;
  }

  float* out = d->mode == MS_BN_TRAIN ? y_raw : y;
  const int a_vec = (Kg % 4 == 0) && (((uintptr_t)w & 15) == 0);
  const int ep = d->mode == MS_BARE ? EP_BARE : d->mode == MS_LRELU ? EP_LRELU : d->mode == MS_BN_EVAL ? EP_BN_EVAL : EP_RAW_STATS;
  const int sg = d->mode == MS_BN_TRAIN ? sg_of(d) : 1;
  if (sg > 1 && !p.pair_epilogue)
    return set_error("ms_conv_block_fwd: MS_DT_STAT_PAIR is not implemented for this block's kernels (ms_stat_pair_ok)");
  if (p.c1) {
    // one input channel (the AudioEncoder's first block): VALU kernel bound by the output write
    rc = launch_conv_c1(x, w, bias, out, gamma, beta, running_mean, running_var, stats, counts, d->B, d->H, d->W, ep, d->slope,
                        d->eps, s);
    if (rc) return rc;
    if (d->mode == MS_BN_TRAIN) {
      rc = launch_bn_finalize_apply(stats, counts, p.c1_tiles, 0, npix, C, gamma, beta, running_mean, running_var, save, d->eps,
                                    d->momentum, y_raw, y, d->B, hw, d->slope, s);
    }
    return rc;
  }
  if (p.pp.ok) {
    // rows >= 16 wide: patch-staged kernel (raw input patch in LDS, no im2col address math in the K loop)
    const PatchPlan& pp = p.pp;
    PatchArgs q = {};
    q.A = w; q.src = x; q.src2 = x2; q.out = out;
    q.bias = bias; q.bn_g = gamma; q.bn_b = beta; q.bn_m = running_mean; q.bn_v = running_var;
    q.stats = stats; q.counts = counts;
    q.Mg = d->Cout; q.Kg = Kg; q.groups = d->groups; q.Kc = d->Cin; q.bcast = g.bcast; q.a_vec = a_vec; q.ep = ep;
    fill_src(q, plane_strides(g.one_d, d->B, g.cin_tot, d->H, d->W));
    fill_out(q, plane_strides(g.one_d, d->B, C, d->OH, d->OW));
    q.PH = g.one_d ? 0 : d->PH;
    q.PW = d->PW; q.tiles_x = pp.tiles_x; q.tiles_y = pp.tiles_y; q.slope = d->slope; q.eps = d->eps;
    q.o_sh = 1; q.o_sw = 1; q.o_ry = 0; q.o_rx = 0;
    q.splitk = pp.splitk; q.chunks_per_split = pp.chunks_per_split;
    q.src_elems = (size_t)d->B * g.cin_tot * d->H * d->W; q.a_elems = (size_t)C * Kg;
    // BN_TRAIN with the intra-workgroup split: raw tile out, then the split-K epilogue (1 slice) does bias + batch
    // statistics + normalisation in ONE launch instead of finalize + apply
    const bool raw_out = pp.splitk > 1 || (pp.ksi > 1 && d->mode == MS_BN_TRAIN);
    if (raw_out) { q.part = part; q.part_stride = (size_t)npix * C; }
    const double flops = 2.0 * d->Cout * Kg * (double)npix * d->groups;
    const double bytes = 4.0 * ((double)C * Kg + (double)d->B * g.cin_tot * d->H * d->W + (double)npix * C);
    if (pp.p6) {
      // bf16x6: three bf16 planes of the weights -- the trainer's (ms_fwd_options.w_planes) or built here behind the other scratch
      const int re = patch6_row_elems(d->Cin, d->KH, d->KW);
      const unsigned short* planes = w_planes;
      if (!planes) {
        unsigned short* mine = ws_at<unsigned short>(workspace, p.ws.planes);
        rc = launch_split_weights(w, mine, C, d->Cin, d->KH, d->KW, s);
        if (rc) return rc;
        planes = mine;
      }
      q.Aplanes = planes; q.plane_stride = (unsigned)((size_t)C * re); q.a_row_elems = re;
      rc = launch_patch6(q, pp, d->KH, d->KW, d->SW, g.up2 != 0, flops, bytes, s);
    } else {
      rc = launch_patch(q, pp, d->KH, d->KW, d->SW, g.up2 != 0, flops, bytes, s);
    }
    if (rc) return rc;
    if (raw_out)
      return launch_splitk_fwd_epilogue(q.part, pp.splitk, q.part_stride, bias, gamma, beta, running_mean, running_var, y_raw,
                                        y, save, d->B, C, hw, ep, d->slope, d->eps, d->momentum, s, sg);
    if (d->mode == MS_BN_TRAIN) {
      rc = launch_bn_finalize_apply(stats, counts, pp.n_tiles, 0, npix, C, gamma, beta, running_mean, running_var, save, d->eps,
                                    d->momentum, y_raw, y, d->B, hw, d->slope, s);
    }
    return rc;
  }
  const GatherPlan& pl = p.pl;
  GatherArgs a = {};
  a.A = w; a.src = x; a.src2 = x2; a.out = out;
  a.bias = bias; a.bn_g = gamma; a.bn_b = beta; a.bn_m = running_mean; a.bn_v = running_var;
  a.stats = stats;
  a.Mg = d->Cout; a.Kg = Kg; a.groups = d->groups; a.Kc = d->Cin;
  a.bcast = g.bcast; a.src_ctotal = g.cin_tot;
  a.SRCH = d->H; a.SRCW = d->W; a.OUTH = d->OH; a.OUTW = d->OW; a.Npix = npix;
  a.KH = d->KH; a.KW = d->KW; a.SH = d->SH; a.SW = d->SW; a.PH = d->PH; a.PW = d->PW;
  a.a_vec = a_vec; a.ep = ep;
  a.slope = d->slope; a.eps = d->eps;
  if (pl.splitk > 1) {
    a.part = part;
    a.part_stride = (size_t)npix * C;
  }
  rc = launch_gather(a, false, g.up2 != 0, pl, s);
  if (rc) return rc;
  if (pl.splitk > 1) {
    // few output pixels: K was sliced over workgroups; one launch sums the slices and finishes the block
    return launch_splitk_fwd_epilogue(a.part, pl.splitk, a.part_stride, bias, gamma, beta, running_mean, running_var, y_raw, y,
                                      save, d->B, C, hw, ep, d->slope, d->eps, d->momentum, s, sg);
  }
  if (d->mode == MS_BN_TRAIN) {
    rc = launch_bn_finalize_apply(stats, nullptr, pl.n_tiles, 64 * pl.tn, npix, C, gamma, beta, running_mean, running_var, save,
                                  d->eps, d->momentum, y_raw, y, d->B, hw, d->slope, s);
  }
  return rc;
}

size_t ms_wgrad_partials_elems(const ms_conv_desc* d, int* splits) {
  if (validate(d, "ms_wgrad_partials_elems")) return 0;
  const int sp = dt_of(d) != DT_F32 ? wgrad16_splits(d) : bwd_plan(d).wg_splits;
  if (splits) *splits = sp;
  return sp > 1 ? (size_t)sp * wsize_of(d) : 0;
}

int ms_wgrad_reduce_multi(int n, const float* const* partials, float* const* dw, const int* elems, const int* splits,
                          void* stream) {
  if (n < 0 || (n && (!partials || !dw || !elems || !splits))) return set_error("ms_wgrad_reduce_multi: null argument");
  // every job is checked before the first launch: a bad job behind REDUCE_BATCH_MAX good ones must not leave half the call done
  for (int i = 0; i < n; ++i)
    if (!partials[i] || !dw[i] || elems[i] <= 0 || splits[i] < 1) return set_error("ms_wgrad_reduce_multi: bad job %d", i);
  ReduceBatch rb;
  rb.n = 0;
  for (int i = 0; i < n; ++i) {
    ReduceJob jb = {partials[i], dw[i], elems[i], splits[i], 0, 0};
    rb.job[rb.n++] = jb;
    if (rb.n == REDUCE_BATCH_MAX) {
      const int rc = launch_reduce_splits_multi(rb, (hipStream_t)stream);
      if (rc) return rc;
      rb.n = 0;
    }
  }
  return rb.n ? launch_reduce_splits_multi(rb, (hipStream_t)stream) : 0;
}

size_t ms_dgrad_weights_elems(const ms_conv_desc* d, const float* w) {
  if (validate(d, "ms_dgrad_weights_elems")) return 0;
  if (dt_of(d) != DT_F32) return 0;          // 16-bit modes: ms_weights16_bytes / ms_weights16_prepare
  const BwdPlan p = bwd_plan(d);
  const int kind = dgrad_weights_of(d, p, w);
  if (kind == DW_NONE) return 0;
  return align_up(dgrad_weights_elems(d, p, kind), 64) + (p.dg_planes_bytes + 3) / 4;      // fp32 copy | bf16 planes (bf16x6 mode)
}

size_t ms_fwd_weights_bytes(const ms_conv_desc* d) {
  if (validate(d, "ms_fwd_weights_bytes")) return 0;
  if (dt_of(d) != DT_F32) return 0;          // 16-bit modes: ms_weights16_bytes / ms_weights16_prepare
  return fwd_plan(d).w_bytes;
}

int ms_fwd_weights_prepare(int n, const ms_conv_desc* descs, const float* const* w, void* const* planes, void* stream) {
  if (n < 0 || (n && (!descs || !w || !planes))) return set_error("ms_fwd_weights_prepare: null argument");
  PrepQueueGuard queue_guard;          // (after the flush below the queues are empty: the guard only matters on error paths)
  SplitBatch sb;
  sb.n = 0;
  for (int i = 0; i < n; ++i) {
    const ms_conv_desc* d = descs + i;
    int rc = validate(d, "ms_fwd_weights_prepare");
    if (rc) return rc;
    if (dt_of(d) != DT_F32) continue;
    const FwdPlan p = fwd_plan(d);
    if (!p.w_bytes) continue;
    if (!planes[i]) return set_error("ms_fwd_weights_prepare: block %d needs a buffer of ms_fwd_weights_bytes bytes", i);
    if (p.clip) {
      rc = clip32_prep_queue(w[i], (float*)planes[i], d->Cout, d->Cin, d->KW, 0, d->Cin, (hipStream_t)stream);
      if (rc) return rc;
      continue;
    }
    SplitJob jb = {w[i], (unsigned short*)planes[i], p.g.C, d->Cin, p.g.khw, 0, 0, 0};
    sb.job[sb.n++] = jb;
    if (sb.n == SPLIT_BATCH_MAX) {
      rc = launch_split_weights_multi(sb, (hipStream_t)stream);
      if (rc) return rc;
      sb.n = 0;
    }
  }
  { const int rcq = clip32_prep_flush((hipStream_t)stream); if (rcq) return rcq; }
  return sb.n ? launch_split_weights_multi(sb, (hipStream_t)stream) : 0;
}

int ms_dgrad_weights_prepare(int n, const ms_conv_desc* descs, const float* const* w, float* const* wt, void* stream) {
  if (n < 0 || (n && (!descs || !w || !wt))) return set_error("ms_dgrad_weights_prepare: null argument");
  PrepQueueGuard queue_guard;
  TransposeBatch tb;
  tb.n = 0;
  for (int i = 0; i < n; ++i) {
    const ms_conv_desc* d = descs + i;
    int rc = validate(d, "ms_dgrad_weights_prepare");
    if (rc) return rc;
    const BwdPlan p = bwd_plan(d);
    const int kind = dgrad_weights_of(d, p, w[i]);
    if (kind == DW_NONE) continue;
    if (!wt[i]) return set_error("ms_dgrad_weights_prepare: block %d needs a buffer of ms_dgrad_weights_elems floats", i);
    if (kind == DW_CLIP) {
      rc = clip32_prep_queue(w[i], wt[i], d->Cin, d->Cout, d->KW, d->KW == 4 ? 2 : 1, d->Cin, (hipStream_t)stream);
      if (rc) return rc;
      continue;
    }
    if (kind == DW_GROUPED) {
      rc = gdgrad32_prepare(d, w[i], wt[i], (hipStream_t)stream);
      if (rc) return rc;
      continue;
    }
    TransposeJob jb = {w[i], wt[i], p.dg.tg, p.dg.tcog, d->Cin, d->KH, d->KW, d->SH, d->SW, d->PH, d->PW, p.dpp.ok ? 1 : 0, 0};
    tb.job[tb.n++] = jb;
    if (tb.n == TRANSPOSE_BATCH_MAX) {
      rc = launch_transpose_weight_multi(tb, (hipStream_t)stream);
      if (rc) return rc;
      tb.n = 0;
    }
  }
  if (tb.n) {
    const int rc = launch_transpose_weight_multi(tb, (hipStream_t)stream);
    if (rc) return rc;
  }
  { int rcq = clip32_prep_flush((hipStream_t)stream); if (!rcq) rcq = gdgrad32_prep_flush((hipStream_t)stream); if (rcq) return rcq; }
  // bf16x6 mode: the planes of the fp32 copies just built, behind them
  SplitBatch sb;
  sb.n = 0;
  for (int i = 0; i < n; ++i) {
    const ms_conv_desc* d = descs + i;
    const BwdPlan p = bwd_plan(d);
    if (!p.dg_planes_bytes || dgrad_weights_of(d, p, w[i]) != DW_TRANSPOSED) continue;
    SplitJob jb = {wt[i], (unsigned short*)(wt[i] + align_up(p.wt_elems, 64)), p.dg.ncls * p.dg.tg * d->Cin, p.dg.tcog, p.dg.jh * p.dg.jw, 0, 0, 0};
    sb.job[sb.n++] = jb;
    if (sb.n == SPLIT_BATCH_MAX) {
      const int rc = launch_split_weights_multi(sb, (hipStream_t)stream);
      if (rc) return rc;
      sb.n = 0;
    }
  }
  return sb.n ? launch_split_weights_multi(sb, (hipStream_t)stream) : 0;
}

int ms_stat_pair_ok(const ms_conv_desc* d) {
  if (!d || (d->B & 1) || validate(d, "ms_stat_pair_ok")) return 0;
  if (d->mode != MS_BN_TRAIN) return 1;                 // no batch statistics: a batch of B
  if (dt_of(d) != DT_F32) return stat_pair16_ok(d) ? 1 : 0;
  if (g_precision != 0) return 0;
  // backward: the one-launch BatchNorm backward walks the groups
  if ((long)d->B / 2 * d->OH * d->OW > BN_BWD32_FUSED_MAX) return 0;
  const FwdPlan p = fwd_plan(d);
  if (p.clip) {
    // the clip-resident launch: whole pixel workgroups per half, every workgroup resident at once (else the kernels below)
    const int npx = d->SW == 2 ? 32 : 64, npw = d->B * d->OW / npx, cus = current_device_cus();
    if (npw % 2 == 0 && cus > 0 && cdiv(d->Cout, 32) * npw <= cus) return 1;
  }
  return p.pair_epilogue ? 1 : 0;
}

int ms_dgrad_fuses_prev_bn(const ms_conv_desc* d) {
  if (!d || validate(d, "ms_dgrad_fuses_prev_bn") || (d->dtype & MS_DT_STAT_PAIR)) return 0;
  return (dt_of(d) == DT_F32 && g_precision == 0 && clip32_dgrad_bn_ok(d)) ? 1 : 0;
}

int ms_dgrad_takes_accum(const ms_conv_desc* d) {
  if (!d || validate(d, "ms_dgrad_takes_accum")) return 0;
  if (dt_of(d) != DT_F32) return dgrad16_takes_accum(d) ? 1 : 0;
  return (g_precision == 0 && d->in_mode == MS_IN_PLAIN && clip32_dgrad_ok(d)) ? 1 : 0;
}

int ms_conv_block_bwd(const ms_conv_desc* d, const float* x, const float* x2, const float* w, const float* gamma,
                      const float* running_mean, const float* running_var, const float* y_raw, const float* y,
                      const float* save, const float* dy, float* dyr, float* dx, float* dx2, float* dw, float* dbias,
                      float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  ms_bwd_options o = {};
  return ms_conv_block_bwd_ex(d, x, x2, w, gamma, running_mean, running_var, y_raw, y, save, dy, dyr, dx, dx2, dw, dbias,
                              dgamma, dbeta, workspace, workspace_bytes, stream, &o);
}

static hipEvent_t fork_event() {
  static thread_local hipEvent_t ev = nullptr;
  if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
  return ev;
}

int ms_conv_block_bwd_overlap(const ms_conv_desc* d, const float* x, const float* x2, const float* w, const float* gamma,
                              const float* running_mean, const float* running_var, const float* y_raw, const float* y,
                              const float* save, const float* dy, float* dyr, float* dx, float* dx2, float* dw,
                              float* dbias, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                              void* stream, void* side_stream, void* side_workspace, size_t side_workspace_bytes) {
  ms_bwd_options o = {};
  o.side_stream = side_stream; o.side_workspace = side_workspace; o.side_workspace_bytes = side_workspace_bytes;
  return ms_conv_block_bwd_ex(d, x, x2, w, gamma, running_mean, running_var, y_raw, y, save, dy, dyr, dx, dx2, dw, dbias,
                              dgamma, dbeta, workspace, workspace_bytes, stream, &o);
}

static int conv_block_bwd_impl(const ms_conv_desc* d, const float* x, const float* x2, const float* w, const float* gamma,
                               const float* running_mean, const float* running_var, const float* y_raw, const float* y,
                               const float* save, const float* dy, float* dyr, float* dx, float* dx2, float* dw, float* dbias,
                               float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream,
                               const ms_bwd_options* opt);

int ms_conv_block_bwd_ex(const ms_conv_desc* d, const float* x, const float* x2, const float* w, const float* gamma,
                         const float* running_mean, const float* running_var, const float* y_raw, const float* y,
                         const float* save, const float* dy, float* dyr, float* dx, float* dx2, float* dw, float* dbias,
                         float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream,
                         const ms_bwd_options* opt) {
  // the stream's hold (ms_clip_hold), as in ms_conv_block_fwd_ex: a data gradient held back from an earlier call goes first unless
  // this call's data gradient can share its launch
  int rc = validate(d, "ms_conv_block_bwd");      // (once, here: a bad descriptor leaves the hold as it is)
  if (rc) return rc;
  const bool side = opt && opt->side_stream && opt->side_stream != stream;
  const bool clip_path = dx && !side && dt_of(d) == DT_F32 && g_precision == 0 && clip32_dgrad_ok(d);
  rc = clip32_call_begin((hipStream_t)stream, clip_path, workspace, workspace_bytes);
  if (!rc) rc = conv_block_bwd_impl(d, x, x2, w, gamma, running_mean, running_var, y_raw, y, save, dy, dyr, dx, dx2, dw, dbias, dgamma, dbeta,
                                    workspace, workspace_bytes, stream, opt);
  clip32_call_end((hipStream_t)stream);
  return rc;
}

static int conv_block_bwd_impl(const ms_conv_desc* d, const float* x, const float* x2, const float* w, const float* gamma,
                               const float* running_mean, const float* running_var, const float* y_raw, const float* y,
                               const float* save, const float* dy, float* dyr, float* dx, float* dx2, float* dw, float* dbias,
                               float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream,
                               const ms_bwd_options* opt) {
  (void)running_mean; (void)running_var;
  ms_bwd_options none = {};
  if (!opt) opt = &none;
  void* side_stream = opt->side_stream;
  const float* wt_prepared = opt->wt_prepared;
  const bool defer_wgrad = opt->wgrad_partials != nullptr;
  int rc = 0;                                      // (d is validated: ms_conv_block_bwd_ex)
  if (!dy || !w || !workspace) return set_error("ms_conv_block_bwd: null tensor");
  // BN_EVAL: the frozen-statistics block (forward: BN_EVAL with y_raw).  Only step 1 below knows the mode.
  const bool frozen = d->mode == MS_BN_EVAL;
  if (frozen && (!y_raw || !save || !gamma || !dyr)) return set_error("ms_conv_block_bwd: BN_EVAL (frozen statistics) needs y_raw/save/gamma/dyr");
  if (frozen && opt->dy_is_dyr) return set_error("ms_conv_block_bwd: dy_is_dyr on a BN_EVAL block: a frozen block is never a fused producer");
  if (frozen && side_stream && side_stream != stream) return set_error("ms_conv_block_bwd: no side-stream form for BN_EVAL (frozen statistics) blocks");
  if (d->mode == MS_BN_TRAIN && !opt->dy_is_dyr && (!y_raw || !save || !gamma || !dyr)) return set_error("ms_conv_block_bwd: BN_TRAIN needs y_raw/save/gamma/dyr");
  if ((opt->dy_is_dyr || opt->prev_y) && (dt_of(d) != DT_F32 || side_stream)) return set_error("ms_conv_block_bwd: the fused producer-BatchNorm backward is an fp32, single-stream form");
  if (d->mode == MS_LRELU && (!y || !dyr)) return set_error("ms_conv_block_bwd: LRELU needs y/dyr");
  if (dw && !x) return set_error("ms_conv_block_bwd: dw needs x");
  if (opt->dx_accum && !(dx && ms_dgrad_takes_accum(d))) return set_error("ms_conv_block_bwd: dx_accum on a block ms_dgrad_takes_accum() declines");
  if (d->in_mode == MS_IN_UP2ADD && ((dw && !x2) || (dx && !dx2))) return set_error("ms_conv_block_bwd: UP2ADD needs x2/dx2");
  if (dt_of(d) != DT_F32) {
    if (side_stream) return set_error("ms_conv_block_bwd: no side-stream form in the 16-bit modes");
    if (d->mode == MS_BARE && out_f32_of(d) && !dyr) return set_error("ms_conv_block_bwd: fp32 dy needs the dyr scratch");
    return block_bwd16(d, x, x2, w, gamma, y_raw, y, save, dy, dyr, dx, dx2, dw, dbias, dgamma, dbeta, workspace, workspace_bytes,
                       (hipStream_t)stream, wt_prepared, opt->wgrad_partials, opt->defer_wgrad_launch, opt->dx_accum);
  }
  const BwdPlan p = bwd_plan(d);
  if (workspace_bytes < p.ws.total) return set_error("ms_conv_block_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const BlockGeo& g = p.g;
  const DgradGeo& dg = p.dg;
  const int C = g.C, npix = g.npix, hw = g.hw, Kg = d->Cin * g.khw;
  const bool up2 = g.up2 != 0, bcast = g.bcast != 0;

  float* fuse_part = ws_at<float>(workspace, p.ws.fuse_part);
  float* bn_part = ws_at<float>(workspace, p.ws.bn_part);
  float* colpart = ws_at<float>(workspace, p.ws.colpart);
  float* wt = ws_at<float>(workspace, p.ws.wt);
  float* wg_part = ws_at<float>(workspace, p.ws.wg_part);
  float* dg_part = ws_at<float>(workspace, p.ws.dg_part);
  // weight gradient on the side stream (its own scratch, same layout): it only needs dy_raw and the saved input, so it runs
  // concurrently with this block's data gradient and the earlier blocks' backward on `stream`
  if (defer_wgrad) wg_part = opt->wgrad_partials;   // pixel-split partial slabs stay there; the caller reduces them later
  hipStream_t ws_stream = s;
  if (side_stream && side_stream != stream && dw) {
    if (defer_wgrad) return set_error("ms_conv_block_bwd_ex: wgrad_partials and side_stream are exclusive");
    if (!opt->side_workspace || opt->side_workspace_bytes < p.ws.total)
      return set_error("ms_conv_block_bwd_overlap: side workspace too small");
    ws_stream = (hipStream_t)side_stream;
    wg_part = ws_at<float>(opt->side_workspace, p.ws.wg_part);
  }

  // 1. gradient wrt the raw conv output (+ per-channel column sums = bias gradient)
  const float* gr = dy;
  int bias_done = 0;
  const bool have_prev = opt->prev_y != nullptr;
  if (have_prev && !(dx && g_precision == 0 && clip32_dgrad_bn_ok(d)))
    return set_error("ms_conv_block_bwd: this block's data gradient cannot carry the producer's BatchNorm backward (ms_dgrad_fuses_prev_bn)");
  if (opt->dy_is_dyr) {
    // a consumer's fused data-gradient launch already applied this block's BatchNorm + activation backward (and wrote dgamma / dbeta / dbias)
    if (d->mode != MS_BN_TRAIN) return set_error("ms_conv_block_bwd: dy_is_dyr is the BN_TRAIN form");
    bias_done = 1;
  } else if (d->mode == MS_BN_TRAIN) {
    rc = launch_bn_bwd(dy, y_raw, y, save, gamma, bn_part, dyr, colpart, dbias, dgamma, dbeta, d->B, C, hw, d->slope, &bias_done, s, sg_of(d));
    gr = dyr;
  } else if (frozen) {
    rc = launch_bn_bwd(dy, y_raw, nullptr, save, gamma, bn_part, dyr, colpart, dbias, dgamma, dbeta, d->B, C, hw, d->slope, &bias_done, s, 1, true);
    gr = dyr;
  } else if (d->mode == MS_LRELU) {
    rc = launch_act_bwd(dy, y, dyr, colpart, dbias, d->B, C, hw, 1, d->slope, &bias_done, s);
    gr = dyr;
  } else if (dbias) {
    rc = launch_act_bwd(dy, nullptr, nullptr, colpart, dbias, d->B, C, hw, 0, 0.f, &bias_done, s);
  }
  if (rc) return rc;
  if (dbias && !bias_done && !opt->dy_is_dyr) {
    rc = launch_colsum_finalize(colpart, dbias, d->B, C, s);
    if (rc) return rc;
  }

  if (ws_stream != s) {
    hipEvent_t ev = fork_event();
    if (!ev || hipEventRecord(ev, s) != hipSuccess || hipStreamWaitEvent(ws_stream, ev, 0) != hipSuccess)
      return set_error("ms_conv_block_bwd_overlap: stream fork failed");
  }

  // 2. data gradient: transposed gather over dyr with wt[g][ci][co][khw]
  bool dx_done = false;
  if (dx && p.dg_clip) {
    // k3 s1 blocks whose reduction fits a workgroup: one launch of the clip-resident kernel (clip32.hip), no split-K slab
    const float* wp = wt_prepared;
    if (!wp) {
      rc = clip32_prep_queue(w, wt, d->Cin, d->Cout, d->KW, d->KW == 4 ? 2 : 1, d->Cin, s);
      if (!rc) rc = clip32_prep_flush(s);
      if (rc) return rc;
      wp = wt;
    }
    if (have_prev) {
      const Clip32PrevBN pv = {opt->prev_y, opt->prev_y_raw, opt->prev_save, opt->prev_gamma, opt->prev_dgamma, opt->prev_dbeta, opt->prev_dbias, opt->prev_slope};
      rc = clip32_block_dgrad(d, gr, wp, dx, dx2, s, &pv, fuse_part, opt->bn_sync, opt->bn_sync_words, opt->dx_accum);
      if (rc == -2) return set_error("ms_conv_block_bwd: the fused data gradient is not resident at once on this device");
    } else {
      rc = clip32_block_dgrad(d, gr, wp, dx, dx2, s, nullptr, nullptr, nullptr, 0, opt->dx_accum);
    }
    if (rc && rc != -2) return rc;
    // (the data-gradient paths below know nothing of dx_accum: a decline must not leave dx without it)
    if (rc == -2 && opt->dx_accum) return set_error("ms_conv_block_bwd: the clip-resident data gradient declined a launch with dx_accum");
    dx_done = rc == 0;
    rc = dx_done ? 0 : clip32_hold_flush(s);      // (a decline: in stream order behind a block the stream's hold may still hold)
    if (rc) return rc;
  }
  if (dx && !dx_done && p.dg_grouped) {
    // grouped decoder blocks: one clip of one group per workgroup, all 256 rows, weights streamed into registers (chain32.hip)
    const float* wp = wt_prepared;
    if (!wp) {
      rc = gdgrad32_prepare(d, w, wt, s);
      if (!rc) rc = gdgrad32_prep_flush(s);
      if (rc) return rc;
      wp = wt;
    }
    rc = gdgrad32_launch(d, gr, wp, dx, s);
    if (rc) return rc;
    dx_done = true;
  }
  if (dx && !dx_done) {
    // patch-staged path: each output-parity class is a dense stride-1 forward conv of dy_raw with the class's taps
    // reversed (weights prepared by transpose_weight_kernel(flip=1)); outputs are scattered with stride (SH, SW)
    const PatchPlan& pp0 = p.dpp;
    const int Kg2 = dg.tcog * dg.jh * dg.jw;
    const size_t dx_elems = (size_t)d->B * g.cin_tot * d->H * d->W;
    // stride-1 convs with whole 64-channel tiles: the patch kernel reads w in place, no transposed copy
    const bool direct = pp0.ok && !pp0.p6 && patch_dgrad_direct_ok(w, d->Cin, d->KH, d->KW, d->SH, d->SW, bcast);
    if (wt_prepared) {
      wt = const_cast<float*>(wt_prepared);      // built by ms_dgrad_weights_prepare for this very descriptor
    } else if (!direct) {
      rc = launch_transpose_weight(w, wt, dg.tg, dg.tcog, d->Cin, d->KH, d->KW, d->SH, d->SW, d->PH, d->PW, pp0.ok ? 1 : 0, s);
      if (rc) return rc;
    }
    if (pp0.ok) {
      // all output-parity classes in ONE launch (class 0 has the largest extent: its tiling serves the others)
      PatchArgs q = {};
      q.A = wt; q.src = gr; q.out = dx; q.out2 = dx2;
      q.Mg = d->Cin; q.Kg = Kg2; q.groups = dg.tg; q.Kc = dg.tcog; q.bcast = 0; q.a_vec = (Kg2 % 4 == 0);
      if (direct) { q.A = w; q.a_vec = 2; }
      q.ep = up2 ? EP_DGRAD_UP2 : EP_BARE; q.is_dgrad = 1;
      q.cls_a_stride = (unsigned)((size_t)dg.tg * d->Cin * Kg2);
      fill_src(q, plane_strides(g.one_d, d->B, C, d->OH, d->OW));
      fill_out(q, plane_strides(g.one_d, d->B, g.cin_tot, d->H, d->W));
      const double flops = fill_parity_classes(q, d, dg, g.one_d);
      // (the classes' outputs partition dx)
      const double bytes = 4.0 * ((double)dg.ncls * dg.tg * d->Cin * Kg2 + (double)d->B * C * hw) + 4.0 * (double)dx_elems;
      q.tiles_x = pp0.tiles_x; q.tiles_y = pp0.tiles_y;
      q.splitk = pp0.splitk; q.chunks_per_split = pp0.chunks_per_split;
      q.src_elems = (size_t)d->B * C * hw; q.a_elems = (size_t)dg.ncls * dg.tg * d->Cin * Kg2;
      if (pp0.splitk > 1) {
        q.part = dg_part; q.part_stride = dx_elems;
        q.ep = EP_BARE;               // partial tiles: plain full-resolution layout, the reduce kernel splits UP2
      }
      if (pp0.p6) {
        // bf16x6: planes of the transposed class slabs -- behind the prepared fp32 copy when the trainer built them
        // (ms_dgrad_weights_prepare), else split here
        const int re = patch6_row_elems(dg.tcog, dg.jh, dg.jw), rows = dg.ncls * dg.tg * d->Cin;
        const unsigned short* planes;
        if (wt_prepared) {
          planes = (const unsigned short*)(wt_prepared + align_up(p.wt_elems, 64));
        } else {
          unsigned short* mine = ws_at<unsigned short>(workspace, p.ws.dg_planes);
          rc = launch_split_weights(wt, mine, rows, dg.tcog, dg.jh, dg.jw, s);
          if (rc) return rc;
          planes = mine;
        }
        q.Aplanes = planes; q.plane_stride = (unsigned)((size_t)rows * re); q.a_row_elems = re;
        q.cls_a_stride = (unsigned)(dg.tg * d->Cin);
        rc = launch_patch6(q, pp0, dg.jh, dg.jw, 1, false, flops, bytes, s);
      } else {
        rc = launch_patch(q, pp0, dg.jh, dg.jw, 1, false, flops, bytes, s);
      }
      if (rc) return rc;
      if (pp0.splitk > 1) {
        rc = launch_splitk_dgrad_epilogue(dg_part, pp0.splitk, dx_elems, dx, dx2, dx_elems, d->W, up2 ? 1 : 0, s);
        if (rc) return rc;
      }
    } else {
      const GatherPlan& pl = p.dpl;
      GatherArgs a = {};
      a.A = wt; a.src = gr; a.out = dx; a.out2 = dx2;
      a.Mg = d->Cin; a.Kg = Kg2; a.groups = dg.tg; a.Kc = dg.tcog; a.src_ctotal = C;
      a.SRCH = d->OH; a.SRCW = d->OW; a.OUTH = d->H; a.OUTW = d->W; a.Npix = d->B * d->H * d->W; a.batch = d->B;
      a.KH = dg.jh; a.KW = dg.jw; a.SH = d->SH; a.SW = d->SW; a.PH = d->PH; a.PW = d->PW;
      a.bcast = 0;
      a.a_vec = (a.Kg % 4 == 0);
      a.ep = up2 ? EP_DGRAD_UP2 : EP_DGRAD;
      if (pl.splitk > 1) {
        a.part = dg_part;
        a.part_stride = dx_elems;
        a.ep = EP_DGRAD;               // partial tiles use the plain full-resolution layout
      }
      rc = launch_gather(a, true, up2, pl, s);
      if (rc) return rc;
      if (pl.splitk > 1) {
        rc = launch_splitk_dgrad_epilogue(dg_part, pl.splitk, dx_elems, dx, dx2, dx_elems, d->W, up2 ? 1 : 0, s);
        if (rc) return rc;
      }
    }
  }

  // 3. weight gradient
  if (dw && p.wg_c1) {
    // the single-input-channel 3x3 block: a stream over dy_raw on the vector unit (conv_c1.hip), slabs reduced like any split
    rc = launch_wgrad_c1(gr, x, wg_part, d->B, d->H, d->W, ws_stream);
    if (!rc && !defer_wgrad) rc = launch_reduce_splits(wg_part, dw, C * Kg, p.wg_splits, ws_stream);
    return rc;
  }
  if (dw && p.wp.ok) {
    const WgradPatchPlan& wp = p.wp;
    WgradPatchArgs q = {};
    q.dyr = gr; q.src = x; q.src2 = x2;
    q.out = wp.splits > 1 ? wg_part : dw;
    q.Cog = d->Cout; q.Cig = d->Cin; q.Kg = Kg; q.groups = d->groups; q.bcast = bcast;
    fill_src(q, plane_strides(g.one_d, d->B, g.cin_tot, d->H, d->W));
    fill_out(q, plane_strides(g.one_d, d->B, C, d->OH, d->OW));
    q.PH = g.one_d ? 0 : d->PH;
    q.PW = d->PW; q.tiles_x = wp.tiles_x; q.tiles_y = wp.tiles_y; q.n_tiles = wp.n_tiles;
    q.tiles_per_split = wp.tiles_per_split; q.splits = wp.splits;
    const double flops = 2.0 * d->Cout * q.Kg * (double)npix * d->groups;
    const double bytes = 4.0 * ((double)npix * C + (double)d->B * g.cin_tot * d->H * d->W + (double)C * q.Kg);
    if (wp.splits > 1 && !defer_wgrad && !wp.p6) {
      q.counters = counter_region(CNT_WGRAD, cdiv(q.Kg, 64) * cdiv(d->Cout, 64) * d->groups);
      q.final_out = dw;
    }
    // queued form (ms_wgrad_flush): only when nothing of this call reads the result -- dw written in place, or slabs left
    // for the caller's ms_wgrad_reduce_multi
    if (opt->defer_wgrad_launch && !wp.p6 && ws_stream == s && (wp.splits == 1 || defer_wgrad))
      return queue_wgrad_patch(q, wp, d->KH, d->KW, d->SW, up2, flops, bytes);
    rc = wp.p6 ? launch_wgrad_patch6(q, wp, d->KH, d->KW, d->SW, up2, flops, bytes, ws_stream)
               : launch_wgrad_patch(q, wp, d->KH, d->KW, d->SW, up2, flops, bytes, ws_stream);
    if (rc) return rc;
    if (wp.splits > 1 && !q.counters && !defer_wgrad) rc = launch_reduce_splits(wg_part, dw, C * q.Kg, wp.splits, ws_stream);
  } else if (dw) {
    WgradArgs a = {};
    a.dyr = gr; a.src = x; a.src2 = x2;
    a.Cog = d->Cout; a.Cig = d->Cin; a.Kg = Kg; a.groups = d->groups;
    a.src_ctotal = g.cin_tot;
    a.H = d->H; a.W = d->W; a.OH = d->OH; a.OW = d->OW; a.Npix = npix;
    a.KH = d->KH; a.KW = d->KW; a.SH = d->SH; a.SW = d->SW; a.PH = d->PH; a.PW = d->PW;
    a.bcast = bcast;
    rc = launch_wgrad(a, up2, dw, wg_part, defer_wgrad, ws_stream, opt->defer_wgrad_launch && ws_stream == s);
  }
  return rc;
}

int ms_clip_hold(void* stream) { return clip32_hold_arm((hipStream_t)stream); }
int ms_clip_hold_flush(void* stream) { return clip32_hold_flush((hipStream_t)stream); }
int ms_clip_hold_discard(void* stream) { clip32_hold_discard((hipStream_t)stream); return 0; }
int ms_clip_grid(const ms_conv_desc* d) {
  if (validate(d, "ms_clip_grid") || dt_of(d) != DT_F32 || g_precision != 0) return 0;
  return clip32_fwd_grid(d);
}
int ms_clip_pair_ok(const ms_conv_desc* host, const ms_conv_desc* guest) {
  if (validate(host, "ms_clip_pair_ok") || validate(guest, "ms_clip_pair_ok") || dt_of(host) != DT_F32 || dt_of(guest) != DT_F32 || g_precision != 0) return 0;
  return clip32_fwd_pair_ok(host, guest) ? 1 : 0;
}
int ms_clip_dgrad_grid(const ms_conv_desc* d) {
  if (validate(d, "ms_clip_dgrad_grid") || dt_of(d) != DT_F32 || g_precision != 0) return 0;
  return clip32_dgrad_grid(d);
}
int ms_clip_dgrad_pair_ok(const ms_conv_desc* host, const ms_conv_desc* guest) {
  if (validate(host, "ms_clip_dgrad_pair_ok") || validate(guest, "ms_clip_dgrad_pair_ok") || dt_of(host) != DT_F32 || dt_of(guest) != DT_F32 || g_precision != 0) return 0;
  return clip32_dgrad_pair_ok(host, guest) ? 1 : 0;
}
int ms_debug_set_clip_corun(int on) {
  const int prev = g_clip_corun < 0 ? 1 : g_clip_corun;
  g_clip_corun = on ? 1 : 0;
  return prev;
}
int ms_debug_set_clip_corun_bwd(int on) {
  const int prev = g_clip_corun_bwd < 0 ? 1 : g_clip_corun_bwd;
  g_clip_corun_bwd = on ? 1 : 0;
  return prev;
}

}  // extern "C"
