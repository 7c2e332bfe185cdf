// 16-bit arithmetic mode (desc.dtype = MS_BF16 / MS_F16): one conv block forward / backward on cb8 tensors, reached from the
// ms_conv_block_* entry points of api.hip, plus the batched weight preparation (ms_weights16_prepare).
#include "block_geom.h"

namespace ms {

namespace {

// (the arithmetic: conv16_plan.h, where tests/helpers/conv16_plan_host.cpp reads it too)
Conv16Plan fwd_plan16(const ms_conv_desc* d) { return fwd_plan16_of(d); }
struct Dgrad16 : DgradGeo { Conv16Plan pl; };
Dgrad16 dgrad_plan16(const ms_conv_desc* d) {
  Dgrad16 r;
  static_cast<DgradGeo&>(r) = dgrad_geo_of(d);
  r.pl = dgrad_plan16_of(d, r);
  return r;
}
Wgrad16Plan wgrad_plan16(const ms_conv_desc* d) { return wgrad_plan16_of(d); }
size_t fwd_a_bytes(const ms_conv_desc* d, const Conv16Plan& pl) {
  return conv16_weight_bytes(pl, d->Cout, d->groups, d->Cin, d->KH, d->KW, 1);
}
size_t dgrad_a_bytes(const ms_conv_desc* d, const Dgrad16& dg) {
  return conv16_weight_bytes(dg.pl, d->Cin, dg.tg, dg.tcog, dg.jh, dg.jw, dg.ncls);
}

Prep16Job fwd_job(const ms_conv_desc* d, const Conv16Plan& pl, const float* w, void* out, const float* scale) {
  Prep16Job jb = {};
  jb.w = w; jb.out = out; jb.scale = scale; jb.dgrad = 0;
  jb.groups = d->groups; jb.Cog = d->Cout; jb.Cig = d->Cin; jb.KH = d->KH; jb.KW = d->KW; jb.SH = d->SH; jb.SW = d->SW;
  jb.PH = d->PH; jb.PW = d->PW; jb.bcast = d->in_mode == MS_IN_BCAST;
  jb.BM = 64 * pl.wm; jb.CK8 = pl.ck8; jb.nchunks = pl.nchunks; jb.n_mt = cdiv(d->Cout, jb.BM); jb.dt = dt_of(d);
  return jb;
}
Prep16Job dgrad_job(const ms_conv_desc* d, const Dgrad16& dg, const float* w, void* out) {
  Prep16Job jb = fwd_job(d, dg.pl, w, out, nullptr);
  jb.dgrad = 1;
  jb.n_mt = cdiv(d->Cin, jb.BM);
  return jb;
}

// partial statistics of the in-launch BatchNorm: one (sum, M2, count, 0) per tile and (padded) channel
size_t bn_part_bytes(const ms_conv_desc* d, const Conv16Plan& pl) {
  const int bm = 64 * pl.wm;
  return align_up((size_t)pl.n_tiles * cdiv(d->Cout, bm) * d->groups * bm * 16, 256);
}

}  // namespace

size_t weights16_bytes(const ms_conv_desc* d, int which) {
  if (which == 0) {
    const Conv16Plan pl = fwd_plan16(d);
    if (!pl.ok) return 0;
    size_t b = align_up(fwd_a_bytes(d, pl), 256);
    if (bn_folded_of(d)) b += align_up((size_t)2 * d->groups * d->Cout * sizeof(float), 256);   // folded scale | bias
    return b;
  }
  const Dgrad16 dg = dgrad_plan16(d);
  return dg.pl.ok ? align_up(dgrad_a_bytes(d, dg), 256) : 0;
}

int wgrad16_splits(const ms_conv_desc* d) {
  const Wgrad16Plan wp = wgrad_plan16(d);
  return wp.tp ? wp.splits : 1;
}

namespace {

// Scratch of the forward, byte offsets, regions in this order: tile statistics | tile counts | partials of the in-launch BatchNorm
// (BN_TRAIN) | per-call weight preparation: the A operand (a whole ms_weights16_bytes buffer) | folded scale, bias'
struct Fwd16Layout { size_t stats, counts, bn_part, A, fold, total; };
Fwd16Layout fwd16_layout(const ms_conv_desc* d, const Conv16Plan& pl) {
  Fwd16Layout l = {};
  if (pl.ok) {
    const int C = d->groups * d->Cout;
    l.stats = carve(l.total, align_up((size_t)pl.n_tiles * C * 2 * sizeof(float), 256));
    l.counts = carve(l.total, align_up((size_t)pl.n_tiles * sizeof(float), 256));
    l.bn_part = carve(l.total, d->mode == MS_BN_TRAIN ? bn_part_bytes(d, pl) : 0);
    l.A = carve(l.total, weights16_bytes(d, 0));
    l.fold = carve(l.total, align_up((size_t)2 * C * sizeof(float), 256));
  }
  l.total += 256;
  return l;
}

// ... and of the backward: BatchNorm partials | column sums | per-call data-gradient operand | weight-gradient slabs (splits > 1)
struct Bwd16Layout { size_t bn_part, colpart, wt, wg_part, total; int nchunk; };
Bwd16Layout bwd16_layout(const ms_conv_desc* d) {
  const BlockGeo g = geo_of(d);
  Bwd16Layout l = {};
  int bpc;
  l.nchunk = bwd16_chunks(d->B, g.C8, g.hw, &bpc);
  l.bn_part = carve(l.total, align_up((size_t)g.C8 * 8 * l.nchunk * 2 * sizeof(float), 256));
  l.colpart = carve(l.total, align_up((size_t)g.C8 * 8 * l.nchunk * sizeof(float), 256));
  l.wt = carve(l.total, weights16_bytes(d, 1));
  const int sp = wgrad16_splits(d);
  l.wg_part = carve(l.total, sp > 1 ? align_up((size_t)sp * wsize_of(d) * sizeof(float), 256) : 0);
  l.total += 256;
  return l;
}

}  // namespace

size_t block_fwd16_workspace(const ms_conv_desc* d) { return fwd16_layout(d, fwd_plan16(d)).total; }
size_t block_bwd16_workspace(const ms_conv_desc* d) { return bwd16_layout(d).total; }

// MS_DT_STAT_PAIR in the 16-bit modes: the conv leaves its tile statistics (EP_RAW_STATS) and the normalising launch combines them
// per half of the batch (bn_finalize_apply16_kernel) -- needs whole statistics tiles per half, at most 32 of them, a cb8 output,
// and the one-launch BatchNorm backward
bool stat_pair16_ok(const ms_conv_desc* d) {
  if (d->mode != MS_BN_TRAIN) return true;
  if ((d->B & 1) || out_f32_of(d)) return false;
  const BlockGeo g = geo_of(d);
  const Conv16Plan pl = fwd_plan16(d);
  if (!pl.ok || (pl.n_tiles & 1) || pl.n_tiles > 64) return false;
  if (g.one_d && ((d->B / 2) % pl.th)) return false;          // (1-D: the batch is the row axis of one image; 2-D: tiles per image)
  return (long)d->B / 2 * g.hw <= BN_BWD16_FUSED_MAX;
}

// The data-gradient launch adds ms_bwd_options.dx_accum itself: plain input (dx is one cb8 tensor of the input's shape -- the upsample-add
// form writes two, the broadcast form sums the groups), and a kernel for the geometry.  1-D and 2-D, any stride, grouped or not.
bool dgrad16_takes_accum(const ms_conv_desc* d) {
  if (dt_of(d) != DT_BF16 && dt_of(d) != DT_F16) return false;
  return d->in_mode == MS_IN_PLAIN && dgrad_plan16(d).pl.ok != 0;
}

int block_fwd16(const ms_conv_desc* d, const void* x, const void* x2, const float* w, const float* bias, const float* gamma,
                const float* beta, float* running_mean, float* running_var, void* y_raw, void* y, float* save, void* workspace,
                size_t workspace_bytes, hipStream_t s, const void* w_prepared, int32_t* bn_sync, int bn_sync_words) {
  const BlockGeo g = geo_of(d);
  if (g.dt != DT_BF16 && g.dt != DT_F16) return set_error("ms_conv_block_fwd: dtype %d", d->dtype);
  if (d->mode == MS_BN_EVAL && (d->dtype & MS_DT_BN_FROZEN)) {
    // frozen BatchNorm, the differentiable form (api.hip checked y_raw / save / workspace): the conv as its MS_BARE launch into the
    // cb8 y_raw, then ONE launch that writes `save` from the running statistics, normalises and activates (cb8, or fp32 with
    // MS_DT_OUT_F32).  No statistics groups: MS_DT_STAT_PAIR is a plain batch of B.
    if (workspace_bytes < block_fwd16_workspace(d)) return set_error("ms_conv_block_fwd: workspace too small");
    ms_conv_desc bare = *d;
    bare.mode = MS_BARE;
    bare.dtype &= ~(MS_DT_STAT_PAIR | MS_DT_BN_FROZEN | MS_DT_OUT_F32);
    const int rc = block_fwd16(&bare, x, x2, w, bias, nullptr, nullptr, nullptr, nullptr, nullptr, y_raw, nullptr, workspace, workspace_bytes, s,
                               w_prepared, bn_sync, bn_sync_words);
    if (rc) return rc;
    const bool f32 = out_f32_of(d);
    return launch_bn_apply16_frozen(g.dt, y_raw, f32 ? nullptr : y, f32 ? (float*)y : nullptr, save, gamma, beta, running_mean, running_var,
                                    d->eps, d->B, g.C, g.hw, d->slope, s);
  }
  if (d->mode == MS_BN_TRAIN && sg_of(d) > 1 && !stat_pair16_ok(d))
    return set_error("ms_conv_block_fwd: MS_DT_STAT_PAIR is not implemented for this 16-bit block (ms_stat_pair_ok)");
  if (!bn_sync) { bn_sync = g_bn_sync; bn_sync_words = g_bn_sync_n; }      // (the process-wide buffer of ms_set_bn_sync_buffer)
  const Conv16Plan pl = fwd_plan16(d);
  if (!pl.ok) return set_error("ms_conv_block_fwd: no 16-bit kernel for a %dx%d stride (%d,%d) block", d->KH, d->KW, d->SH, d->SW);
  if (d->groups > 1 && ((d->Cout & 7) || (!g.bcast && (d->Cin & 7))))
    return set_error("ms_conv_block_fwd: 16-bit grouped blocks need channels per group %% 8 == 0");
  const Fwd16Layout ws = fwd16_layout(d, pl);
  if (workspace_bytes < ws.total) return set_error("ms_conv_block_fwd: workspace too small");
  const bool outf32 = out_f32_of(d);
  float* stats = ws_at<float>(workspace, ws.stats);
  float* counts = ws_at<float>(workspace, ws.counts);
  float* bn_part = d->mode == MS_BN_TRAIN ? ws_at<float>(workspace, ws.bn_part) : nullptr;
  // the single-input-channel 3x3 block (AudioEncoder conv.0): vector-unit kernel, no operand preparation
  // (train mode stays on the matrix-pipe kernel: with the tile statistics the vector-unit kernel is the slower one, 46 vs 35 us;
  // eval mode -- the D-step's generator pass -- 41 -> 28.5 us)
  if (conv16_c1_ok(d) && d->mode != MS_BN_TRAIN && !outf32 && conv16_c1_tiles(d) <= pl.n_tiles && w && (!bn_folded_of(d) || w_prepared)) {
    // inference with eval BatchNorm folded: the prepared buffer carries scale | bias' behind the operand stages (the same values the
    // matrix-pipe path folds into its weights and adds in its epilogue); what is left of the block is the activation
    const bool fold = bn_folded_of(d);
    const float* fscale = fold ? (const float*)((const char*)w_prepared + align_up(fwd_a_bytes(d, pl), 256)) : nullptr;
    const int ep = d->mode == MS_BARE ? EP_BARE : (d->mode == MS_LRELU || fold) ? EP_LRELU : EP_BN_EVAL;
    return launch_conv16_c1(g.dt, x, w, fscale, fold ? fscale + g.C : bias, y, gamma, beta, running_mean, running_var, stats, counts,
                            d->B, d->H, d->W, ep, d->slope, d->eps, s);
  }
  const size_t a_bytes = align_up(fwd_a_bytes(d, pl), 256);
  const void* A = w_prepared;
  const float* bias_use = bias;
  int rc;
  const bool folded = bn_folded_of(d);
  if (w_prepared) {
    if (folded) bias_use = (const float*)((const char*)w_prepared + a_bytes) + g.C;
  } else {
    float* fold = ws_at<float>(workspace, ws.fold);        // scale | bias'
    const float* scale = nullptr;
    if (folded) {
      rc = launch_bn_fold(bias, gamma, beta, running_mean, running_var, fold, fold + g.C, g.C, d->eps, s);
      if (rc) return rc;
      scale = fold; bias_use = fold + g.C;
    }
    Prep16Batch pb;
    void* mine = ws_at<void>(workspace, ws.A);
    pb.n = 1; pb.job[0] = fwd_job(d, pl, w, mine, scale);
    rc = launch_prep16_multi(pb, s);
    if (rc) return rc;
    A = mine;
  }
  Conv16Args a = {};
  a.A = A; a.src = x; a.src2 = x2;
  a.out = d->mode == MS_BN_TRAIN ? y_raw : y;
  a.bias = bias_use; a.stats = stats; a.counts = counts;
  a.Mg = d->Cout; a.groups = d->groups; a.Kc8g = c8_of(d->Cin); a.bcast = g.bcast;
  // eval BatchNorm: either folded into the prepared weights and bias (inference: what is left is the activation), or applied
  // from the running statistics in the epilogue (eval passes inside training, whose statistics move between calls)
  a.ep = d->mode == MS_BARE ? EP_BARE : d->mode == MS_BN_TRAIN ? EP_RAW_STATS : (d->mode == MS_LRELU || folded) ? EP_LRELU : EP_BN_EVAL;
  a.bn_g = gamma; a.bn_b = beta; a.bn_m = running_mean; a.bn_v = running_var;
  a.KH = d->KH; a.S = d->SW; a.SV = g.one_d ? 1 : d->SH;
  fill_src8(a, plane_strides(g.one_d, d->B, g.cin8_tot, d->H, d->W));
  fill_out8(a, plane_strides(g.one_d, d->B, g.C8, d->OH, d->OW));
  const PlaneStrides of = plane_strides(g.one_d, d->B, g.C, d->OH, d->OW);      // the fp32 output: element strides
  a.of_img = of.img; a.of_chan = of.chan; a.of_row = of.row;
  a.PH = g.one_d ? 0 : d->PH; a.PW = d->PW; a.o_sh = 1; a.o_sw = 1;
  a.slope = d->slope; a.eps = d->eps;
  if (outf32 && d->mode != MS_BN_TRAIN) a.out_f32 = (float*)y;
  // train-mode BatchNorm inside the conv launch (conv16_kernel.h, EP_BN_FUSED): the workgroups of a channel tile exchange
  // their partial statistics and normalise from registers -- taken when the whole grid is resident at once
  bool fused = false;
  const int sg = d->mode == MS_BN_TRAIN ? sg_of(d) : 1;
  if (d->mode == MS_BN_TRAIN && !outf32 && g_bn_fused && bn_sync && sg == 1) {
    const int bm = 64 * pl.wm, gy = cdiv(d->Cout, bm), nwg = pl.n_tiles * gy * d->groups;
    const int scratch = (pl.nwn * bm * 4 + (128 * pl.nwn / bm) * bm * 3 * 2 + bm * 2 + bm / 8 + pl.nwn + 1) * 4;      // red | dred | scsh | rawflag | wcnt
    // (every workgroup reads its group's n_tiles partials: beyond 64 tiles per channel tile that traffic -- n_tiles^2 x 1 KB per
    // channel tile -- costs more than the normalising launch it replaces; measured on the 512-tile audio-encoder layers)
    fused = pl.n_tiles <= 64 && nwg >= g_bn_fused_min_wgs && (1 + gy * d->groups) * BNF_SYNC_WORDS_PER_GROUP <= bn_sync_words &&
            pl.lds_bytes >= scratch &&
            conv16_coresident(g.dt, pl, d->KW, g.up2 != 0, nwg);
  }
  if (fused) {
    a.ep = EP_BN_FUSED; a.out = y; a.out_raw = y_raw; a.bn_part = bn_part; a.bn_sync = bn_sync; a.save = save;
    a.momentum = d->momentum;
    a.raw_all = (long)d->B * g.hw > BN_BWD16_FUSED_MAX;      // its two-pass backward reads y_raw for the blocks y does not invert
  }
  const double esz = 2.0;
  const double flops = 2.0 * d->Cout * d->Cin * d->KH * d->KW * (double)g.npix * d->groups;
  const double bytes = esz * ((double)g.C * d->Cin * d->KH * d->KW + (double)d->B * g.cin_tot * d->H * d->W) +
                       (a.out_f32 ? 4.0 : esz) * (double)g.npix * g.C;
  rc = launch_conv16(g.dt, a, pl, d->KW, g.up2 != 0, flops, bytes, s);          // (bytes: algorithmic |x| + |w| + |y| of the block)
  if (rc || fused) return rc;
  if (d->mode == MS_BN_TRAIN && pl.n_tiles <= 64)      // few statistics tiles: finalize inside the normalising launch
    return launch_bn_finalize_apply16(g.dt, stats, counts, pl.n_tiles, g.npix, gamma, beta, running_mean, running_var, save, d->eps,
                                      d->momentum, y_raw, outf32 ? nullptr : y, outf32 ? (float*)y : nullptr, d->B, g.C, g.hw,
                                      d->slope, s, sg);
  if (d->mode == MS_BN_TRAIN) {
    rc = launch_bn_finalize(stats, counts, pl.n_tiles, 0, g.npix, g.C, gamma, beta, running_mean, running_var, save, d->eps,
                            d->momentum, s);
    if (rc) return rc;
    rc = launch_bn_apply16(g.dt, y_raw, outf32 ? nullptr : y, outf32 ? (float*)y : nullptr, save, d->B, g.C, g.hw, d->slope, s);
  }
  return rc;
}

int block_bwd16(const ms_conv_desc* d, const void* x, const void* x2, const float* w, const float* gamma, const void* y_raw,
                const void* y, const float* save, const void* dy, void* dyr, void* dx, void* dx2, float* dw, float* dbias,
                float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, hipStream_t s, const void* wt_prepared,
                float* wgrad_partials, int defer_wgrad_launch, const void* dx_accum) {
  const BlockGeo g = geo_of(d);
  if (g.dt != DT_BF16 && g.dt != DT_F16) return set_error("ms_conv_block_bwd: dtype %d", d->dtype);
  const Bwd16Layout ws = bwd16_layout(d);
  if (workspace_bytes < ws.total) return set_error("ms_conv_block_bwd: workspace too small");
  const bool outf32 = out_f32_of(d);
  if (outf32 && d->mode == MS_LRELU) return set_error("ms_conv_block_bwd: fp32 outputs are for BARE and BatchNorm blocks");
  float* bn_part = ws_at<float>(workspace, ws.bn_part);
  float* colpart = ws_at<float>(workspace, ws.colpart);
  void* wt_ws = ws_at<void>(workspace, ws.wt);
  float* wg_part = ws_at<float>(workspace, ws.wg_part);
  int rc = 0;

  // 1. gradient wrt the raw conv output (+ per-channel column sums = bias gradient)
  const void* gsrc = dy;
  const float* dyf = outf32 ? (const float*)dy : nullptr;
  int bias_done = 0;
  if (d->mode == MS_BN_TRAIN) {
    // (y: blocks with a cb8 output read x_hat and the activation mask from it wherever the map inverts safely -- conv16.h)
    rc = launch_bn_bwd16(g.dt, outf32 ? nullptr : dy, dyf, y_raw, outf32 ? nullptr : y, save, gamma, bn_part, dyr, colpart, dbias, dgamma, dbeta, d->B, g.C,
                         g.hw, d->slope, &bias_done, s, sg_of(d));
    gsrc = dyr;
  } else if (d->mode == MS_BN_EVAL) {
    // frozen BatchNorm: `save` holds the running statistics (block_fwd16), y_raw is whole
    rc = launch_bn_bwd16(g.dt, outf32 ? nullptr : dy, dyf, y_raw, nullptr, save, gamma, bn_part, dyr, colpart, dbias, dgamma, dbeta, d->B, g.C,
                         g.hw, d->slope, &bias_done, s, 1, true);
    gsrc = dyr;
  } else if (d->mode == MS_LRELU) {
    rc = launch_act_bwd16(g.dt, dy, nullptr, y, dyr, colpart, d->B, g.C, g.hw, 1, d->slope, s);
    gsrc = dyr;
  } else if (dbias || outf32) {
    rc = launch_act_bwd16(g.dt, outf32 ? nullptr : dy, dyf, nullptr, dyr, colpart, d->B, g.C, g.hw, 0, 0.f, s);
    if (outf32) gsrc = dyr;
  }
  if (rc) return rc;
  if (dbias && !bias_done) {
    rc = launch_colsum16(colpart, dbias, g.C, ws.nchunk, s);
    if (rc) return rc;
  }

  // 2. data gradient: each output-parity class is a dense stride-1 forward conv of dy_raw with the class's taps reversed
  if (dx) {
    const Dgrad16 dg = dgrad_plan16(d);
    if (!dg.pl.ok) return set_error("ms_conv_block_bwd: no 16-bit data-gradient kernel for this geometry");
    const void* A = wt_prepared;
    if (!A) {
      Prep16Batch pb;
      pb.n = 1; pb.job[0] = dgrad_job(d, dg, w, wt_ws);
      rc = launch_prep16_multi(pb, s);
      if (rc) return rc;
      A = wt_ws;
    }
    Conv16Args q = {};
    q.A = A; q.src = gsrc; q.out = dx; q.out2 = dx2;
    q.Mg = d->Cin; q.groups = dg.tg; q.Kc8g = c8_of(dg.tcog); q.bcast = 0;
    // dx_accum: the input's other consumer's gradient (cb8, dx's own layout) joins the fp32 accumulators in the epilogue
    q.ep = g.up2 ? EP_DGRAD_UP2 : dx_accum ? EP_DGRAD_ACC : EP_BARE; q.is_dgrad = 1;
    q.acc = dx_accum;
    q.KH = dg.jh; q.S = 1; q.SV = 1;
    fill_src8(q, plane_strides(g.one_d, d->B, g.C8, d->OH, d->OW));
    fill_out8(q, plane_strides(g.one_d, d->B, g.cin8_tot, d->H, d->W));
    const double flops = fill_parity_classes(q, d, dg, g.one_d);
    q.slope = d->slope; q.eps = d->eps;
    const double bytes = 2.0 * ((double)g.C * d->Cin * d->KH * d->KW + (double)d->B * g.C * g.hw +
                                (dx_accum ? 2.0 : 1.0) * (double)d->B * g.cin_tot * d->H * d->W);
    rc = launch_conv16(g.dt, q, dg.pl, dg.jw, false, flops, bytes, s);
    if (rc) return rc;
  }

  // 3. weight gradient
  if (dw) {
    const Wgrad16Plan wp = wgrad_plan16(d);
    if (!wp.tp) return set_error("ms_conv_block_bwd: no 16-bit weight-gradient kernel for this geometry");
    const size_t wsize = wsize_of(d);
    Wgrad16Args a = {};
    a.dyr = gsrc; a.src = x; a.src2 = x2;
    const bool defer = wgrad_partials != nullptr && wp.splits > 1;
    a.out = wp.splits > 1 ? (defer ? wgrad_partials : wg_part) : dw;
    a.out_split_stride = wsize;
    a.Cog = d->Cout; a.Cig = d->Cin; a.groups = d->groups; a.bcast = g.bcast;
    a.KH = d->KH; a.KW = d->KW; a.S = d->SW; a.SV = g.one_d ? 1 : d->SH; a.PW = d->PW;
    fill_src8(a, plane_strides(g.one_d, d->B, g.cin8_tot, d->H, d->W));
    fill_out8(a, plane_strides(g.one_d, d->B, g.C8, d->OH, d->OW));
    a.PH = g.one_d ? 0 : d->PH;
    const double flops = 2.0 * d->Cout * d->Cin * d->KH * d->KW * (double)g.npix * d->groups;
    const double bytes = 2.0 * ((double)g.npix * g.C + (double)d->B * g.cin_tot * d->H * d->W) + 4.0 * (double)wsize;
    // queued form: only when nothing of this call reads the result (dw written in place, or slabs left for the caller)
    if (defer_wgrad_launch && (wp.splits == 1 || defer) && !wgrad16_c1_ok(a, g.up2 != 0)) return queue_wgrad16(g.dt, a, wp, g.up2 != 0, flops, bytes);
    rc = launch_wgrad16(g.dt, a, wp, g.up2 != 0, flops, bytes, s);
    if (rc) return rc;
    if (wp.splits > 1 && !defer) rc = launch_reduce_splits(wg_part, dw, (int)wsize, wp.splits, s);
  }
  return rc;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_wgrad_flush(void* stream) {
  const int rc = wgrad_patch_flush((hipStream_t)stream);
  const int rcg = wgrad_gather_flush((hipStream_t)stream);
  const int rc16 = wgrad16_flush((hipStream_t)stream);
  return rc ? rc : rcg ? rcg : rc16;
}
int ms_wgrad_discard(void) { wgrad_patch_discard(); wgrad_gather_discard(); wgrad16_discard(); return 0; }

int ms_set_bn_sync_buffer(int32_t* zeroed_words, int n) {
  g_bn_sync = zeroed_words;
  g_bn_sync_n = zeroed_words ? n : 0;
  return 0;
}
int ms_debug_set_bn_fused(int on) {
  const int prev = g_bn_fused;
  g_bn_fused = on ? 1 : 0;
  return prev;
}
int ms_debug_set_bn_fused_min_workgroups(int n) {
  const int prev = g_bn_fused_min_wgs;
  g_bn_fused_min_wgs = n < 0 ? 0 : n;
  return prev;
}

size_t ms_weights16_bytes(const ms_conv_desc* d, int which) {
  if (!d || (dt_of(d) != DT_BF16 && dt_of(d) != DT_F16) || (which != 0 && which != 1)) return 0;
  return weights16_bytes(d, which);
}

int ms_weights16_prepare(int n, const ms_prep16_item* items, void* stream) {
  if (n < 0 || (n && !items)) return set_error("ms_weights16_prepare: null argument");
  hipStream_t s = (hipStream_t)stream;
  Prep16Batch pb;
  pb.n = 0;
  auto flush = [&]() -> int {
    const int rc = pb.n ? launch_prep16_multi(pb, s) : 0;
    pb.n = 0;
    return rc;
  };
  for (int i = 0; i < n; ++i) {
    const ms_prep16_item& it = items[i];
    const ms_conv_desc* d = it.desc;
    if (!d || !it.w) return set_error("ms_weights16_prepare: item %d: null descriptor or weights", i);
    if (dt_of(d) != DT_BF16 && dt_of(d) != DT_F16) return set_error("ms_weights16_prepare: item %d is not a 16-bit block", i);
    int rc;
    if (it.fwd) {
      const Conv16Plan pl = fwd_plan16(d);
      if (!pl.ok) return set_error("ms_weights16_prepare: item %d: geometry not supported", i);
      const float* scale = nullptr;
      if (bn_folded_of(d)) {
        if (!it.gamma || !it.beta || !it.running_mean || !it.running_var) return set_error("ms_weights16_prepare: item %d: BN tensors missing", i);
        const int C = d->groups * d->Cout;
        float* fold = ws_at<float>(it.fwd, align_up(fwd_a_bytes(d, pl), 256));
        rc = launch_bn_fold(it.bias, it.gamma, it.beta, it.running_mean, it.running_var, fold, fold + C, C, d->eps, s);
        if (rc) return rc;
        scale = fold;
      }
      pb.job[pb.n++] = fwd_job(d, pl, it.w, it.fwd, scale);
      if (pb.n == PREP16_BATCH_MAX && (rc = flush())) return rc;
    }
    if (it.dgrad) {
      const Dgrad16 dg = dgrad_plan16(d);
      if (!dg.pl.ok) return set_error("ms_weights16_prepare: item %d: data-gradient geometry not supported", i);
      pb.job[pb.n++] = dgrad_job(d, dg, it.w, it.dgrad);
      if (pb.n == PREP16_BATCH_MAX && (rc = flush())) return rc;
    }
  }
  return flush();
}

}  // extern "C"
