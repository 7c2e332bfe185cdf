// Host-side geometry shared by the two block dispatchers (api.hip: fp32 / bf16x6, api16.hip: bf16 / fp16).  No device code.
#pragma once
#include <algorithm>

#include "conv16.h"

namespace ms {

// What a descriptor implies for every kernel family.  C8 / cin8_tot: channel blocks of the cb8 layout (conv16.h).
struct BlockGeo { int dt, nd, one_d, up2, bcast, C, C8, cin_tot, cin8_tot, npix, hw, khw; };
inline BlockGeo geo_of(const ms_conv_desc* d) {
  BlockGeo g;
  g.dt = dt_of(d);
  g.nd = plan_nd_of(d);
  g.one_d = g.nd == 1;
  g.C = d->groups * d->Cout; g.C8 = c8_of(g.C);
  g.bcast = d->in_mode == MS_IN_BCAST; g.up2 = plan_up2_of(d);
  g.cin_tot = g.bcast ? d->Cin : d->groups * d->Cin; g.cin8_tot = c8_of(g.cin_tot);
  g.npix = d->B * d->OH * d->OW; g.hw = d->OH * d->OW; g.khw = d->KH * d->KW;
  return g;
}
inline size_t wsize_of(const ms_conv_desc* d) { return (size_t)d->groups * d->Cout * d->Cin * d->KH * d->KW; }

// (DgradGeo, dgrad_geo_of: conv16_plan.h)

// Per class: padding, output extent and scatter phase (class 0 has the largest extent: its values are the launch's own); the output
// scatter strides.  Returns the flops of all classes.  PatchArgs and Conv16Args share these field names.
template <class Args>
double fill_parity_classes(Args& q, const ms_conv_desc* d, const DgradGeo& dg, bool one_d) {
  double flops = 0;
  q.ncls = dg.ncls;
  for (int cls = 0; cls < dg.ncls; ++cls) {
    const int ry = cls / d->SW, rx = cls - ry * d->SW;
    const int kh0 = (ry + d->PH) % d->SH, kw0 = (rx + d->PW) % d->SW;
    const int cy = (ry + d->PH - kh0) / d->SH, cx = (rx + d->PW - kw0) / d->SW;
    const int QH = std::max(0, (d->H - ry + d->SH - 1) / d->SH), QW = std::max(0, (d->W - rx + d->SW - 1) / d->SW);
    q.cls_PH[cls] = one_d ? 0 : (dg.jh - 1) - cy; q.cls_PW[cls] = (dg.jw - 1) - cx;
    q.cls_OUTH[cls] = one_d ? d->B : QH; q.cls_OUTW[cls] = QW;
    q.cls_ry[cls] = one_d ? 0 : ry; q.cls_rx[cls] = rx;
    flops += 2.0 * d->Cin * dg.tcog * dg.jh * dg.jw * (double)d->B * (one_d ? 1 : QH) * QW * dg.tg;
  }
  q.PH = q.cls_PH[0]; q.PW = q.cls_PW[0]; q.OUTH = q.cls_OUTH[0]; q.OUTW = q.cls_OUTW[0]; q.o_ry = q.cls_ry[0]; q.o_rx = q.cls_rx[0];
  q.o_sh = one_d ? 1 : d->SH; q.o_sw = d->SW;
  return flops;
}

// A (B, ch, H, W) tensor as the patch-staged kernels walk it.  1-D blocks: the batch is the row axis of ONE image; 2-D: image
// strides.  ch counts elements for the fp32 tensors and 16-byte vectors (channel blocks) for cb8.
struct PlaneStrides { int rows, cols, img, chan, row; };
inline PlaneStrides plane_strides(bool one_d, int B, int ch, int H, int W) {
  return one_d ? PlaneStrides{B, W, 0, W, ch * W} : PlaneStrides{H, W, ch * H * W, H * W, W};
}
// ... into the source / output fields of PatchArgs and WgradPatchArgs (s_chan) and of Conv16Args and Wgrad16Args (s_cblk)
template <class Args> void fill_src(Args& q, const PlaneStrides& p) { q.SRCH = p.rows; q.SRCW = p.cols; q.s_img = p.img; q.s_chan = p.chan; q.s_row = p.row; }
template <class Args> void fill_out(Args& q, const PlaneStrides& p) { q.OUTH = p.rows; q.OUTW = p.cols; q.o_img = p.img; q.o_chan = p.chan; q.o_row = p.row; }
template <class Args> void fill_src8(Args& q, const PlaneStrides& p) { q.SRCH = p.rows; q.SRCW = p.cols; q.s_img = p.img; q.s_cblk = p.chan; q.s_row = p.row; }
template <class Args> void fill_out8(Args& q, const PlaneStrides& p) { q.OUTH = p.rows; q.OUTW = p.cols; q.o_img = p.img; q.o_cblk = p.chan; q.o_row = p.row; }

// Scratch layouts are built by appending regions: returns the region's offset and advances the running total.
inline size_t carve(size_t& total, size_t bytes) { const size_t at = total; total += bytes; return at; }
template <class T> T* ws_at(void* base, size_t off) { return (T*)((char*)base + off); }

}  // namespace ms
