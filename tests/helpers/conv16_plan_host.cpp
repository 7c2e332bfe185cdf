// Host driver of csrc/conv16_plan.h for tests/test_conv16_plan_table_cpu.py and tests/test_gpu_conv16_plans.py: no GPU, no Python.
// Reads one block per line from stdin
//   <id> <nd> <B> <cin> <cout> <groups> <KH> <KW> <SH> <SW> <PH> <PW> <H> <W> <in_mode>      (channels per group; in_mode 0 plain, 1 bcast, 2 up2)
// and prints three lines per block, the planner's own choice (no knob is set: the globals below hold the library's defaults):
//   <id> fwd   ok=.. KW=.. wm=.. wn=.. nwn=.. up2=.. dma=.. ckx=.. nstg=.. nstages=.. wait=.. form=.. refill=.. tiles=.. bm=.. bn=.. tw=..
//              r_rows=.. r_ow=.. r_mg=.. r_k=..
//   <id> dgrad (the same fields; KW = taps per row of one parity class)
//   <id> wgrad ok=.. tp=.. up2=.. npxt=.. nstg=.. splits=.. one=.. c1=.. tiles=.. tw=..
// wait = (nstg - 2) * (NA + npd), the count of conv16_kernel's steady-state s_waitcnt; form: lit (a loop of its own with the literal),
// run (the run-time 64-way switch), over (above 63: the switch's default, vmcnt(0)), none (register-staged: no ring).
// refill: the ring is refilled inside the K loop (nstages + 1 > nstg).  r_*: ragged bits -- rows % TH, OW % TW, Mg % BM, reduction
// channels not a multiple of the stage's 8 * CK8.
#include <cstdio>
#include <cstring>

#include "conv16_plan.h"

namespace ms {
int g_conv16_force_wm = 0, g_conv16_force_wn = 0, g_conv16_dma = CONV16_DMA_DEFAULT, g_conv16_wide8 = 0, g_conv16_ring = 0,
    g_conv16_big_stages = CONV16_BIG_STAGES_DEFAULT;
int g_wgrad16_ring = WGRAD16_RING_DEFAULT, g_wgrad16_target_wgs = WGRAD16_TARGET_WGS_DEFAULT;
}  // namespace ms

// the K loop's literal wait counts: the list conv16_kernel.h builds its loops from
static bool literal_wait(int w) {
#define MS_IS_LIT(N) if (w == N) return true;
  CONV16_WAIT_LITERALS(MS_IS_LIT)
#undef MS_IS_LIT
  return false;
}

static void print_conv(const char* id, const char* dir, const ms::Conv16Plan& pl, int KH, int KW, bool up2, int rows, int OW, int Mg, int Kc) {
  if (!pl.ok) {
    printf("%s %s ok=0\n", id, dir);
    return;
  }
  const int bm = 64 * pl.wm, nt = 128 * pl.nwn, bn = 32 * pl.wn * pl.nwn;
  const int ckx = pl.ck8 / ms::conv16_ck8(KW), nstages = pl.nchunks * KH;
  const int na = (KW * pl.ck8 * bm) / nt, npd = ms::cdiv(pl.ck8 * pl.th * pl.pc, nt);
  const int wait = pl.dma ? (pl.nstg - 2) * (na + npd) : -1;
  const char* form = !pl.dma ? "none" : literal_wait(wait) ? "lit" : wait <= 63 ? "run" : "over";
  printf("%s %s ok=1 KW=%d wm=%d wn=%d nwn=%d up2=%d dma=%d ckx=%d nstg=%d nstages=%d wait=%d form=%s refill=%d tiles=%d bm=%d bn=%d tw=%d "
         "r_rows=%d r_ow=%d r_mg=%d r_k=%d\n",
         id, dir, KW, pl.wm, pl.wn, pl.nwn, up2 ? 1 : 0, pl.dma, ckx, pl.dma ? pl.nstg : 0, nstages, wait, form,
         pl.dma ? (nstages + 1 > pl.nstg ? 1 : 0) : 0, pl.n_tiles, bm, bn, pl.tw, rows % pl.th != 0, OW % pl.tw != 0, Mg % bm != 0,
         Kc % (8 * pl.ck8) != 0);
}

int main() {
  char line[512], id[128];
  while (fgets(line, sizeof line, stdin)) {
    if (line[0] == '\n' || line[0] == '#') continue;
    int nd, B, cin, cout, groups, KH, KW, SH, SW, PH, PW, H, W, in_mode;
    if (sscanf(line, "%127s %d %d %d %d %d %d %d %d %d %d %d %d %d %d", id, &nd, &B, &cin, &cout, &groups, &KH, &KW, &SH, &SW, &PH, &PW, &H,
               &W, &in_mode) != 15 || nd < 1 || nd > 2 || B < 1 || cin < 1 || cout < 1 || groups < 1 || KH < 1 || KW < 1 || SH < 1 || SW < 1 ||
        PH < 0 || PW < 0 || H < 1 || W < 1 || in_mode < 0 || in_mode > 2 || (nd == 1 && (H != 1 || KH != 1))) {
      fprintf(stderr, "bad line: %s", line);
      return 2;
    }
    ms_conv_desc d;
    memset(&d, 0, sizeof d);
    d.B = B; d.Cin = cin; d.Cout = cout; d.groups = groups; d.H = H; d.W = W;
    d.KH = KH; d.KW = KW; d.SH = SH; d.SW = SW; d.PH = PH; d.PW = PW;
    d.OH = (H + 2 * PH - KH) / SH + 1; d.OW = (W + 2 * PW - KW) / SW + 1;
    d.in_mode = in_mode;
    if (H + 2 * PH < KH || W + 2 * PW < KW) {
      fprintf(stderr, "%s: the kernel does not fit the padded input\n", id);
      return 2;
    }
    const bool up2 = ms::plan_up2_of(&d);
    const int one_d = ms::plan_nd_of(&d) == 1;
    print_conv(id, "fwd", ms::fwd_plan16_of(&d), d.KH, d.KW, up2, one_d ? d.B : d.OH, d.OW, d.Cout, d.Cin);
    const ms::DgradGeo dg = ms::dgrad_geo_of(&d);
    const int qh = ms::cdiv(d.H, d.SH), qw = ms::cdiv(d.W, d.SW);
    print_conv(id, "dgrad", ms::dgrad_plan16_of(&d, dg), dg.jh, dg.jw, false, one_d ? d.B : qh, qw, d.Cin, dg.tcog);
    const ms::Wgrad16Plan wp = ms::wgrad_plan16_of(&d);
    if (!wp.tp) {
      printf("%s wgrad ok=0\n", id);
    } else {
      printf("%s wgrad ok=1 tp=%d up2=%d npxt=%d nstg=%d splits=%d one=%d c1=%d tiles=%d tw=%d\n", id, up2 ? 3 : wp.tp, up2 ? 1 : 0,
             up2 ? 0 : ms::wg16_npxt(wp.npx), wp.nstg, wp.splits, wp.splits == 1 ? 1 : 0,
             ms::wgrad16_c1_shape(d.Cin, d.groups, d.KH, d.KW, up2) ? 1 : 0, wp.n_tiles, wp.tw);
    }
  }
  return 0;
}
