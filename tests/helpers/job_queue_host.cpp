// Host driver of csrc/job_queue.h for tests/test_job_queue_cpu.py: no GPU, no Python.  Reads cases from stdin
//   case <name>
//   <family> <k0> <k1> <k2> <k3> <k4> <k5> <length> <workgroups>     one queued job; its index is its position in the case
//   discard                                                          what ms_wgrad_discard does
//   end
// queues each job in its family's PendingQueue, flushes the three queues in ms_wgrad_flush's order with the family's ordering and
// predicate (restated from wgrad_patch_flush, wgrad_gather_flush, wgrad16_flush) and prints one line per launch:
//   <family> <k0> .. <k5> | <job indices> | <workgroups>
// family p: key = (KH, KW, S, tw, up2, wave);  g: key = (shape);  h: key = (dt, tp, up2, npxt).  The job limits come from the build
// line (-DWGP_MAX_JOBS=.. -DWG_MAX_JOBS=.. -DWG16_MAX_JOBS=..): the test passes the mirror's constants.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "job_queue.h"

struct Pending { int key[6], len, a, nwg; double flops, bytes; };
template <int MAX>
struct Batch { int n; int block_end[MAX]; int job[MAX]; };

static ms::PendingQueue<Pending> g_patch, g_gather, g_h16;

template <typename B, typename Same>
static int flush(char family, const std::vector<Pending>& q, Same same) {
  return ms::pack_jobs<B>(q, same, [family](const Pending& h, const B& b, const std::vector<const Pending*>& jobs, const ms::JobTotals& t) -> int {
    long wgs = 0;
    double bytes = 0;
    if ((size_t)b.n != jobs.size() || b.n < 1) return 1;
    for (int i = 0; i < b.n; ++i) {
      wgs += jobs[i]->nwg; bytes += jobs[i]->bytes;
      if (b.job[i] != jobs[i]->a || b.block_end[i] != wgs) return 1;
    }
    if (wgs != t.wgs || t.flops != (double)b.n || t.bytes != bytes) return 1;
    printf("%c %d %d %d %d %d %d |", family, h.key[0], h.key[1], h.key[2], h.key[3], h.key[4], h.key[5]);
    for (int i = 0; i < b.n; ++i) printf(" %d", b.job[i]);
    printf(" | %ld\n", t.wgs);
    return 0;
  });
}

static int flush_all() {
  std::vector<Pending> q = g_patch.take();
  ms::sort_jobs(q, [](const Pending& x) { return -x.len; });
  const int rc = flush<Batch<WGP_MAX_JOBS>>('p', q, [](const Pending& x, const Pending& h) {
    return x.key[0] == h.key[0] && x.key[1] == h.key[1] && x.key[2] == h.key[2] && x.key[3] == h.key[3] && x.key[4] == h.key[4] &&
           (x.key[5] != 0) == (h.key[5] != 0);
  });
  q = g_gather.take();
  ms::sort_jobs(q, [](const Pending& x) { return x.key[0]; });
  const int rcg = flush<Batch<WG_MAX_JOBS>>('g', q, [](const Pending& x, const Pending& h) { return x.key[0] == h.key[0]; });
  const int rc16 = flush<Batch<WG16_MAX_JOBS>>('h', g_h16.take(), [](const Pending& x, const Pending& h) {
    return x.key[0] == h.key[0] && x.key[1] == h.key[1] && x.key[2] == h.key[2] && x.key[3] == h.key[3];
  });
  return rc ? rc : rcg ? rcg : rc16;
}

int main() {
  char line[256], name[128];
  int next = 0;
  while (fgets(line, sizeof line, stdin)) {
    Pending p = {};
    char family;
    if (sscanf(line, "case %127s", name) == 1) {
      printf("case %s\n", name);
      next = 0;
    } else if (!strncmp(line, "discard", 7)) {
      g_patch.discard(); g_gather.discard(); g_h16.discard();
    } else if (!strncmp(line, "end", 3)) {
      if (flush_all()) { fprintf(stderr, "%s: a launch does not hold what pack_jobs says it holds\n", name); return 1; }
      printf("end\n");
    } else if (sscanf(line, " %c %d %d %d %d %d %d %d %d", &family, &p.key[0], &p.key[1], &p.key[2], &p.key[3], &p.key[4], &p.key[5], &p.len, &p.nwg) == 9) {
      p.a = next++; p.flops = 1; p.bytes = p.nwg;
      (family == 'p' ? g_patch : family == 'g' ? g_gather : g_h16).push(p);
    } else {
      fprintf(stderr, "bad line: %s", line);
      return 2;
    }
  }
  return 0;
}
