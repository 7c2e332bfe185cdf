// Many small jobs in ONE launch: the one place the packing rule lives.
//   device: a workgroup finds its job in the launch's table of block ranges (find_job);
//   host:   a process-wide queue of pending jobs (PendingQueue) and the rule that turns its contents into launches (pack_jobs).
// The host part is plain C++17 and needs no HIP header (tests/helpers/job_queue_host.cpp compiles it with the host compiler).
#pragma once
#include <algorithm>
#include <mutex>
#include <vector>

namespace ms {

#if defined(__HIPCC__)
// Job j owns the workgroups [end_of(j - 1), end_of(j)) of the launch; `end_of` reads the exclusive prefix sums wherever the batch
// keeps them (block_end[] beside the jobs, or block_end inside each job).
struct JobSlot { int j, first, count; };     // job index, the job's first workgroup, its workgroup count
template <typename EndOf>
__device__ __forceinline__ JobSlot find_job(int n, int wg, EndOf end_of) {
  int j = 0;
  while (j + 1 < n && wg >= end_of(j)) ++j;
  const int first = j ? end_of(j - 1) : 0;
  return {j, first, end_of(j) - first};
}
#endif

// Process-wide: autograd's device thread queues, the caller's thread flushes.
template <typename Pending>
class PendingQueue {
 public:
  void push(const Pending& p) { std::lock_guard<std::mutex> lk(mu_); q_.push_back(p); }
  void discard() { std::lock_guard<std::mutex> lk(mu_); q_.clear(); }
  std::vector<Pending> take() {
    std::vector<Pending> q;
    std::lock_guard<std::mutex> lk(mu_);
    q.swap(q_);
    return q;
  }

 private:
  std::vector<Pending> q_;
  std::mutex mu_;
};

// Ascending by `rank`; equal ranks keep their queue order.
template <typename Pending, typename Rank>
void sort_jobs(std::vector<Pending>& q, Rank rank) {
  std::stable_sort(q.begin(), q.end(), [&](const Pending& x, const Pending& y) { return rank(x) < rank(y); });
}

constexpr long MAX_LAUNCH_WGS = 0x3fffffff;
struct JobTotals { long wgs = 0; double flops = 0, bytes = 0; };

// The launches of one flush.  The first unlaunched job is the head; every later unlaunched job that `same(job, head)` holds for joins
// it, in order, in a Batch { n, block_end[MAX], job[MAX] }.  A batch is launched when it holds MAX jobs, when the next job would take
// its workgroups past MAX_LAUNCH_WGS, and at the end of the group: launch(head, batch, entries, totals) -> 0 or an error, which ends
// the flush (the jobs not yet launched are dropped).  A Pending has the fields a (the job's kernel arguments), nwg, flops, bytes.
template <typename Batch, typename Pending, typename Same, typename Launch>
int pack_jobs(const std::vector<Pending>& q, Same same, Launch launch) {
  constexpr int MAX = (int)(sizeof(Batch::block_end) / sizeof(int));
  std::vector<char> done(q.size(), 0);
  std::vector<const Pending*> entries;
  for (size_t i = 0; i < q.size(); ++i) {
    if (done[i]) continue;
    Batch b;
    b.n = 0;
    JobTotals t;
    auto flush = [&]() -> int {
      if (!b.n) return 0;
      const int rc = launch(q[i], b, entries, t);
      b.n = 0; t = JobTotals(); entries.clear();
      return rc;
    };
    for (size_t k = i; k < q.size(); ++k) {
      if (done[k] || !same(q[k], q[i])) continue;
      if (b.n == MAX || t.wgs + q[k].nwg > MAX_LAUNCH_WGS) {
        const int rc = flush();
        if (rc) return rc;
      }
      t.wgs += q[k].nwg; t.flops += q[k].flops; t.bytes += q[k].bytes;
      b.block_end[b.n] = (int)t.wgs;
      b.job[b.n] = q[k].a;
      ++b.n;
      entries.push_back(&q[k]);
      done[k] = 1;
    }
    const int rc = flush();
    if (rc) return rc;
  }
  return 0;
}

}  // namespace ms
