// host_rq_batch_build.hpp -- batched addPoint for rabitqlib's builder: the order of host_batch_build.hpp -- the
// same schedule, phase A against the graph as the batch found it, phase B's writes in ascending id -- over RqGraph's own members
// (rq_search_layer, rq_heuristic, rq_connect: pair-ordered heaps, Eigen's packet inner product, no second link to a node that
// lists the new one).  The device build (build_gpu.hip, the rq kernels) follows the same definition and is held to this twin byte
// for byte.  batch_max == 1 is the serial construct(): the bytes of RqGraph::rq_build with one thread.
#pragma once
#include "host_batch_build.hpp"
#include "host_rq_graph.hpp"

namespace hs {

// The batches of `steps` on g, whose rows are all in place (ddist reads the new row by its id).  lv: the level of every row.
inline void rq_batch_steps_host(RqGraph &g, const std::vector<BatchStep> &steps, const float *base, const int *lv, int threads) {
  const size_t d = g.dim;
  if (threads < 1) threads = 1;
  std::vector<VanillaGraph::Visited> vl(threads);
  std::vector<std::vector<RqGraph::MaxH>> found;   // per row of the batch, per level: the heap rq_heuristic(top, M) leaves, not yet popped
  for (const BatchStep &s : steps) {
    found.assign(s.size, {});
    if ((int32_t)s.ep != -1) {
      parallel_for(s.size, threads, 1, [&](size_t k, int tid) {   // phase A: read only
        const uint32_t p = s.begin + (uint32_t)k;
        uint32_t cur = s.ep;
        if (lv[p] < s.top) {
          float curdist = g.ddist(cur, p);
          g.descend(cur, curdist, s.top, lv[p], true, [&](uint32_t c) { return g.ddist(c, p); });
        }
        const int l0 = std::min(lv[p], (int)s.top);
        found[k].resize(l0 + 1);
        for (int level = l0; level >= 0; level--) {
          RqGraph::MaxH top = g.rq_search_layer(cur, p, level, vl[tid]);
          g.rq_heuristic(top, g.M);
          found[k][level] = top;
          while (top.size() > 1) top.pop();   // sel.back() of rq_connect(): the last one popped
          cur = top.top().second;
        }
      });
    }
    for (uint32_t k = 0; k < s.size; k++) {   // phase B: the writes, ascending id
      const uint32_t p = s.begin + k;
      g.count = p + 1;
      const VanillaGraph::Insert in = g.begin_insert(base + (size_t)p * d, p, p, lv[p]);
      // (rq_heuristic inside rq_connect() sees at most M entries, every one of which it kept before: it keeps them again)
      for (int level = (int)found[k].size() - 1; level >= 0; level--) g.rq_connect(p, found[k][level], level);
      g.adopt_entry(p, lv[p], in);
    }
  }
}

// What RqGraph::rq_build sets up before its first insertion: the parameters, mult = 1 / ln M, every row in place.
inline void rq_init(RqGraph &g, const float *base, size_t n, size_t d, Metric m, size_t M_, size_t efC_) {
  g.init(n, d, m, M_, efC_, "e");
  g.mult = 1 / log(1.0 * (double)g.M);
  for (size_t i = 0; i < n; i++) memcpy(g.el((uint32_t)i) + g.offsetData, base + i * d, 4 * d);
}

// The batched build on the host.  g: default-constructed; afterwards as RqGraph::rq_build leaves it.  Labels are the row index.
inline void rq_batch_build_host(RqGraph &g, const float *base, size_t n, size_t d, Metric m, size_t M_, size_t efC_, size_t seed, int threads,
                                size_t grow_div, size_t batch_max, BatchBuildStats *stats) {
  rq_init(g, base, n, d, m, M_, efC_);
  const std::vector<int> lv = draw_levels(n, g.mult, seed);
  const std::vector<BatchStep> steps = batch_schedule(lv.data(), n, grow_div, batch_max);
  rq_batch_steps_host(g, steps, base, lv.data(), threads);
  g.count = n;
  if (stats) stats->batches = steps.size();
}

}  // namespace hs
