// host_batch_build.hpp -- batched addPoint: the insertion order that is parallel and still deterministic, as a
// schedule (a pure function of the levels) and as a build over VanillaGraph's own members.  The device build (build_gpu.hip)
// follows the same definition and is held to this twin byte for byte.
//   * points enter in id order, in batches; every point of a batch runs the search half of addPoint (hnswalg.h:1300-1360 without
//     the writes) against the graph as it stood when the batch began (phase A, any order, the worker pool);
//   * the writes -- mutuallyConnectNewElement, VanillaGraph::connect -- are then applied in ascending id (phase B, serial);
//   * a batch ends right after the first row whose level exceeds the current top level, so that the entry point and the top level
//     before every batch follow from the levels alone.
// batch_max == 1 is the reference's serial addPoint loop.
#pragma once
#include <chrono>

#include "host_graph.hpp"

namespace hs {

static constexpr size_t kBatchGrowDiv = 16;      // defaults of hs_batch_build_opts (0 = these)
static constexpr size_t kBatchMax = 16384;

struct BatchStep {
  uint32_t begin, size;   // rows [begin, begin + size)
  uint32_t ep;            // entry point before the batch (0xFFFFFFFF: the empty graph)
  int32_t top;            // top level before the batch (-1: the empty graph)
};

// The schedule of (levels[], grow_div, batch_max): the next batch holds min(batch_max, max(1, inserted / grow_div), n - inserted)
// rows and is cut right after the first row whose level exceeds the current top level.
inline std::vector<BatchStep> batch_schedule(const int *levels, size_t n, size_t grow_div, size_t batch_max) {
  if (grow_div == 0) grow_div = kBatchGrowDiv;
  if (batch_max == 0) batch_max = kBatchMax;
  std::vector<BatchStep> out;
  uint32_t ep = (uint32_t)-1;
  int32_t top = -1;
  for (size_t done = 0; done < n;) {
    size_t sz = std::min(batch_max, std::min(std::max<size_t>(1, done / grow_div), n - done));
    uint32_t nep = ep;
    int32_t ntop = top;
    for (size_t k = 0; k < sz; k++)
      if (levels[done + k] > top) {
        sz = k + 1;
        nep = (uint32_t)(done + k);
        ntop = levels[done + k];
        break;
      }
    out.push_back(BatchStep{(uint32_t)done, (uint32_t)sz, ep, top});
    done += sz;
    ep = nep;
    top = ntop;
  }
  return out;
}

inline std::vector<int> draw_levels(size_t n, double mult, size_t seed) {   // as VanillaGraph::build draws them
  std::default_random_engine gen;
  gen.seed(seed);
  std::vector<int> lv(n);
  for (size_t i = 0; i < n; i++) lv[i] = level_from(gen, mult);
  return lv;
}

struct BatchBuildStats {
  size_t batches = 0, flagged_rows = 0;
  double kernel_ms = 0.0;
};

// The batched build on the host.  g: default-constructed; afterwards as VanillaGraph::build leaves it.
inline void batch_build_host(VanillaGraph &g, const float *base, size_t n, size_t d, Metric m, size_t M_, size_t efC_, const std::string &bf,
                             size_t seed, int threads, const uint64_t *labels, size_t grow_div, size_t batch_max, BatchBuildStats *stats) {
  g.init(n, d, m, M_, efC_, bf);
  const std::vector<int> lv = draw_levels(n, g.mult, seed);
  const std::vector<BatchStep> steps = batch_schedule(lv.data(), n, grow_div, batch_max);
  if (threads < 1) threads = 1;
  std::vector<VanillaGraph::Visited> vl(threads);
  std::vector<std::vector<MaxQ>> found;   // per row of the batch, per level: the heap heuristic(top, M) leaves, not yet popped
  for (const BatchStep &s : steps) {
    found.assign(s.size, {});
    if ((int32_t)s.ep != -1) {
      parallel_for(s.size, threads, 1, [&](size_t k, int tid) {   // phase A: read only
        const uint32_t p = s.begin + (uint32_t)k;
        const float *x = base + (size_t)p * d;
        uint32_t cur = s.ep;
        if (lv[p] < s.top) {
          float curdist = g.dist(x, g.vec(cur));
          g.descend(cur, curdist, s.top, lv[p], true, [&](uint32_t id) { return g.dist(x, g.vec(id)); });
        }
        const int l0 = std::min(lv[p], (int)s.top);
        found[k].resize(l0 + 1);
        for (int level = l0; level >= 0; level--) {
          MaxQ top = g.search_layer(cur, x, level, vl[tid]);
          g.heuristic(top, g.M);
          found[k][level] = top;
          while (top.size() > 1) top.pop();   // sel.back() of connect(): the last one popped
          cur = top.top().second;
        }
      });
    }
    for (uint32_t k = 0; k < s.size; k++) {   // phase B: the writes, ascending id
      const uint32_t p = s.begin + k;
      g.count = p + 1;
      const VanillaGraph::Insert in = g.begin_insert(base + (size_t)p * d, labels ? labels[p] : p, p, lv[p]);
      // (the heuristic inside connect() sees at most M entries, every one of which it kept before: it keeps them again, in the
      //  same order, so the heap it re-emplaces and the order connect() pops are those of phase A)
      for (int level = (int)found[k].size() - 1; level >= 0; level--) g.connect(p, found[k][level], level);
      g.adopt_entry(p, lv[p], in);
    }
  }
  g.count = n;
  if (stats) stats->batches = steps.size();
}

}  // namespace hs
