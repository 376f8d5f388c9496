// host_batch_build.hpp -- batched addPoint: the insertion order that is parallel and still deterministic, as a
// schedule (a pure function of the levels) and as a build over VanillaGraph's own members.  The device build (build_gpu.hip)
// follows the same definition and is held to this twin byte for byte.
//   * points enter in id order, in batches; every point of a batch runs the search half of addPoint (hnswalg.h:1300-1360 without
//     the writes) against the graph as it stood when the batch began (phase A, any order, the worker pool);
//   * the writes -- mutuallyConnectNewElement, VanillaGraph::connect -- are then applied in ascending id (phase B, serial);
//   * a batch ends right after the first row whose level exceeds the current top level, so that the entry point and the top level
//     before every batch follow from the levels alone.
// batch_max == 1 is the reference's serial addPoint loop.
// The same order continued from a loaded graph with room: batch_schedule_from, batch_add_host -- the twin of
// hs_index_add_points_batched; a build split at a batch boundary of its schedule writes the whole build's bytes.
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

// The same rule continued from a graph that holds n0 rows with entry point `ep` and top level `top`: levels[i] is
// the level of row n0 + i, `begin` of a step is the internal id.  n0 == 0 with ep == 0xFFFFFFFF, top == -1 is batch_schedule.
inline std::vector<BatchStep> batch_schedule_from(const int *levels, size_t count, size_t n0, uint32_t ep, int32_t top, size_t grow_div,
                                                  size_t batch_max) {
  if (grow_div == 0) grow_div = kBatchGrowDiv;
  if (batch_max == 0) batch_max = kBatchMax;
  std::vector<BatchStep> out;
  const size_t n = n0 + count;
  for (size_t done = n0; done < n;) {
    size_t sz = std::min(batch_max, std::min(std::max<size_t>(1, done / grow_div), n - done));
    uint32_t nep = ep;
    int32_t ntop = top;
    for (size_t k = 0; k < sz; k++)
      if (levels[done - n0 + k] > top) {
        sz = k + 1;
        nep = (uint32_t)(done + k);
        ntop = levels[done - n0 + k];
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

// The batches of `steps` on g: rows, labels (nullable: the id) and lv are indexed by id - first.  Phase A reads the graph as the batch
// found it, phase B writes in ascending id.
inline void batch_steps_host(VanillaGraph &g, const std::vector<BatchStep> &steps, size_t first, const float *rows, const uint64_t *labels,
                             const int *lv, int threads) {
  const size_t d = g.dim;
  if (threads < 1) threads = 1;
  std::vector<VanillaGraph::Visited> vl(threads);
  std::vector<std::vector<MaxQ>> found;   // per row of the batch, per level: the heap heuristic(top, M) leaves, not yet popped
  for (const BatchStep &s : steps) {
    found.assign(s.size, {});
    if ((int32_t)s.ep != -1) {
      parallel_for(s.size, threads, 1, [&](size_t k, int tid) {   // phase A: read only
        const size_t r = s.begin + k - first;
        const float *x = rows + r * d;
        uint32_t cur = s.ep;
        if (lv[r] < s.top) {
          float curdist = g.dist(x, g.vec(cur));
          g.descend(cur, curdist, s.top, lv[r], true, [&](uint32_t id) { return g.dist(x, g.vec(id)); });
        }
        const int l0 = std::min(lv[r], (int)s.top);
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
      const size_t r = p - first;
      g.count = p + 1;
      const VanillaGraph::Insert in = g.begin_insert(rows + r * d, labels ? labels[r] : p, p, lv[r]);
      // (the heuristic inside connect() sees at most M entries, every one of which it kept before: it keeps them again, in the
      //  same order, so the heap it re-emplaces and the order connect() pops are those of phase A)
      for (int level = (int)found[k].size() - 1; level >= 0; level--) g.connect(p, found[k][level], level);
      g.adopt_entry(p, lv[r], in);
    }
  }
}

// The batched build on the host.  g: default-constructed; afterwards as VanillaGraph::build leaves it.
inline void batch_build_host(VanillaGraph &g, const float *base, size_t n, size_t d, Metric m, size_t M_, size_t efC_, const std::string &bf,
                             size_t seed, int threads, const uint64_t *labels, size_t grow_div, size_t batch_max, BatchBuildStats *stats) {
  g.init(n, d, m, M_, efC_, bf);
  const std::vector<int> lv = draw_levels(n, g.mult, seed);
  const std::vector<BatchStep> steps = batch_schedule(lv.data(), n, grow_div, batch_max);
  batch_steps_host(g, steps, 0, base, labels, lv.data(), threads);
  g.count = n;
  if (stats) stats->batches = steps.size();
}

// Batched addPoint continued on a graph with room (built here or loaded with max_elements > count): row i becomes
// internal id count + i, its level is drawn from level_gen in row order (as resume() draws them), the schedule continues from the
// graph's element count, entry point and top level.  M, ef_construction and mult are the graph's.  The caller has checked capacity,
// labels and that no element is marked deleted; g.touched0, when set, receives the changed level-0 lists through connect().
inline void batch_add_host(VanillaGraph &g, const float *rows, const uint64_t *labels, size_t count, int threads, size_t grow_div, size_t batch_max,
                           BatchBuildStats *stats) {
  if (g.count + count > g.max_elements) throw std::runtime_error("The number of elements exceeds the specified limit");
  const size_t first = g.count;
  std::vector<int> lv(count);
  for (size_t i = 0; i < count; i++) lv[i] = level_from(g.level_gen, g.mult);
  const std::vector<BatchStep> steps = batch_schedule_from(lv.data(), count, first, g.enterpoint, g.maxlevel, grow_div, batch_max);
  batch_steps_host(g, steps, first, rows, labels, lv.data(), threads);
  g.count = first + count;
  if (stats) stats->batches = steps.size();
}

// The lists of g's first n0 nodes in the device build's form, for n >= n0 nodes with levels lev[]: upb (n + 1 prefix sums of the
// levels), the level-0 slots (maxM0 + 1 words each) and the upper slots (maxM + 1 words, node i's level l at upb[i] + l - 1), each
// slot copied whole -- the stale words behind the count are part of what saveIndex writes.  Slots of the nodes from n0 on are zero.
inline void build_form_lists(const VanillaGraph &g, size_t n0, size_t n, const uint32_t *lev, int threads, std::vector<uint32_t> &upb,
                             std::vector<uint32_t> &l0, std::vector<uint32_t> &lu) {
  const size_t s0 = g.maxM0 + 1, su = g.maxM + 1;
  upb.assign(n + 1, 0);
  for (size_t i = 0; i < n; i++) upb[i + 1] = upb[i] + lev[i];
  l0.assign(n * s0, 0);
  lu.assign((size_t)upb[n] * su, 0);
  parallel_for(n0, threads, 4096, [&](size_t i, int) {
    memcpy(l0.data() + i * s0, g.el((uint32_t)i), g.size_links0);
    if (lev[i]) memcpy(lu.data() + (size_t)upb[i] * su, g.links[i].data(), g.size_links_up * lev[i]);
  });
}

}  // namespace hs
