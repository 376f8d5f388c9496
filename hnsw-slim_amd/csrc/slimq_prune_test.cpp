// slimq_prune_test.cpp -- host-only test of csrc/slimq_prune.hpp, the closed form of HierarchicalNSWSlimQ's PruneByHeuristic that
// convert_slimq.hip evaluates a chunk of candidates at a time, against prune_slimq (host_rq_graph.hpp), the loop as the reference
// writes it.  The chunk loop below is the kernel's (cq_prune) with a wavefront's ballot replaced by a loop over the chunk.
// Lists: random subsets of continuous rows, and small-integer rows whose lists are full of equal keys and equal pair distances;
// budgets 0, 1, 3, 8, 16, 32, 64 and one above the list; both metrics; lists up to 200 ids (a union).
// Build: g++ -std=c++17 -O2 -ffp-contract=off -pthread slimq_prune_test.cpp -o slimq_prune_test   (also with -fsanitize=address,undefined)
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "host_rq_graph.hpp"
#include "slimq_prune.hpp"

using namespace hs;

static std::vector<uint32_t> by_closed_form(const VanillaGraph &g, const std::vector<pairfi> &sorted, size_t mlim) {
  std::vector<uint32_t> kept(mlim);
  const uint32_t sz = (uint32_t)sorted.size();
  uint32_t kc = 0;
  for (uint32_t base = 0; base < sz && kc < mlim; base += kSlimqPruneChunk) {
    const uint32_t cnt = std::min(kSlimqPruneChunk, sz - base);
    unsigned long long good = 0;
    for (uint32_t j = 0; j < cnt; j++) {
      const float pd = rabitq_raw_dist(g.metric, g.vec(base + j), g.vec(sorted[base + j].second), g.dim);
      if (slimq_keeps(base + j, pd, sorted[base + j].first)) good |= 1ull << j;
    }
    for (uint32_t j = 0; j < cnt; j++)
      if ((good >> j & 1) && slimq_slot(good, j, kc) < mlim) kept[slimq_slot(good, j, kc)] = sorted[base + j].second;
    kc = slimq_kept_after(good, kc, (uint32_t)mlim);
  }
  kept.resize(kc);
  return kept;
}

int main() {
  int bad = 0;
  size_t cases = 0, pruned = 0, full = 0;
  std::mt19937 rng(11);
  for (int integer = 0; integer < 2; integer++)
    for (Metric metric : {METRIC_L2, METRIC_IP}) {
      const size_t n = 260, d = integer ? 5 : 24;
      VanillaGraph g;
      g.init(n, d, metric, 8, 40, "e");
      g.count = n;
      std::normal_distribution<float> nd(0.f, 1.f);
      for (size_t i = 0; i < n; i++) {
        float *row = (float *)(g.el((uint32_t)i) + g.offsetData);
        for (size_t k = 0; k < d; k++) row[k] = integer ? (float)((int)(rng() % 5) - 2) : nd(rng);
      }
      for (int rep = 0; rep < 300; rep++) {
        const size_t sz = rep < 8 ? (size_t)rep : 1 + rng() % 200;   // 0 .. 7 ids, then up to 200
        std::vector<uint32_t> all(n);
        for (uint32_t i = 0; i < n; i++) all[i] = i;
        std::shuffle(all.begin(), all.end(), rng);
        const uint32_t v = all.back();
        std::vector<pairfi> sorted(sz);
        for (size_t j = 0; j < sz; j++) sorted[j] = {rabitq_raw_dist(metric, g.vec(v), g.vec(all[j]), d), all[j]};
        std::sort(sorted.begin(), sorted.end(), CmpFirst());
        for (size_t mlim : {(size_t)0, (size_t)1, (size_t)3, (size_t)8, (size_t)16, (size_t)32, (size_t)64, sz + 1}) {
          std::vector<uint32_t> want;
          prune_slimq(g, sorted, want, mlim);
          const std::vector<uint32_t> got = by_closed_form(g, sorted, mlim);
          cases++;
          pruned += want.size() < std::min(sz, mlim);
          full += mlim > 0 && want.size() == mlim && sz > mlim;
          if (want != got) {
            printf("MISMATCH: integer %d metric %d, %zu ids, Mlim %zu: %zu kept, want %zu\n", integer, (int)metric, sz, mlim, got.size(), want.size());
            bad++;
          }
        }
      }
    }
  if (pruned == 0 || full == 0) { printf("slimq_prune: premise failed (%zu lists lost a candidate to the test, %zu stopped at Mlim)\n", pruned, full); return 1; }
  if (bad) { printf("slimq_prune FAILED: %d of %zu cases\n", bad, cases); return 1; }
  printf("slimq_prune ok: %zu cases, %zu with a candidate dropped by the test, %zu stopped at Mlim\n", cases, pruned, full);
  return 0;
}
