// host_update.hpp -- what changes a VanillaGraph after it was built or loaded: resume (the addPoint loop continued, hnswalg.h:1248-1376)
// and the update path: markDelete / unmarkDelete, updatePoint / repairConnectionsForUpdate, addPoint(.., replace_deleted),
// resizeIndex (hnswalg.h:689-717, 943-1001, 1025-1272).  Free functions over the graph; their state (level_gen, allow_replace,
// deleted_elements) is the graph's.  Pinned by the saved file after every operation (tests/test_live_*_cpu.py) and run under
// AddressSanitizer / UBSan by resume_test.cpp and upsert_test.cpp.
#pragma once
#include <unordered_map>

#include "host_graph.hpp"

namespace hs {

// getRandomLevel (hnswalg.h:217-221): one draw of level_gen
inline int draw_level(VanillaGraph &g) { return level_from(g.level_gen, g.mult); }
// level_generator_.seed(seed) as the building constructor does (hnswalg.h:113), then `drawn` levels discarded: the state of a
// build that has added `drawn` points
inline void seed_levels(VanillaGraph &g, size_t seed, size_t drawn) {
  g.level_gen.seed(seed);
  for (size_t i = 0; i < drawn; i++) (void)draw_level(g);
}
// Continue the addPoint loop (hnswalg.h:1248-1376, new labels only) on a graph with spare capacity -- built here or loaded with
// max_elements > count; mult, M and ef_construction are the file header's.  Row i becomes internal id count + i; its level is
// drawn from level_gen in row order, so threads == 1 is the reference's serial order bit for bit.  threads > 1 as build():
// a first point of an empty graph serially, the rest in parallel.  The caller has checked capacity and labels.
inline void resume(VanillaGraph &g, const float *rows, const uint64_t *labels, size_t n_add, int threads) {
  if (g.count + n_add > g.max_elements) throw std::runtime_error("The number of elements exceeds the specified limit");
  const size_t first = g.count, d = g.dim;
  std::vector<int> lv(n_add);
  for (size_t i = 0; i < n_add; i++) lv[i] = draw_level(g);
  if (threads < 1) threads = 1;
  std::vector<VanillaGraph::Visited> vl(threads);
  const size_t serial_head = threads > 1 ? (first == 0 ? std::min<size_t>(n_add, 1) : 0) : n_add;
  for (size_t i = 0; i < serial_head; i++) { g.count = first + i + 1; g.add_point(rows + i * d, labels[i], (uint32_t)(first + i), lv[i], vl[0]); }
  g.count = first + n_add;
  parallel_for(n_add - serial_head, threads, 1, [&](size_t k, int tid) {
    const size_t i = serial_head + k;
    g.add_point(rows + i * d, labels[i], (uint32_t)(first + i), lv[i], vl[tid]);
  });
}

// allow_replace_deleted_ as the constructor sets it; turning it on fills deleted_elements from the marks in increasing id, as
// loadIndex does (:882-888), into a freshly constructed set
inline void set_allow_replace(VanillaGraph &g, bool on) {
  g.allow_replace = on;
  g.deleted_elements = std::unordered_set<uint32_t>();
  if (on)
    for (size_t i = 0; i < g.count; i++)
      if (g.deleted((uint32_t)i)) g.deleted_elements.insert((uint32_t)i);
}
inline void mark(VanillaGraph &g, uint32_t i) {     // markDeletedInternal (:943-958)
  if (g.deleted(i)) throw std::runtime_error("The requested to delete element is already deleted");
  g.set_deleted(i, true);
  if (g.allow_replace) g.deleted_elements.insert(i);
}
inline void unmark(VanillaGraph &g, uint32_t i) {   // unmarkDeletedInternal (:986-1001)
  if (!g.deleted(i)) throw std::runtime_error("The requested to undelete element is not deleted");
  g.set_deleted(i, false);
  if (g.allow_replace) g.deleted_elements.erase(i);
}
inline std::vector<uint32_t> connections(const VanillaGraph &g, uint32_t i, int level) {   // getConnectionsWithLock (:1238-1246)
  const uint32_t *l = g.list_at(i, level);
  return std::vector<uint32_t>(l + 1, l + 1 + VanillaGraph::cnt_of(l));
}

// repairConnectionsForUpdate (:1159-1236)
inline void repair_connections(VanillaGraph &g, const float *x, uint32_t ep, uint32_t id, int dataPointLevel, int maxLevel,
                               VanillaGraph::Visited &vl) {
  uint32_t currObj = ep;
  if (dataPointLevel < maxLevel) {
    float curdist = g.dist(x, g.vec(currObj));
    g.descend(currObj, curdist, maxLevel, dataPointLevel, false, [&](uint32_t c) { return g.dist(x, g.vec(c)); });
  }
  if (dataPointLevel > maxLevel) throw std::runtime_error("Level of item to be updated cannot be bigger than max level");
  for (int level = dataPointLevel; level >= 0; level--) {
    MaxQ top = g.search_layer(currObj, x, level, vl);
    MaxQ filtered;   // the self-filter (:1210-1215)
    while (!top.empty()) {
      if (top.top().second != id) filtered.push(top.top());
      top.pop();
    }
    if (filtered.empty()) continue;
    if (g.deleted(ep)) {   // epDeleted (:1222-1230)
      filtered.emplace(g.dist(x, g.vec(ep)), ep);
      if (filtered.size() > g.efC) filtered.pop();
    }
    currObj = g.connect(id, filtered, level, true);
  }
}

// updatePoint(dataPoint, internalId, updateNeighborProbability = 1.0) (:1067-1157).  The reference draws
// update_probability_generator_ once per one-hop neighbour and skips the neighbour when the draw exceeds the probability; a
// draw from [0, 1) never exceeds 1.0 and nothing else reads that generator, so no state is kept for it here.
// sCand / sNeigh are std::unordered_set as in the reference: the iteration order of sCand is the insertion order of the
// candidate heap, which decides how equal distances are ordered.
inline void update_point(VanillaGraph &g, const float *x, uint32_t id, VanillaGraph::Visited &vl) {
  memcpy(g.el(id) + g.offsetData, x, 4 * g.dim);
  g.note_touched0(id);
  const int maxLevelCopy = g.maxlevel;
  const uint32_t entryPointCopy = g.enterpoint;
  if (entryPointCopy == id && g.count == 1) return;   // :1076-1077
  const int elemLevel = g.levels[id];
  for (int layer = 0; layer <= elemLevel; layer++) {
    std::unordered_set<uint32_t> sCand, sNeigh;
    const std::vector<uint32_t> listOneHop = connections(g, id, layer);
    if (listOneHop.empty()) continue;
    sCand.insert(id);
    for (uint32_t elOneHop : listOneHop) {
      sCand.insert(elOneHop);
      sNeigh.insert(elOneHop);
      for (uint32_t elTwoHop : connections(g, elOneHop, layer)) sCand.insert(elTwoHop);
    }
    for (uint32_t neigh : sNeigh) {
      MaxQ candidates;
      const size_t size = sCand.find(neigh) == sCand.end() ? sCand.size() : sCand.size() - 1;
      const size_t elementsToKeep = std::min(g.efC, size);
      for (uint32_t cand : sCand) {
        if (cand == neigh) continue;
        const float distance = g.dist(g.vec(neigh), g.vec(cand));
        if (candidates.size() < elementsToKeep) {
          candidates.emplace(distance, cand);
        } else if (distance < candidates.top().first) {
          candidates.pop();
          candidates.emplace(distance, cand);
        }
      }
      g.heuristic(candidates, layer == 0 ? g.maxM0 : g.maxM);
      uint32_t *l = g.list_at(neigh, layer);
      const size_t candSize = candidates.size();
      VanillaGraph::set_cnt(l, (uint16_t)candSize);   // the count alone: ids behind it stay (and are saved)
      for (size_t idx = 0; idx < candSize; idx++) { l[1 + idx] = candidates.top().second; candidates.pop(); }
      if (layer == 0) g.note_touched0(neigh);
    }
  }
  repair_connections(g, x, entryPointCopy, id, elemLevel, maxLevelCopy, vl);
}

// addPoint(data_point, label, replace_deleted) (:1025-1065) with the existing-label branch of addPoint(.., level) (:1251-1272),
// serial.  `lookup` is label_lookup_, kept by the caller.  Returns the internal id written; *replaced_label (when given) receives
// the label that left the index and *reused says whether a deleted slot was taken.
inline uint32_t upsert(VanillaGraph &g, const float *x, uint64_t lab, bool replace_deleted, std::unordered_map<uint64_t, uint32_t> &lookup,
                       VanillaGraph::Visited &vl, bool *reused = nullptr, uint64_t *replaced_label = nullptr) {
  if (reused) *reused = false;
  if (!g.allow_replace && replace_deleted) throw std::runtime_error("Replacement of deleted elements is disabled in constructor");
  if (replace_deleted && !g.deleted_elements.empty()) {
    const uint32_t id = *g.deleted_elements.begin();
    g.deleted_elements.erase(id);
    const uint64_t old = g.label(id);
    memcpy(g.el(id) + g.label_offset, &lab, 8);
    lookup.erase(old);
    lookup[lab] = id;
    unmark(g, id);
    update_point(g, x, id, vl);
    if (reused) *reused = true;
    if (replaced_label) *replaced_label = old;
    return id;
  }
  auto it = lookup.find(lab);
  if (it != lookup.end()) {
    const uint32_t id = it->second;
    if (g.allow_replace && g.deleted(id))
      throw std::runtime_error("Can't use addPoint to update deleted elements if replacement of deleted elements is enabled.");
    if (g.deleted(id)) unmark(g, id);
    update_point(g, x, id, vl);
    return id;
  }
  if (g.count >= g.max_elements) throw std::runtime_error("The number of elements exceeds the specified limit");
  const uint32_t cur_c = (uint32_t)g.count;
  g.count++;
  lookup[lab] = cur_c;
  g.add_point(x, lab, cur_c, draw_level(g), vl);
  return cur_c;
}

// resizeIndex (:689-717).  The reference reallocs, which leaves the rows beyond the old capacity undefined until addPoint
// clears each one; here they are zero.
inline void resize(VanillaGraph &g, size_t new_max) {
  if (new_max < g.count) throw std::runtime_error("Cannot resize, max element is less than the current number of elements");
  g.levels.resize(new_max);
  g.locks.reset(new std::mutex[std::max<size_t>(new_max, 1)]);
  g.level0.resize(new_max * g.size_per_el);
  g.links.resize(new_max);
  g.max_elements = new_max;
}

}  // namespace hs
