// slim_diff.hpp -- the patch server's host core: convertFromHNSWWithDiff (hnswalg_slim.h:1110-1424, 1478-1751) and genPatch
// (:1427-1476) as free functions over a SlimGraph.  Pinned byte for byte by tests/test_slim_diff_cpu.py.
#pragma once
#include <atomic>
#include <set>
#include <unordered_map>

#include "host_graph.hpp"

namespace hs {

// What one call leaves behind: the two changed lists in ascending id (the reference fills them from an OpenMP loop, in any
// order), the nodes whose image changed in any way (what a device copy has to rewrite), genPatch's two cursors.
struct SlimDiff {
  size_t count = 0;
  std::vector<uint32_t> old_ids, new_ids;
  std::vector<uint32_t> dirty;      // blob, row or label differs from before the call, or the node is beyond the previous count
  std::vector<uint32_t> stale;      // the part of `dirty` whose row or label differs (or is new): a device copy rewrites the row too
  size_t n_reprune = 0;             // lists that went through the re-prune (:1279-1303)
  size_t ind_old = 0, ind_new = 0;  // ind_old_ / ind_new_ (:78-79)
};
// label_lookup_ of a Slim index that is re-derived on the device: the map, and the nodes i whose label it maps to ANOTHER id
// (`lookup[label(i)] != i`, :1360: such a node is new whenever it has neighbours).  Every other node maps to itself, so a call
// looks up only the nodes whose label changed or that are new; the set is rebuilt (one pass) after a call that did not keep it.
struct SlimLookup {
  std::unordered_map<uint64_t, uint32_t> map;
  std::set<uint32_t> mismatch;
  bool mismatch_valid = false;
};

// The final per-level lists of every node, before the hierarchical filter: first prune with getNeighborsByHeuristic2
// (:1189-1232; only the kept set matters, the lists are sorted by id at :1269-1273), reverse edges (:1234-1241), union sorted
// by id and made unique, and the re-prune of a union above its level's capacity (:1279-1303), whose list is the pop order of
// the heap the heuristic returns -- every kept entry, where the reference pops `limit` times whatever was kept.
inline void diff_lists(const VanillaGraph &g, const SlimParams &p, size_t maxM0_, size_t maxM_, int threads,
                       std::vector<std::vector<std::vector<uint32_t>>> &nn, size_t &n_reprune) {
  const size_t n = g.count;
  const std::vector<size_t> thr = SlimGraph::hub_thresholds(g, p);
  nn.assign(n, {});
  std::vector<std::vector<std::vector<uint32_t>>> rev(n);
  parallel_for(n, threads, 64, [&](size_t v, int) {
    const int L = g.levels[v];
    nn[v].resize(L + 1); rev[v].resize(L + 1);
    for (int l = L; l >= 0; l--) {
      const uint32_t *ll = g.list_at(v, l);
      const size_t size = VanillaGraph::cnt_of(ll);
      const size_t M0 = l == 0 ? (size > thr[l] ? p.top_M0 : p.low_m0) : (size > thr[l] ? p.top_M : p.low_m);
      MaxQ heap;
      for (size_t j = 0; j < size; j++) heap.emplace(g.dist(g.vec(v), g.vec(ll[1 + j])), ll[1 + j]);
      g.heuristic(heap, M0);
      while (!heap.empty()) { nn[v][l].push_back(heap.top().second); heap.pop(); }
    }
  });
  for (size_t v = 0; v < n; v++)
    for (int l = 0; l <= g.levels[v]; l++)
      for (uint32_t u : nn[v][l]) rev[u][l].push_back(v);
  std::atomic<size_t> reprunes(0);
  parallel_for(n, threads, 64, [&](size_t i, int) {
    for (int l = 0; l <= g.levels[i]; l++) {
      auto &a = nn[i][l];
      a.insert(a.end(), rev[i][l].begin(), rev[i][l].end());
      std::sort(a.begin(), a.end());
      a.erase(std::unique(a.begin(), a.end()), a.end());
      const size_t limit = l == 0 ? maxM0_ : maxM_;
      if (a.size() <= limit) continue;
      MaxQ heap;
      for (uint32_t u : a) heap.emplace(g.dist(g.vec(i), g.vec(u)), u);
      g.heuristic(heap, limit);
      a.clear();
      while (!heap.empty()) { a.push_back(heap.top().second); heap.pop(); }
      reprunes++;
    }
  });
  n_reprune = reprunes;
}
// The head of the call (:1113-1135): counts and entry from the HNSW index, label_lookup_.merge (keys the Slim index already
// holds keep their id), room for the new elements -- zero, where the reference's realloc leaves them undefined.
inline void diff_begin(SlimGraph &s, const VanillaGraph &g, std::unordered_map<uint64_t, uint32_t> &lookup) {
  s.count = g.count;
  s.has_deleted = g.num_deleted() > 0;
  s.maxlevel = g.maxlevel; s.enterpoint = g.enterpoint;
  for (size_t i = 0; i < g.count; i++) lookup.emplace(g.label((uint32_t)i), (uint32_t)i);
  s.elements.resize(s.count * s.size_per_el, 0);
  s.blobs.resize(s.count);
}
// Elements, blobs and the classification (:1243-1379) from the final lists `list_of(v, l, cnt)`.
template <class GetList>
void diff_assemble(SlimGraph &s, const VanillaGraph &g, size_t prev_count, std::unordered_map<uint64_t, uint32_t> &lookup, int threads,
                   const GetList &list_of, SlimDiff &out) {
  const size_t n = s.count;
  std::vector<uint8_t> cls(n, 0);   // bit 0: old-changed, bit 1: new, bit 2: dirty, bit 3: stale
  parallel_for(n, threads, 256, [&](size_t i, int) {
    const char *e = s.el((uint32_t)i);
    const uint64_t lab = g.label((uint32_t)i);
    const bool stale = i >= prev_count || s.label((uint32_t)i) != lab || memcmp(e + 24, g.vec((uint32_t)i), 4 * s.dim) != 0;
    std::vector<char> prev = std::move(s.blobs[i]);
    s.blobs[i].clear();
    s.assemble_node(g, i, list_of);
    uint8_t c = stale ? 12 : prev != s.blobs[i] ? 4 : 0;
    if (s.total((uint32_t)i) != 0) {   // (a node without neighbours leaves at the `continue` of :1340-1343)
      const bool changed = prev.empty() || prev != s.blobs[i];
      if (lookup.find(lab)->second != i) c |= 2;
      else if (changed) c |= i >= prev_count ? 2 : 1;
    }
    cls[i] = c;
  });
  out.count = n;
  for (size_t i = 0; i < n; i++) {
    if (cls[i] & 1) out.old_ids.push_back((uint32_t)i);
    if (cls[i] & 2) out.new_ids.push_back((uint32_t)i);
    if (cls[i] & 4) out.dirty.push_back((uint32_t)i);
    if (cls[i] & 8) out.stale.push_back((uint32_t)i);
  }
}
// `lookup` is the Slim index's label_lookup_ (buildLabelLookup :216-220 and what earlier calls merged into it).  The Slim
// index keeps its own threshold_level, maxM and maxM0; an empty one takes the capacities of the HNSW index.
inline void convert_diff(SlimGraph &s, const VanillaGraph &g, const SlimParams &p, int threads, std::unordered_map<uint64_t, uint32_t> &lookup,
                         SlimDiff &out) {
  const size_t prev_count = s.count;
  std::vector<std::vector<std::vector<uint32_t>>> nn;
  diff_lists(g, p, s.maxM0, s.maxM, threads, nn, out.n_reprune);
  diff_begin(s, g, lookup);
  diff_assemble(s, g, prev_count, lookup, threads, [&](size_t v, int l, size_t &cnt) { cnt = nn[v][l].size(); return nn[v][l].data(); }, out);
}
// One record of the stream (:1390-1402 old, :1406-1422 new; genPatch :1433-1466): id, the element's first 8 (old) or 16 (new)
// bytes, the blob's size and the blob, and the row of a new node when `with_row`.
inline void diff_record(const SlimGraph &s, std::string &o, uint32_t v, bool is_new, bool with_row) {
  o.append((const char *)&v, 4);
  o.append(s.el(v), is_new ? 16 : 8);
  const uint32_t sz = 2 * (uint32_t)s.level(v) + 4 * s.total(v);
  o.append((const char *)&sz, 4);
  if (sz) o.append(s.blobs[v].data(), s.blobs[v].size());
  if (is_new && with_row) o.append(s.el(v) + 24, 4 * s.dim);
}
inline std::string diff_stream(const SlimGraph &s, const SlimDiff &d) {   // the std::ostream overload's whole output (:1384-1422)
  std::string o;
  const uint64_t h[3] = {d.count, d.old_ids.size(), d.new_ids.size()};
  o.append((const char *)h, 24);
  for (uint32_t v : d.old_ids) diff_record(s, o, v, false, false);
  for (uint32_t v : d.new_ids) diff_record(s, o, v, true, false);
  return o;
}
// genPatch (:1427-1476) from cursors (io, in): the record that reaches `limit` is written and its cursor is NOT advanced (the
// `return` skips the loop increment), so the next call sends that node again; `written` counts a new record's row whether or
// not `to_add` writes it (:1468-1469).  Returns `finished`.
inline uint32_t gen_patch(const SlimGraph &s, const SlimDiff &d, size_t &io, size_t &in, std::string &o, size_t &old_written,
                          size_t &new_written, size_t limit, bool to_add) {
  size_t written = 0;
  for (; io < d.old_ids.size(); io++) {
    old_written++;
    const uint32_t v = d.old_ids[io];
    diff_record(s, o, v, false, false);
    written += 2 * (size_t)s.level(v) + 4 * (size_t)s.total(v) + 4 + 8 + 4;
    if (written >= limit) return 0;
  }
  for (; in < d.new_ids.size(); in++) {
    new_written++;
    const uint32_t v = d.new_ids[in];
    diff_record(s, o, v, true, to_add);
    written += 2 * (size_t)s.level(v) + 4 * (size_t)s.total(v) + 4 + 16 + 4 + 4 * s.dim;
    if (written >= limit) return 0;
  }
  return 1;
}

}  // namespace hs
