// packed_index.hpp -- what the GPU consumes: vectors row-major + CSR adjacency (level 0 and upper levels), labels, delete
// flags -- produced from either host image (host_graph.hpp).
#pragma once
#include "host_graph.hpp"

namespace hs {

// Device-facing packed form.  Level-0 adjacency is plain CSR (row_ptr0[n+1], cols); nodes with upper
// levels own (level+1) consecutive entries of up_ptr starting at up_base[i]: the level-l slice
// (l >= 1) is cols[up_ptr[up_base[i]+l-1] .. up_ptr[up_base[i]+l]).
struct PackedIndex {
  int kind = 0;  // 0 = HierarchicalNSW, 1 = HierarchicalNSWSlim
  Metric metric = METRIC_L2;
  size_t n = 0, dim = 0;
  int maxlevel = 0, threshold_level = 0;
  uint32_t enterpoint = 0;
  bool has_deleted = false;
  size_t max_deg0 = 0;
  size_t index_size = 0;   // what the reference's indexSize() reports for this index (graph structure without vectors)
  std::vector<float> vec;
  bool rows_on_device = false;   // `vec` left empty on purpose: the device already holds the n rows (from_vanilla(g, false))
  size_t row_values() const { return rows_on_device ? n * dim : vec.size(); }
  std::vector<uint32_t> row_ptr0, cols, up_base, up_ptr;
  std::vector<uint64_t> labels;
  std::vector<uint8_t> deleted;

  static constexpr uint32_t NONE = 0xFFFFFFFFu;

  // Does some level-0 list name an id twice?  (Legal: the reference skips the second occurrence through its visited array,
  // hnswalg.h:392-393.  The flat kernel marks the ids of one expansion in all lanes at once and so needs them distinct: the
  // launch plan keeps an index with such a list off it, search_plan.cpp.)  One pass over the edges: seen[id] = the last list
  // that named id.
  bool repeats_id0() const {
    std::vector<uint32_t> seen(n, NONE);
    for (size_t i = 0; i < n; i++)
      for (size_t j = row_ptr0[i]; j < row_ptr0[i + 1]; j++) {
        const uint32_t c = cols[j];
        if (c >= n) continue;
        if (seen[c] == (uint32_t)i) return true;
        seen[c] = (uint32_t)i;
      }
    return false;
  }

  // with_rows = false (hs_index_add_points, whose device rows are written record by record): `vec` stays empty
  void from_vanilla(const VanillaGraph &g, bool with_rows = true) {
    kind = 0; metric = g.metric; n = g.count; dim = g.dim;
    // HierarchicalNSW::indexSize() (hnswalg.h:1533-1547): level-0 block without vectors and labels, element_levels_,
    // one pointer per element + its upper link lists (+1 as malloc'd)
    index_size = g.max_elements * (g.size_per_el - g.dim * 4 - 8) + g.max_elements * sizeof(int);
    for (size_t i = 0; i < g.count; i++) index_size += 8 + (g.levels[i] > 0 ? g.size_links_up * (size_t)g.levels[i] + 1 : 0);
    maxlevel = g.maxlevel; threshold_level = 0; enterpoint = g.enterpoint;
    rows_on_device = !with_rows;
    vec.resize(with_rows ? n * dim : 0); labels.resize(n); deleted.resize(n);
    row_ptr0.assign(n + 1, 0); up_base.assign(n, NONE); up_ptr.clear(); cols.clear();
    max_deg0 = 0;
    size_t nd = 0;
    for (size_t i = 0; i < n; i++) {
      if (with_rows) memcpy(&vec[i * dim], g.vec(i), 4 * dim);
      labels[i] = g.label(i);
      deleted[i] = g.deleted(i);
      nd += deleted[i];
      const uint32_t *l = g.list_at(i, 0);
      size_t c = VanillaGraph::cnt_of(l);
      max_deg0 = std::max(max_deg0, c);
      cols.insert(cols.end(), l + 1, l + 1 + c);
      row_ptr0[i + 1] = cols.size();
    }
    has_deleted = nd > 0;
    for (size_t i = 0; i < n; i++) {
      int L = g.levels[i];
      if (L <= 0) continue;
      up_base[i] = up_ptr.size();
      for (int l = 1; l <= L; l++) {
        up_ptr.push_back(cols.size());
        const uint32_t *ll = g.list_at(i, l);
        cols.insert(cols.end(), ll + 1, ll + 1 + VanillaGraph::cnt_of(ll));
      }
      up_ptr.push_back(cols.size());
    }
    if (cols.size() >= NONE) throw std::runtime_error("adjacency too large for 32-bit CSR offsets");
  }

  // CHAL blobs ([u16 cumulative offsets x level][u32 ids x total], hnswalg_slim.h:1981-2000) -> CSR.
  // level_of(i), total_of(i), blob_of(i) -> const std::vector<char>&
  template <class LF, class TF, class BF>
  void pack_chal(LF level_of, TF total_of, BF blob_of) {
    row_ptr0.assign(n + 1, 0); up_base.assign(n, NONE); up_ptr.clear(); cols.clear();
    auto slice = [&](size_t i, int lvl, const uint32_t *&ids, size_t &cnt) {   // (index_check.hpp P5: the one copy of the offsets test)
      if (!chal_slice(level_of(i), total_of(i), blob_of(i), lvl, ids, cnt)) throw std::runtime_error(kCorruptText);
    };
    for (size_t i = 0; i < n; i++) {
      if (!blob_of(i).empty()) {
        const uint32_t *ids; size_t c;
        slice(i, 0, ids, c);
        max_deg0 = std::max(max_deg0, c);
        cols.insert(cols.end(), ids, ids + c);
      }
      row_ptr0[i + 1] = cols.size();
    }
    for (size_t i = 0; i < n; i++) {
      const int L = level_of(i);
      if (L <= 0 || blob_of(i).empty()) continue;
      up_base[i] = up_ptr.size();
      for (int l = 1; l <= L; l++) {
        up_ptr.push_back(cols.size());
        const uint32_t *ids; size_t c;
        slice(i, l, ids, c);
        cols.insert(cols.end(), ids, ids + c);
      }
      up_ptr.push_back(cols.size());
    }
    for (uint32_t c : cols) if (c >= n) throw std::runtime_error("Index seems to be corrupted or unsupported");
    if (cols.size() >= NONE) throw std::runtime_error("adjacency too large for 32-bit CSR offsets");
  }

  // with_rows = false (hs_slim_convert_diff, whose device rows are written record by record): `vec` stays empty
  void from_slim(const SlimGraph &g, bool with_rows = true) {
    kind = 1; metric = g.metric; n = g.count; dim = g.dim;
    // HierarchicalNSWSlim::indexSize() (hnswalg_slim.h:2435-2444): 16 bytes per element + every neighbour blob
    index_size = g.count * 16;
    for (size_t i = 0; i < g.count; i++) index_size += 2 * (size_t)g.level((uint32_t)i) + 4 * (size_t)g.total((uint32_t)i);
    maxlevel = g.maxlevel; threshold_level = g.threshold_level; enterpoint = g.enterpoint;
    has_deleted = g.has_deleted;
    rows_on_device = !with_rows;
    vec.resize(with_rows ? n * dim : 0); labels.resize(n); deleted.resize(n);
    for (size_t i = 0; i < n; i++) {
      if (with_rows) memcpy(&vec[i * dim], g.vec(i), 4 * dim);
      labels[i] = g.label(i);
      deleted[i] = g.deleted(i);
    }
    pack_chal([&](size_t i) { return (int)g.level(i); }, [&](size_t i) { return (size_t)g.total(i); },
              [&](size_t i) -> const std::vector<char> & { return g.blobs[i]; });
  }
};

}  // namespace hs
