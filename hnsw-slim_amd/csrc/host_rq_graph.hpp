// host_rq_graph.hpp -- the host side of HNSW-SlimQ's graph: rabitqlib's raw distance (rq_dist.hpp), the base graph its HNSW builds (RqGraph)
// and HierarchicalNSWSlimQ::convertFromHNSW's graph passes.  Pinned edge for edge by tests/test_slimq_graph_cpu.py.
#pragma once
#include "host_graph.hpp"
#include "rq_dist.hpp"

namespace hs {

// The base graph HNSW-SlimQ is converted from: rabitqlib::hnsw::HierarchicalNSW::construct
// (third_party/rabitqlib/index/hnsw/hnsw.hpp:667-704, add_point :706-825, search_base_layer :827-905,
// mutually_connect_new_element :907-1014, get_neighbors_by_heuristic2 :1016-1054), as include/strategy/hnsw_slimq_strategy.h:101-133
// drives it (M = 32, ef_construction = 128, seed 100).  It "builds edges with non-quantized vectors" (:696): every distance is
// get_data_dist on the RAW rows (:381-387), so this is hnswlib's insertion algorithm with three differences that change the graph:
// the heaps order (distance, id) PAIRS lexicographically (maxheap = std::priority_queue<pair>, minheap with std::greater, :33-36)
// instead of by distance alone, maxM = M and maxM0 = 2 M with mult = 1 / ln M (:445-493), and a neighbour that already lists the
// new node is not connected twice (:973-980).  Storage and file layout are VanillaGraph's (hnswalg.h:748-779), so the Slim / SlimQ
// converters read it like any vanilla index.
struct RqGraph : VanillaGraph {
  typedef std::pair<float, uint32_t> P;
  typedef std::priority_queue<P> MaxH;
  typedef std::priority_queue<P, std::vector<P>, std::greater<P>> MinH;
  float ddist(uint32_t a, uint32_t b) const { return rabitq_raw_dist(metric, vec(a), vec(b), dim); }

  MaxH rq_search_layer(uint32_t ep, uint32_t cur_c, int layer, Visited &vl) {   // :827-905
    vl.begin(max_elements);
    MaxH top;
    MinH cand;
    float lower = ddist(ep, cur_c);
    top.emplace(lower, ep);
    cand.emplace(lower, ep);
    vl.mass[ep] = vl.cur;
    while (!cand.empty()) {
      const P c = cand.top();
      if (c.first > lower && top.size() == efC) break;
      cand.pop();
      const uint32_t node = c.second;
      std::unique_lock<std::mutex> lk(locks[node]);
      const uint32_t *l = list_at(node, layer);
      const size_t n = cnt_of(l);
      for (size_t j = 0; j < n; j++) {
        const uint32_t id = l[1 + j];
        if (vl.mass[id] == vl.cur) continue;
        vl.mass[id] = vl.cur;
        const float d = ddist(id, cur_c);
        if (top.size() < efC || lower > d) {
          cand.emplace(d, id);
          top.emplace(d, id);
          if (top.size() > efC) top.pop();
          if (!top.empty()) lower = top.top().first;
        }
      }
    }
    return top;
  }
  void rq_heuristic(MaxH &top, size_t Mlim) const {   // :1016-1054
    if (top.size() < Mlim) return;
    MinH closest;
    std::vector<P> keep;
    while (!top.empty()) { closest.emplace(top.top()); top.pop(); }
    while (!closest.empty()) {
      if (keep.size() >= Mlim) break;
      const P cur = closest.top();
      closest.pop();
      bool good = true;
      for (const P &sp : keep)
        if (ddist(sp.second, cur.second) < cur.first) { good = false; break; }
      if (good) keep.push_back(cur);
    }
    for (const P &pp : keep) top.emplace(pp);
  }
  uint32_t rq_connect(uint32_t cur_c, MaxH &top, int level) {   // :907-1014
    const size_t max_m = level > 0 ? maxM : maxM0;
    rq_heuristic(top, M);
    if (top.size() > M) throw std::runtime_error("Should be not be more than M_ candidates returned by the heuristic");
    std::vector<uint32_t> sel;
    sel.reserve(M);
    while (!top.empty()) { sel.push_back(top.top().second); top.pop(); }
    const uint32_t next_ep = sel.back();
    {
      uint32_t *l = list_at(cur_c, level);
      if (*l) throw std::runtime_error("The newly inserted element should have blank link list");
      set_cnt(l, sel.size());
      for (size_t i = 0; i < sel.size(); i++) {
        if (l[1 + i]) throw std::runtime_error("Possible memory corruption");
        if (level > levels[sel[i]]) throw std::runtime_error("Trying to make a link on a non-existent level");
        l[1 + i] = sel[i];
      }
    }
    for (uint32_t nb : sel) {
      std::unique_lock<std::mutex> lk(locks[nb]);
      uint32_t *lo = list_at(nb, level);
      const size_t sz = cnt_of(lo);
      if (sz > max_m) throw std::runtime_error("Bad value of sz_link_list_other");
      if (nb == cur_c) throw std::runtime_error("Trying to connect an element to itself");
      if (level > levels[nb]) throw std::runtime_error("Trying to make a link on a non-existent level");
      uint32_t *data = lo + 1;
      bool present = false;
      for (size_t j = 0; j < sz; j++)
        if (data[j] == cur_c) { present = true; break; }
      if (present) continue;
      if (sz < max_m) {
        data[sz] = cur_c;
        set_cnt(lo, sz + 1);
      } else {
        MaxH cands;
        cands.emplace(ddist(nb, cur_c), cur_c);
        for (size_t j = 0; j < sz; j++) cands.emplace(ddist(data[j], nb), data[j]);
        rq_heuristic(cands, max_m);
        int idx = 0;
        while (!cands.empty()) { data[idx++] = cands.top().second; cands.pop(); }
        set_cnt(lo, idx);
      }
    }
    return next_ep;
  }
  void rq_add_point(const float *x, uint32_t cur_c, int curlevel, Visited &vl) {   // :706-825 (label == internal id)
    const Insert in = begin_insert(x, cur_c, cur_c, curlevel);
    if ((int32_t)in.ep != -1) {
      uint32_t curr = in.ep;
      if (curlevel < in.maxlevelcopy) {
        float curdist = ddist(curr, cur_c);
        descend(curr, curdist, in.maxlevelcopy, curlevel, true, [&](uint32_t c) { return ddist(c, cur_c); });
      }
      for (int level = std::min(curlevel, in.maxlevelcopy); level >= 0; level--) {
        MaxH top = rq_search_layer(curr, cur_c, level, vl);
        curr = rq_connect(cur_c, top, level);
      }
    }
    adopt_entry(cur_c, curlevel, in);
  }
  // rows 0..n-1, labels == row index; levels drawn up front in row order from std::default_random_engine(seed) (:222, 324-328, 477),
  // so threads == 1 reproduces the reference's serial construct(); threads > 1 is as timing-dependent as the reference's own
  // parallel_for (:698-703) but keeps ids == labels (the SlimQ rerank indexes raw rows by internal id, hnswalg_slimq.h:748).
  void rq_build(const float *base, size_t n, size_t d, Metric m, size_t M_, size_t efC_, size_t seed, int threads) {
    init(n, d, m, M_, efC_, "e");
    mult = 1 / log(1.0 * (double)M);   // :493
    std::default_random_engine gen;
    gen.seed(seed);
    std::vector<int> lv(n);
    for (size_t i = 0; i < n; i++) lv[i] = level_from(gen, mult);
    if (threads < 1) threads = 1;
    // the new element's row must be in place before anyone measures against it: rows are copied by rq_add_point itself, and
    // get_data_dist(x, cur_c) reads row cur_c -> copy every row first (the reference reads rawDataPtr_, which is complete;
    // rq_add_point clears the element and writes the same row again)
    for (size_t i = 0; i < n; i++) memcpy(el((uint32_t)i) + offsetData, base + i * d, 4 * d);
    std::vector<Visited> vl(threads);
    const size_t serial_head = threads > 1 ? std::min<size_t>(n, 1) : n;
    for (size_t i = 0; i < serial_head; i++) { count = i + 1; rq_add_point(base + i * d, (uint32_t)i, lv[i], vl[0]); }
    count = n;
    parallel_for(n - serial_head, threads, 1, [&](size_t k, int tid) {
      const size_t i = serial_head + k;
      rq_add_point(base + i * d, (uint32_t)i, lv[i], vl[tid]);
    });
  }
};

// HierarchicalNSWSlimQ's own PruneByHeuristic (hnswalg_slimq.h:1334-1362), mirrored as written: the occlusion test measures the
// candidate against the node whose INTERNAL ID is the loop index i over the sorted candidates (`hnsw->get_data_dist(i, ...)`,
// :1349), not against the neighbours kept so far, and only once something has been kept.
inline void prune_slimq(const VanillaGraph &g, const std::vector<pairfi> &sorted, std::vector<uint32_t> &out, size_t Mlim) {
  out.clear();
  for (size_t i = 0; i < sorted.size(); i++) {
    if (out.size() >= Mlim) break;
    const pairfi &cur = sorted[i];
    bool good = true;
    if (!out.empty()) {
      float d = rabitq_raw_dist(g.metric, g.vec((uint32_t)i), g.vec(cur.second), g.dim);
      if (d < cur.first) good = false;
    }
    if (good) out.push_back(cur.second);
  }
}
// HierarchicalNSWSlimQ::convertFromHNSW's graph part (hnswalg_slimq.h:1471-1762): SlimGraph::convert's passes with its own
// PruneByHeuristic and hnsw->get_data_dist (:1623, 1706).
inline void convert_slimq_graph(SlimGraph &s, const VanillaGraph &g, const SlimParams &p, int threads) {
  s.convert(g, p, threads,
            [](const VanillaGraph &gg, const std::vector<pairfi> &sorted, std::vector<uint32_t> &out, size_t Mlim) { prune_slimq(gg, sorted, out, Mlim); },
            [&](uint32_t a, uint32_t b) { return rabitq_raw_dist(g.metric, g.vec(a), g.vec(b), g.dim); });
}

}  // namespace hs
