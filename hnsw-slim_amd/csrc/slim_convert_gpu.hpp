// slim_convert_gpu.hpp -- the host glue of the device conversions (convert_gpu.hip, convert_diff.hip): the task lists they read,
// and the element / blob assembly from the lists they hand back.  Read by the C ABI only: it needs the HIP runtime.
#pragma once
#include <functional>

#include "convert_engine.hpp"
#include "slim_diff.hpp"

namespace hs {

// The task lists of the device conversions (convert_engine.hpp), without the rows.  False: a shape outside the device path.
inline bool make_convert_input(const VanillaGraph &g, const SlimParams &p, const std::vector<size_t> &thr, size_t maxM0, size_t maxM,
                               ConvertInput &in) {
  const size_t n = g.count;
  in.vec = nullptr; in.n = (uint32_t)n; in.dim = (uint32_t)g.dim; in.metric = (int)g.metric;
  // the stride of the pruned / final lists: 32 slots, as for every graph up to M = 16 with budgets up to 32, unless a capacity or
  // a degree budget needs more (the callers have checked that none exceeds 64)
  in.keep = std::max({maxM0, maxM, p.top_M0, p.low_m0, p.top_M, p.low_m}) <= 32 ? 32 : 64;
  in.upb.assign(n, 0);
  size_t nup = 0;
  for (size_t i = 0; i < n; i++) { in.upb[i] = (uint32_t)nup; nup += g.levels[i]; }
  const size_t nt = n + nup;
  in.t_node.resize(nt); in.t_level.resize(nt); in.t_off.resize(nt); in.t_size.resize(nt); in.t_mlim.resize(nt); in.t_limit.resize(nt);
  auto add = [&](size_t t, size_t v, int l) {
    const uint32_t *ll = g.list_at(v, l);
    const size_t size = VanillaGraph::cnt_of(ll);
    in.t_node[t] = (uint32_t)v; in.t_level[t] = (uint32_t)l; in.t_off[t] = (uint32_t)in.lists.size(); in.t_size[t] = (uint32_t)size;
    in.t_mlim[t] = (uint32_t)(l == 0 ? (size > thr[l] ? p.top_M0 : p.low_m0) : (size > thr[l] ? p.top_M : p.low_m));   // :957-961, 969-973
    in.t_limit[t] = (uint32_t)(l == 0 ? maxM0 : maxM);
    in.lists.insert(in.lists.end(), ll + 1, ll + 1 + size);
  };
  in.lists.reserve(n * 16);
  for (size_t v = 0; v < n; v++) add(v, v, 0);
  for (size_t v = 0; v < n; v++)
    for (int l = 1; l <= g.levels[v]; l++) add(n + in.upb[v] + l - 1, v, l);
  for (size_t t = 0; t < nt; t++)
    if (in.t_size[t] > 64) return false;
  // what the device kernels index with: every list entry a node of at least the list's level (the reverse-edge kernels address
  // task n + upb[u] + l - 1 for a level-l edge to u), 32-bit prefix sums and slot numbers (nt * keep).  A file that breaks this takes the CPU conversion.
  if (nt * in.keep >= 0xFFFFFFFFull || in.lists.size() >= 0xFFFFFFFFull || 2 * in.lists.size() >= 0xFFFFFFFFull) return false;
  for (size_t t = 0; t < nt; t++) {
    const uint32_t l = in.t_level[t];
    for (uint32_t j = 0; j < in.t_size[t]; j++) {
      const uint32_t u = in.lists[in.t_off[t] + j];
      if (u >= n || (uint32_t)g.levels[u] < l) return false;
    }
  }
  return true;
}
// The final lists as the device hands them back: in.keep slots per task, task (v, l) where make_convert_input() put it.
struct DeviceLists {
  const ConvertInput &in;
  std::vector<uint32_t> fin, fin_cnt;
  const uint32_t *operator()(size_t v, int l, size_t &cnt) const {
    const size_t t = l == 0 ? v : (size_t)in.n + in.upb[v] + l - 1;
    cnt = fin_cnt[t];
    return fin.data() + t * in.keep;
  }
};

// convert_diff() on the device (convert_diff.hip): the list passes read the rows from `d_vec`, the resident fp32 array of the HNSW
// index; the diff kernel compares the final lists with the Slim index's resident adjacency (dd) and hands back the compacted
// lists; the host then assembles the element and blob of the flagged nodes only and looks up the labels of the nodes whose
// label changed.  Returns false, with `s` untouched, when the shape is outside the device path (capacities or
// degree budgets above 64 ids, a source list above 64, a union above 2048): the caller then runs convert_diff().
// accept (nullable): called with the nodes whose row or label the call would rewrite, before anything changes; false refuses the
// call (*refused set, `s` untouched).
inline bool convert_diff_gpu(SlimGraph &s, const VanillaGraph &g, const SlimParams &p, const float *d_vec, int device, int threads,
                             SlimLookup &lk, DiffDev &dd, SlimDiff &out, double *kernel_ms, std::string *err,
                             const std::function<bool(const std::vector<uint32_t> &)> *accept = nullptr, bool *refused = nullptr) {
  if (g.maxM0 > 64 || g.maxM > 64 || s.maxM0 > 64 || s.maxM > 64 || p.top_M0 > 64 || p.low_m0 > 64 || p.top_M > 64 || p.low_m > 64) return false;
  const size_t prev_count = s.count, n = g.count;
  ConvertInput in;
  if (!make_convert_input(g, p, SlimGraph::hub_thresholds(g, p), s.maxM0, s.maxM, in)) return false;
  dd.levels.assign(g.levels.begin(), g.levels.begin() + n);
  dd.prev_count = (uint32_t)prev_count;
  dd.threshold_level = s.threshold_level;
  dd.want_flags = true;
  DeviceLists lists{in, {}, {}};
  bool needs_host = false;
  uint32_t n_reprune = 0;
  hipError_t e = gpu_convert_diff_lists(in, d_vec, device, lists.fin, lists.fin_cnt, needs_host, n_reprune, kernel_ms, &dd);
  if (e != hipSuccess) {
    if (err) *err = std::string("GPU convert: ") + hipGetErrorString(e);
    return false;
  }
  if (needs_host) return false;
  if (accept && !(*accept)(dd.stale)) {
    if (refused) *refused = true;
    return false;
  }
  if (!lk.mismatch_valid) {
    lk.mismatch.clear();
    for (size_t i = 0; i < prev_count; i++)
      if (lk.map.find(s.label((uint32_t)i))->second != i) lk.mismatch.insert((uint32_t)i);
    lk.mismatch_valid = true;
  }
  out.n_reprune = n_reprune;
  s.count = n;   // the head of the call (:1113-1135); the merge concerns only labels the Slim index does not hold at that id
  s.has_deleted = g.num_deleted() > 0;
  s.maxlevel = g.maxlevel; s.enterpoint = g.enterpoint;
  s.elements.resize(s.count * s.size_per_el, 0);
  s.blobs.resize(s.count);
  for (uint32_t id : dd.stale) {
    lk.mismatch.erase(id);
    if (lk.map.emplace(g.label(id), id).first->second != id) lk.mismatch.insert(id);
  }
  out.count = n;
  out.old_ids = std::move(dd.old_ids); out.new_ids = std::move(dd.new_ids);
  out.dirty = std::move(dd.dirty); out.stale = std::move(dd.stale);
  for (uint32_t id : lk.mismatch) {   // :1360-1362: new whatever its blob did, when it has neighbours
    if (id >= n || !(dd.flags[id] & 2)) continue;
    auto o = std::lower_bound(out.old_ids.begin(), out.old_ids.end(), id);
    if (o != out.old_ids.end() && *o == id) out.old_ids.erase(o);
    auto w = std::lower_bound(out.new_ids.begin(), out.new_ids.end(), id);
    if (w == out.new_ids.end() || *w != id) out.new_ids.insert(w, id);
  }
  parallel_for(out.dirty.size(), threads, 64, [&](size_t k, int) {
    const size_t i = out.dirty[k];
    s.blobs[i].clear();
    s.assemble_node(g, i, lists);
  });
  return true;
}
// convert() with the list-level work on the GPU: `run` is gpu_convert_lists (convert_gpu.hip) or gpu_convert_slimq_lists
// (convert_slimq.hip).  Returns false when the shape is outside the device path (lists longer than 64 / capacities or degree budgets
// above 64 ids, `extra_ok` refusing the task lists, or a reverse-edge list that outgrew the on-chip buffers): the caller then runs the
// host conversion.  kernel_ms: device time of the kernels.
typedef hipError_t (*ConvertListsFn)(const ConvertInput &, int, std::vector<uint32_t> &, std::vector<uint32_t> &, bool &, double *);
inline bool convert_gpu_with(ConvertListsFn run, bool (*extra_ok)(const ConvertInput &), SlimGraph &s, const VanillaGraph &g, const SlimParams &p,
                             int device, int threads, double *kernel_ms, std::string *err) {
  if (g.maxM0 > 64 || g.maxM > 64 || p.top_M0 > 64 || p.low_m0 > 64 || p.top_M > 64 || p.low_m > 64) return false;
  s.take_header(g, p);
  const size_t n = s.count;
  const std::vector<size_t> thr = SlimGraph::hub_thresholds(g, p);
  ConvertInput in;
  if (!make_convert_input(g, p, thr, s.maxM0, s.maxM, in)) return false;
  if (extra_ok && !extra_ok(in)) return false;
  std::vector<float> rows(n * s.dim);
  for (size_t i = 0; i < n; i++) memcpy(&rows[i * s.dim], g.vec(i), 4 * s.dim);
  in.vec = rows.data();
  DeviceLists lists{in, {}, {}};
  bool needs_host = false;
  hipError_t e = run(in, device, lists.fin, lists.fin_cnt, needs_host, kernel_ms);
  if (e != hipSuccess) {
    if (err) *err = std::string("GPU convert: ") + hipGetErrorString(e);
    return false;
  }
  if (needs_host) return false;
  s.elements.assign(n * s.size_per_el, 0);
  s.blobs.assign(n, {});
  parallel_for(n, threads, 256, [&](size_t i, int) { s.assemble_node(g, i, lists); });
  return true;
}
// SlimGraph::convert on the device (convert_gpu.hip)
inline bool convert_gpu(SlimGraph &s, const VanillaGraph &g, const SlimParams &p, int device, int threads, double *kernel_ms, std::string *err) {
  return convert_gpu_with(gpu_convert_lists, nullptr, s, g, p, device, threads, kernel_ms, err);
}
// What the SlimQ kernels need beyond make_convert_input(): a row that fits their LDS, and no source list longer than n -- the
// prune measures candidate i of a list against row i (slimq_prune.hpp), which must exist.  A graph's lists hold distinct neighbours
// other than the node itself, so only a damaged file breaks the second; it then takes the host path, which reads the file as it is.
inline bool cq_input_ok(const ConvertInput &in) {
  if (!gpu_convert_slimq_fits(in.dim)) return false;
  for (uint32_t sz : in.t_size)
    if (sz > in.n) return false;
  return true;
}
// convert_slimq_graph (host_rq_graph.hpp) on the device (convert_slimq.hip)
inline bool convert_slimq_gpu(SlimGraph &s, const VanillaGraph &g, const SlimParams &p, int device, int threads, double *kernel_ms, std::string *err) {
  return convert_gpu_with(gpu_convert_slimq_lists, cq_input_ok, s, g, p, device, threads, kernel_ms, err);
}

}  // namespace hs
