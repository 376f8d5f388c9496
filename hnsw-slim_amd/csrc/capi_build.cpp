// capi_build.cpp -- the C ABI (include/hnsw_slim_amd.h): index construction (serial, batched on the host or a device, resumed), the
// four file-to-file graph conversions (Slim and SlimQ, host and device), brute force, and the exact search over a resident index's rows.
#include "capi_internal.hpp"

#include "bf_engine.hpp"
#include "build_engine.hpp"
#include "exact_engine.hpp"
#include "host_rq_batch_build.hpp"
#include "host_rq_graph.hpp"
#include "host_update.hpp"
#include "rabitq_host.hpp"
#include "slim_convert_gpu.hpp"
#include "slimq_chain.hpp"

hs_status hs_build_hnsw(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction,
                        const char *branching_factor, size_t seed, int threads, const char *out_path) {
  return hs_build_hnsw_labeled(base, nullptr, n, dim, metric, M, ef_construction, branching_factor, seed, threads, out_path);
}

hs_status hs_build_hnsw_labeled(const float *base, const uint64_t *labels, size_t n, size_t dim, int metric, size_t M,
                                size_t ef_construction, const char *branching_factor, size_t seed, int threads,
                                const char *out_path) {
  if (!base || !out_path || !branching_factor || n == 0) return fail(HS_ERR_INVALID, "bad argument");
  return guarded([&] {
    VanillaGraph g;
    g.build(base, n, dim, (Metric)metric, M, ef_construction, branching_factor, seed, threads, labels);
    g.save(out_path);
    return HS_OK;
  });
}

// ---- batched addPoint (host_batch_build.hpp; on a device build_gpu.hip) -------------------------------------------------------------
static bool pow2(uint64_t v) { return v && (v & (v - 1)) == 0; }
hs_status batch_opts_ok(const hs_batch_build_opts *opts) {
  if (!opts) return fail(HS_ERR_INVALID, "bad argument");
  if (opts->device < -1) return fail(HS_ERR_INVALID, "device: -1 (the host twin) or a HIP device");
  if (opts->scratch_ids && (!pow2(opts->scratch_ids) || opts->scratch_ids < 64 || opts->scratch_ids > 8192))
    return fail(HS_ERR_INVALID, "scratch_ids: 0 or a power of two from 64 to 8192");
  if (opts->grow_div > 0xFFFFFFFFu || opts->batch_max > 0xFFFFFFFFu) return fail(HS_ERR_INVALID, "grow_div / batch_max out of range");
  return HS_OK;
}

// The device build's lists into the image VanillaGraph::save writes: rows and labels as begin_insert lays them out, the level-0 lists
// in front of them, the upper lists per node, entry point and top level as the schedule ends.
static void image_from_lists(VanillaGraph &g, const float *base, const uint64_t *labels, const std::vector<int> &lv, const std::vector<BatchStep> &steps,
                             const std::vector<uint32_t> &l0, const std::vector<uint32_t> &lu, const std::vector<uint32_t> &upb, int threads) {
  const size_t n = g.max_elements, s0 = g.maxM0 + 1, su = g.maxM + 1;
  parallel_for(n, threads, 1024, [&](size_t i, int) {
    char *e = g.el((uint32_t)i);
    memcpy(e, l0.data() + i * s0, g.size_links0);
    memcpy(e + g.offsetData, base + i * g.dim, 4 * g.dim);
    const uint64_t lab = labels ? labels[i] : i;
    memcpy(e + g.label_offset, &lab, 8);
    g.levels[i] = lv[i];
    if (lv[i]) {
      g.links[i].assign(g.size_links_up * lv[i] + 1, 0);
      memcpy(g.links[i].data(), lu.data() + (size_t)upb[i] * su, g.size_links_up * lv[i]);
    }
  });
  g.count = n;
  for (const BatchStep &s : steps)
    for (uint32_t p = s.begin; p < s.begin + s.size; p++)
      if (lv[p] > g.maxlevel) { g.maxlevel = lv[p]; g.enterpoint = p; }
}

// The batched build on a device, for both graph flavours (rq: rabitqlib's builder, whose labels are the row index -- labels null):
// levels and schedule as the host twin draws them, the kernels of build_gpu.hip, the lists laid into the image of `g`, which the
// caller has initialised for n rows (g.init / rq_init) after its own support test.
static hs_status batched_build_on_device(VanillaGraph &g, bool rq, const float *base, const uint64_t *labels, size_t n, size_t seed,
                                         const hs_batch_build_opts *opts, hs_batch_build_stats &st) {
  const std::vector<int> lv = draw_levels(n, g.mult, seed);
  const std::vector<BatchStep> steps = batch_schedule(lv.data(), n, opts->grow_div, opts->batch_max);
  GpuBuildInput in;
  in.base = base; in.n = (uint32_t)n; in.dim = (uint32_t)g.dim; in.metric = (int)g.metric;
  in.M = (uint32_t)g.M; in.maxM = (uint32_t)g.maxM; in.maxM0 = (uint32_t)g.maxM0; in.efc = (uint32_t)g.efC;
  in.levels = lv.data(); in.steps = &steps; in.scratch_ids = (uint32_t)opts->scratch_ids; in.rq = rq;
  std::vector<uint32_t> l0, lu, upb;
  uint64_t flagged = 0;
  const hipError_t e = gpu_batch_build(in, opts->device, l0, lu, upb, flagged, &st.kernel_ms);
  if (e != hipSuccess) return fail(HS_ERR_DEVICE, std::string("batched build: ") + hipGetErrorString(e));
  image_from_lists(g, base, labels, lv, steps, l0, lu, upb, std::max(1, (int)opts->threads));
  st.used_gpu = 1; st.batches = steps.size(); st.flagged_rows = flagged;
  return HS_OK;
}

hs_status hs_build_hnsw_batched(const float *base, const uint64_t *labels, size_t n, size_t dim, int metric, size_t M, size_t ef_construction,
                                const char *branching_factor, size_t seed, const hs_batch_build_opts *opts, const char *out_path,
                                hs_batch_build_stats *stats) {
  if (!base || !out_path || !branching_factor || n == 0) return fail(HS_ERR_INVALID, "bad argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  if (M == 0) return fail(HS_ERR_INVALID, "M must be > 0");
  if (n > 0x7FFFFFF0u) return fail(HS_ERR_INVALID, "too many rows");
  if (batch_opts_ok(opts) != HS_OK) return HS_ERR_INVALID;
  if (opts->device >= 0 && device_ok(opts->device, false) != HS_OK) return HS_ERR_DEVICE;
  return guarded([&] {
    const auto t0 = std::chrono::steady_clock::now();
    hs_batch_build_stats st{};
    VanillaGraph g;
    bool on_device = false;
    if (opts->device >= 0) {
      g.init(n, dim, (Metric)metric, M, ef_construction, branching_factor);
      on_device = gpu_build_supported((uint32_t)dim, (uint32_t)g.M, (uint32_t)g.efC, (uint32_t)opts->scratch_ids);
    }
    if (on_device) {
      const hs_status s = batched_build_on_device(g, false, base, labels, n, seed, opts, st);
      if (s != HS_OK) return s;
    } else {
      BatchBuildStats bs;
      batch_build_host(g, base, n, dim, (Metric)metric, M, ef_construction, branching_factor, seed, std::max(1, (int)opts->threads), labels, opts->grow_div,
                       opts->batch_max, &bs);
      st.batches = bs.batches;
    }
    g.save(out_path);
    st.total_ms = ms_since(t0);
    if (stats) *stats = st;
    return HS_OK;
  });
}

hs_status hs_build_schedule(size_t n, size_t M, const char *branching_factor, size_t seed, size_t grow_div, size_t batch_max, size_t cap,
                            uint32_t *sizes, uint32_t *entry_points, int32_t *top_levels, size_t *n_batches) {
  if (!branching_factor || !n_batches || n == 0 || M == 0 || n > 0x7FFFFFF0u) return fail(HS_ERR_INVALID, "bad argument");
  return guarded([&] {
    const std::vector<int> lv = draw_levels(n, branching_mult(branching_factor, M), seed);
    const std::vector<BatchStep> steps = batch_schedule(lv.data(), n, grow_div, batch_max);
    *n_batches = steps.size();
    for (size_t b = 0; b < std::min(cap, steps.size()); b++) {
      if (sizes) sizes[b] = steps[b].size;
      if (entry_points) entry_points[b] = steps[b].ep;
      if (top_levels) top_levels[b] = steps[b].top;
    }
    return HS_OK;
  });
}

// What hs_hnsw_resume and hs_hnsw_resume_batched share once their arguments are checked: loadIndex(in_path, space, max_elements), the
// refusals that need the graph -- capacity, a label that exists or appears twice, then `also_refuse` -- all before anything is added
// and with nothing written; the level generator put where a build that has drawn `drawn` levels from `seed` left it; `add`; saveIndex.
template <class Refuse, class Add>
static hs_status resume_file(const char *in_path, int metric, size_t dim, size_t max_elements, const uint64_t *labels, size_t count, size_t seed,
                             size_t drawn, const char *out_path, Refuse &&also_refuse, Add &&add) {
  VanillaGraph g;
  g.load(in_path, (Metric)metric, dim, max_elements);
  if (g.count + count > g.max_elements) return fail(HS_ERR_CAPACITY, "The number of elements exceeds the specified limit");   // hnswalg.h:1274-1277
  std::unordered_set<uint64_t> held;
  held.reserve(g.count);
  for (size_t i = 0; i < g.count; i++) held.insert(g.label((uint32_t)i));
  hs_status s = labels_new_ok([&](uint64_t label) { return held.count(label) != 0; }, labels, count);
  if (s == HS_OK) s = also_refuse(g);
  if (s != HS_OK) return s;
  seed_levels(g, seed, drawn);
  add(g);
  g.save(out_path);
  return HS_OK;
}
static hs_status resume_args_ok(const char *in_path, const char *out_path, int metric, size_t dim, const float *rows, const uint64_t *labels, size_t count) {
  if (!in_path || !out_path || (count && (!rows || !labels))) return fail(HS_ERR_INVALID, "bad argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  return HS_OK;
}

// Continue a saved build on the host: addPoint for each row.
hs_status hs_hnsw_resume(const char *in_path, int metric, size_t dim, size_t max_elements, const float *rows, const uint64_t *labels,
                         size_t count, size_t seed, size_t drawn, int threads, const char *out_path) {
  if (resume_args_ok(in_path, out_path, metric, dim, rows, labels, count) != HS_OK) return HS_ERR_INVALID;
  return guarded([&] {
    return resume_file(in_path, metric, dim, max_elements, labels, count, seed, drawn, out_path, [](const VanillaGraph &) { return HS_OK; },
                       [&](VanillaGraph &g) { resume(g, rows, labels, count, threads); });
  });
}

// hs_hnsw_resume in the batched order, on the host twin: what hs_index_add_points_batched does to a resident index's
// host image, without a device.  The refusals are those of that call, marks included, before anything is added.
hs_status hs_hnsw_resume_batched(const char *in_path, int metric, size_t dim, size_t max_elements, const float *rows, const uint64_t *labels,
                                 size_t count, size_t seed, size_t drawn, const hs_batch_build_opts *opts, const char *out_path,
                                 hs_batch_build_stats *stats) {
  if (resume_args_ok(in_path, out_path, metric, dim, rows, labels, count) != HS_OK) return HS_ERR_INVALID;
  if (batch_opts_ok(opts) != HS_OK) return HS_ERR_INVALID;
  return guarded([&] {
    const auto t0 = std::chrono::steady_clock::now();
    hs_batch_build_stats st{};
    const hs_status s = resume_file(
        in_path, metric, dim, max_elements, labels, count, seed, drawn, out_path,
        [&](const VanillaGraph &g) { return count && g.num_deleted() > 0 ? fail(HS_ERR_UNSUPPORTED, kBatchedAddMarksRefusal) : HS_OK; },
        [&](VanillaGraph &g) {
          BatchBuildStats bs;
          batch_add_host(g, rows, labels, count, std::max(1, (int)opts->threads), opts->grow_div, opts->batch_max, &bs);
          st.batches = bs.batches;
        });
    if (s != HS_OK) return s;
    st.total_ms = ms_since(t0);
    if (stats) *stats = st;
    return HS_OK;
  });
}

// The frame of the four file-to-file converters once their arguments are checked: load the vanilla graph, `step` makes the Slim graph of
// it (and reports used_gpu / kernel_ms), save.
template <class Step>
static hs_status convert_file(const char *hnsw_path, int metric, size_t dim, const char *out_path, Step &&step) {
  return guarded([&] {
    VanillaGraph g;
    g.load(hnsw_path, (Metric)metric, dim);
    SlimGraph s;
    const hs_status st = step(s, g);
    if (st != HS_OK) return st;
    s.save(out_path);
    return HS_OK;
  });
}

hs_status hs_convert_slim(const char *hnsw_path, int metric, size_t dim, int threshold_level, float top_degree_percent0,
                          float top_degree_percent, size_t top_degree_M0, size_t low_degree_m0, size_t top_degree_M,
                          size_t low_degree_m, int threads, const char *out_path) {
  if (!hnsw_path || !out_path) return fail(HS_ERR_INVALID, "bad argument");
  const SlimParams p = slim_params(threshold_level, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0, top_degree_M, low_degree_m);
  return convert_file(hnsw_path, metric, dim, out_path, [&](SlimGraph &s, const VanillaGraph &g) {
    s.convert(g, p, threads);
    return HS_OK;
  });
}

// convertFromHNSW with the list-level work on the GPU (convert_gpu.hip); identical output bytes.  Shapes outside the device path
// (degree capacities or budgets above 64, a source list above 64 ids, a reverse-edge list that outgrows the on-chip buffers) run the CPU conversion instead.
hs_status hs_convert_slim_gpu(const char *hnsw_path, int metric, size_t dim, int threshold_level, float top_degree_percent0,
                              float top_degree_percent, size_t top_degree_M0, size_t low_degree_m0, size_t top_degree_M,
                              size_t low_degree_m, int device, int threads, const char *out_path, int *used_gpu, double *kernel_ms) {
  if (!hnsw_path || !out_path) return fail(HS_ERR_INVALID, "bad argument");
  if (device_ok(device, false) != HS_OK) return HS_ERR_DEVICE;
  const SlimParams p = slim_params(threshold_level, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0, top_degree_M, low_degree_m);
  return convert_file(hnsw_path, metric, dim, out_path,
                      [&](SlimGraph &s, const VanillaGraph &g) { return slim_graph_step(s, g, p, device, threads, used_gpu, kernel_ms); });
}

// HierarchicalNSWSlimQ::convertFromHNSW's graph passes (hnswalg_slimq.h:1546-1762): Slim's passes with SlimQ's own
// PruneByHeuristic (:1334-1362) and rabitqlib's raw distance.  Output: a Slim-layout file for hs_convert_slimq.
hs_status hs_convert_slimq_graph(const char *hnsw_path, int metric, size_t dim, int threshold_level, float top_degree_percent0,
                                 float top_degree_percent, size_t top_degree_M0, size_t low_degree_m0, size_t top_degree_M,
                                 size_t low_degree_m, int threads, const char *out_path) {
  if (!hnsw_path || !out_path) return fail(HS_ERR_INVALID, "bad argument");
  const SlimParams p = slim_params(threshold_level, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0, top_degree_M, low_degree_m);
  return convert_file(hnsw_path, metric, dim, out_path, [&](SlimGraph &s, const VanillaGraph &g) {
    convert_slimq_graph(s, g, p, threads);
    return HS_OK;
  });
}

// The same with the list-level work on a device (convert_slimq.hip); the host conversion for a shape outside the device path.
hs_status hs_convert_slimq_graph_gpu(const char *hnsw_path, int metric, size_t dim, int threshold_level, float top_degree_percent0,
                                     float top_degree_percent, size_t top_degree_M0, size_t low_degree_m0, size_t top_degree_M,
                                     size_t low_degree_m, int device, int threads, const char *out_path, int *used_gpu, double *kernel_ms) {
  if (!hnsw_path || !out_path) return fail(HS_ERR_INVALID, "bad argument");
  hs_status st = metric_ok(metric);
  if (st == HS_OK) st = slimq_device_ok(device);
  if (st != HS_OK) return st;
  const SlimParams p = slim_params(threshold_level, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0, top_degree_M, low_degree_m);
  return convert_file(hnsw_path, metric, dim, out_path,
                      [&](SlimGraph &s, const VanillaGraph &g) { return slimq_graph_step(s, g, p, device, threads, used_gpu, kernel_ms); });
}

// The base graph of HNSW-SlimQ: rabitqlib::hnsw::HierarchicalNSW::construct's edges (RqGraph in host_rq_graph.hpp), stored in the
// vanilla file layout so that the converters read it like any hnswlib index.
hs_status hs_build_rabitq_hnsw(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction, size_t seed,
                               int threads, const char *out_path) {
  if (!base || !out_path || n == 0 || dim == 0) return fail(HS_ERR_INVALID, "bad argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (M < 2) return fail(HS_ERR_INVALID, "M must be >= 2");   // mult = 1 / ln M
  return guarded([&] {
    RqGraph g;
    g.rq_build(base, n, dim, (Metric)metric, M, ef_construction, seed, threads);
    g.save(out_path);
    return HS_OK;
  });
}

// The same graph in the batched order: on a device the rq kernels of build_gpu.hip, otherwise -- device -1, or a
// shape outside the device envelope -- the host twin (host_rq_batch_build.hpp); the same bytes either way.
hs_status rq_batched_args_ok(const float *base, size_t n, size_t dim, int metric, size_t M, const hs_batch_build_opts *opts) {
  if (!base || n == 0 || dim == 0) return fail(HS_ERR_INVALID, "bad argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (M < 2) return fail(HS_ERR_INVALID, "M must be >= 2");   // mult = 1 / ln M
  if (n > 0x7FFFFFF0u) return fail(HS_ERR_INVALID, "too many rows");
  if (batch_opts_ok(opts) != HS_OK) return HS_ERR_INVALID;
  if (opts->device >= 0 && device_ok(opts->device, false) != HS_OK) return HS_ERR_DEVICE;
  return HS_OK;
}
// (throws what the builders throw: the exported entries that call it guard)
hs_status rq_batched_build_into(RqGraph &g, const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction, size_t seed,
                                const hs_batch_build_opts *opts, hs_batch_build_stats &st) {
  if (opts->device >= 0 && gpu_rq_build_supported((uint32_t)dim, (uint32_t)std::min<size_t>(M, 10000), (uint32_t)std::min<size_t>(std::max(ef_construction, M), 0xFFFFFFFFu),
                                                  (uint32_t)opts->scratch_ids)) {
    rq_init(g, base, n, dim, (Metric)metric, M, ef_construction);
    return batched_build_on_device(g, true, base, nullptr, n, seed, opts, st);
  }
  BatchBuildStats bs;
  rq_batch_build_host(g, base, n, dim, (Metric)metric, M, ef_construction, seed, std::max(1, (int)opts->threads), opts->grow_div, opts->batch_max, &bs);
  st.batches = bs.batches;
  return HS_OK;
}
// (the in-memory form, hs_build_rabitq_hnsw_batched_mem in capi_slimq_resident.cpp, followed by hs_graph_save)
hs_status hs_build_rabitq_hnsw_batched(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction, size_t seed,
                                       const hs_batch_build_opts *opts, const char *out_path, hs_batch_build_stats *stats) {
  if (!out_path) return fail(HS_ERR_INVALID, "bad argument");
  const auto t0 = std::chrono::steady_clock::now();
  hs_graph *g = nullptr;
  hs_batch_build_stats st{};
  hs_status s = hs_build_rabitq_hnsw_batched_mem(base, n, dim, metric, M, ef_construction, seed, opts, &g, &st);
  if (s != HS_OK) return s;
  s = hs_graph_save(g, out_path);
  hs_graph_free(g);
  if (s != HS_OK) return s;
  st.total_ms = ms_since(t0);
  if (stats) *stats = st;
  return HS_OK;
}

// rabitq_raw_dist over n_pairs pairs of rows: the host text (device -1), or the wavefront recipe of the build kernels on a device.
hs_status hs_debug_rq_raw_dist(const float *a, const float *b, size_t n_pairs, size_t dim, int metric, int device, float *out) {
  if (!a || !b || !out || dim == 0) return fail(HS_ERR_INVALID, "bad argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (device < -1) return fail(HS_ERR_INVALID, "device: -1 (the host recipe) or a HIP device");
  return guarded([&] {
    if (device < 0) {
      for (size_t i = 0; i < n_pairs; i++) out[i] = rabitq_raw_dist((Metric)metric, a + i * dim, b + i * dim, dim);
      return HS_OK;
    }
    if (dim > 8192) return fail(HS_ERR_UNSUPPORTED, "hs_debug_rq_raw_dist on a device supports dim <= 8192");
    if (device_ok(device, false) != HS_OK) return HS_ERR_DEVICE;
    const hipError_t e = gpu_rq_raw_dist(a, b, n_pairs, (uint32_t)dim, metric, device, out);
    if (e != hipSuccess) return fail(HS_ERR_DEVICE, std::string("rq raw dist: ") + hipGetErrorString(e));
    return HS_OK;
  });
}

// ---- exhaustive k-NN: hnswlib::BruteforceSearch::searchKnn (bruteforce.h:106-135) for a batch ----------------------
hs_status hs_brute_force_dev(const float *d_base, const uint64_t *d_labels, size_t n, size_t dim, int metric,
                             const float *d_queries, size_t nq, size_t k, uint64_t *d_out_labels, float *d_out_dists,
                             uint32_t *d_out_counts, void *stream_) {
  if (!d_base || !d_queries || !d_out_labels || !d_out_dists) return fail(HS_ERR_INVALID, "null argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  if (dim > 4096) return fail(HS_ERR_UNSUPPORTED, "brute force supports dim <= 4096");
  if (k == 0 || k > 64) return fail(HS_ERR_UNSUPPORTED, "brute force supports 1 <= k <= 64");
  if (n > 0xFFFFFFF0u || nq > 0x7FFFFFFFu) return fail(HS_ERR_INVALID, "too many rows / queries");
  if (nq == 0) return HS_OK;
  return guarded([&] {
    hipStream_t stream = (hipStream_t)stream_;
    hipPointerAttribute_t attr;   // run (and allocate the workspace) on the device that holds the rows
    if (hipPointerGetAttributes(&attr, d_base) == hipSuccess) HIP_TRY(hipSetDevice(attr.device));
    uint32_t gx = 0, rpb = 0;
    const size_t bytes = bf_partial_bytes((uint32_t)n, (uint32_t)nq, (uint32_t)k, &gx, &rpb);
    void *partial = nullptr;
    HIP_TRY(hipMalloc(&partial, std::max<size_t>(bytes, 16)));
    hipError_t e = launch_brute_force(d_base, d_labels, (uint32_t)n, (uint32_t)dim, metric, d_queries, (uint32_t)nq, (uint32_t)k, partial, gx,
                                      rpb, d_out_labels, d_out_dists, d_out_counts, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(partial);
    if (e != hipSuccess) return fail(HS_ERR_DEVICE, std::string("brute force: ") + hipGetErrorString(e));
    return HS_OK;
  });
}

hs_status hs_brute_force(const float *base, size_t n, size_t dim, int metric, const uint64_t *labels, const float *queries,
                         size_t nq, size_t k, int device, uint64_t *out_labels, float *out_dists, uint32_t *out_counts) {
  if (!base || !queries || !out_labels || !out_dists) return fail(HS_ERR_INVALID, "null argument");
  if (device_ok(device, true) != HS_OK) return HS_ERR_DEVICE;
  if (nq == 0) return HS_OK;
  return guarded([&] {
    HIP_TRY(hipSetDevice(device));
    DevBuf<float> db, dq, dd;
    DevBuf<uint64_t> dl, dol;
    DevBuf<uint32_t> dc;
    HIP_TRY(db.alloc(std::max<size_t>(n * dim, 1))); HIP_TRY(dq.alloc(nq * dim)); HIP_TRY(dd.alloc(nq * k)); HIP_TRY(dol.alloc(nq * k));
    HIP_TRY(dc.alloc(nq));
    if (labels) { HIP_TRY(dl.alloc(std::max<size_t>(n, 1))); HIP_TRY(hipMemcpy(dl.p, labels, n * 8, hipMemcpyHostToDevice)); }
    HIP_TRY(hipMemcpy(db.p, base, n * dim * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dq.p, queries, nq * dim * 4, hipMemcpyHostToDevice));
    hs_status s = hs_brute_force_dev(db.p, labels ? dl.p : nullptr, n, dim, metric, dq.p, nq, k, dol.p, dd.p, dc.p, nullptr);
    if (s != HS_OK) return s;
    HIP_TRY(hipMemcpy(out_labels, dol.p, nq * k * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, dd.p, nq * k * 4, hipMemcpyDeviceToHost));
    if (out_counts) HIP_TRY(hipMemcpy(out_counts, dc.p, nq * 4, hipMemcpyDeviceToHost));
    return HS_OK;
  });
}

// ---- exact k-NN over the rows a resident index holds (exact_search.hip) -------------------------------------------------
// One launch group: grid.y is a tile of 8 queries and at most 65535.
static constexpr size_t kExactGroupQueries = 262144;

// Everything an exact search is refused for on the host, before anything is launched.
static hs_status exact_use_ok(const hs_index *ix, const hs_filter_set *fs, const void *queries, const void *filter_of_query, size_t nq,
                              size_t k, const void *out_labels64, const void *out_dists) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (!queries || !out_labels64 || !out_dists) return fail(HS_ERR_INVALID, "null argument");
  if ((fs != nullptr) != (filter_of_query != nullptr)) return fail(HS_ERR_INVALID, "a filter set and filter_of_query go together: both or neither");
  if (ix->info.kind == HS_KIND_SLIMQ) return fail(HS_ERR_UNSUPPORTED, "exact search on a SlimQ index is not supported (its rows are RaBitQ records)");
  if (ix->info.dim > 4096) return fail(HS_ERR_UNSUPPORTED, "exact search supports dim <= 4096");
  if (k == 0 || k > 64) return fail(HS_ERR_UNSUPPORTED, "exact search supports 1 <= k <= 64");
  if (exact_lds_bytes((uint32_t)ix->info.dim, (uint32_t)k) > kLdsPerCU)
    return fail(HS_ERR_UNSUPPORTED, "exact search: a tile of 8 queries of dim " + std::to_string(ix->info.dim) + " with k = " + std::to_string(k) + " does not fit the on-chip memory");
  if (nq > 0x7FFFFFFFu) return fail(HS_ERR_INVALID, "nq too large");
  if (fs) {
    if (fs->device != ix->device)
      return fail(HS_ERR_INVALID, "the filter set lives on device " + std::to_string(fs->device) + ", the index on device " + std::to_string(ix->device));
    if (fs->n != ix->info.n)
      return fail(HS_ERR_INVALID, "the filter set was created for " + std::to_string(fs->n) + " elements, the index holds " + std::to_string(ix->info.n));
  }
  return HS_OK;
}

// d_order (nullable): per launch group, a permutation of the group's own query indices.
static hs_status exact_dev(hs_index *ix, const hs_filter_set *fs, const float *d_q, size_t nq, size_t k, const uint32_t *d_foq,
                           const uint32_t *d_order, uint64_t *l64, float *dd, uint32_t *cnt, hipStream_t stream) {
  HIP_TRY(hipSetDevice(ix->device));
  hs_index::StreamWs *w = ix->stream_ws(stream);
  if (w->counters.n < 48) {   // (as search_dev_group: sticky until hs_search_check reads and clears them)
    HIP_TRY(w->counters.ensure(48));
    HIP_TRY(hipMemsetAsync(w->counters.p, 0, 48 * sizeof(uint32_t), stream));
  }
  // the narrow copy where the index has one: fewer bytes, the same bits; the only rows of an fp32-free index
  const int fmt = ix->row_fmt;
  const void *rows = fmt != ROWS_F32 ? (const void *)ix->narrow.p : nullptr;
  const size_t dim = ix->info.dim;
  ix->last_kernel = (dim & 15) ? "hs::exact_scan_general_kernel" : fmt == ROWS_U8 ? "hs::exact_scan_kernel_u8" : fmt == ROWS_F16 ? "hs::exact_scan_kernel_f16" : "hs::exact_scan_kernel";
  for (size_t off = 0; off < nq; off += kExactGroupQueries) {
    const size_t m = std::min(kExactGroupQueries, nq - off);
    ExactArgs a{};
    const size_t bytes = bf_partial_bytes(ix->dev.n, (uint32_t)m, (uint32_t)k, &a.grid_x, &a.rows_per_block);
    HIP_TRY(w->xruns.ensure(std::max<size_t>(bytes, 16)));
    a.queries = d_q + off * dim; a.nq = (uint32_t)m; a.k = (uint32_t)k; a.order = d_order ? d_order + off : nullptr;
    a.partial = w->xruns.p;
    a.out_labels = l64 + off * k; a.out_dists = dd + off * k; a.out_counts = cnt ? cnt + off : nullptr;
    FilterArgs fa{};
    if (fs) fa = FilterArgs{fs->bits.p, d_foq + off, w->counters.p + 12, (uint32_t)fs->row_words, (uint32_t)fs->nf};
    HIP_TRY(launch_exact_search(ix->dev, rows, fmt, a, fs ? &fa : nullptr, stream));
  }
  return HS_OK;
}

hs_status hs_index_exact_search_dev(hs_index *ix, const hs_filter_set *fs, const float *d_queries, size_t nq, size_t k,
                                    const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                    uint32_t *d_out_counts, void *stream) {
  return guarded([&] {
    hs_status s = exact_use_ok(ix, fs, d_queries, d_filter_of_query, nq, k, d_out_labels64, d_out_dists);
    if (s != HS_OK || nq == 0) return s;
    return exact_dev(ix, fs, d_queries, nq, k, d_filter_of_query, nullptr, d_out_labels64, d_out_dists, d_out_counts, (hipStream_t)stream);
  });
}

hs_status hs_index_exact_search(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, size_t k,
                                const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts) {
  return guarded([&] {
    hs_status s = exact_use_ok(ix, fs, queries, filter_of_query, nq, k, out_labels64, out_dists);
    if (s != HS_OK) return s;
    if (fs)
      for (size_t i = 0; i < nq; i++)
        if (filter_of_query[i] >= fs->nf)
          return fail(HS_ERR_INVALID, "query " + std::to_string(i) + " names filter " + std::to_string(filter_of_query[i]) + " of a set of " + std::to_string(fs->nf));
    if (nq == 0) return HS_OK;
    if (device_ok(ix->device, true) != HS_OK) return HS_ERR_DEVICE;
    HIP_TRY(hipSetDevice(ix->device));
    hs_index::StreamWs *w = ix->stream_ws(nullptr);
    const size_t dim = ix->info.dim;
    HIP_TRY(w->aq.ensure(nq * dim)); HIP_TRY(w->al64.ensure(nq * k)); HIP_TRY(w->adist.ensure(nq * k)); HIP_TRY(w->acnt.ensure(nq));
    HIP_TRY(hipMemcpyAsync(w->aq.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, nullptr));
    std::vector<uint32_t> order;   // (outlives the asynchronous copy: the call synchronises before it returns)
    if (fs) {
      // queries of one filter into the same tiles: a tile skips the rows that none of its filters allows
      order.resize(nq);
      for (size_t off = 0; off < nq; off += kExactGroupQueries) {
        const size_t m = std::min(kExactGroupQueries, nq - off);
        for (size_t i = 0; i < m; i++) order[off + i] = (uint32_t)i;
        std::stable_sort(order.begin() + off, order.begin() + off + m,
                         [&](uint32_t x, uint32_t y) { return filter_of_query[off + x] < filter_of_query[off + y]; });
      }
      HIP_TRY(w->afoq.ensure(nq)); HIP_TRY(w->xorder.ensure(nq));
      HIP_TRY(hipMemcpyAsync(w->afoq.p, filter_of_query, nq * 4, hipMemcpyHostToDevice, nullptr));
      HIP_TRY(hipMemcpyAsync(w->xorder.p, order.data(), nq * 4, hipMemcpyHostToDevice, nullptr));
    }
    s = exact_dev(ix, fs, w->aq.p, nq, k, fs ? w->afoq.p : nullptr, fs ? w->xorder.p : nullptr, w->al64.p, w->adist.p, w->acnt.p, nullptr);
    if (s != HS_OK) return s;
    HIP_TRY(hipMemcpyAsync(out_labels64, w->al64.p, nq * k * 8, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpyAsync(out_dists, w->adist.p, nq * k * 4, hipMemcpyDeviceToHost, nullptr));
    if (out_counts) HIP_TRY(hipMemcpyAsync(out_counts, w->acnt.p, nq * 4, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return HS_OK;
  });
}

hs_status hs_convert_slimq(const char *slim_path, int metric, size_t dim, const float *centroids, size_t num_cluster,
                           const uint32_t *cluster_ids, uint64_t flip_seed, int threads, const char *out_path) {
  if (!slim_path || !out_path || !centroids || num_cluster == 0) return fail(HS_ERR_INVALID, "bad argument");
  if (dim < 64 || dim >= 4096) return fail(HS_ERR_UNSUPPORTED, "SlimQ supports 64 <= dim < 4096");
  return guarded([&] {
    SlimGraph s;
    s.load(slim_path, (Metric)metric, dim);
    if (cluster_ids)
      for (size_t i = 0; i < s.count; i++)
        if (cluster_ids[i] >= num_cluster) return fail(HS_ERR_INVALID, "cluster id out of range");
    SlimQGraph q;
    q.from_slim(s, metric, centroids, num_cluster, cluster_ids, flip_seed, threads);
    q.save(out_path);
    return HS_OK;
  });
}
