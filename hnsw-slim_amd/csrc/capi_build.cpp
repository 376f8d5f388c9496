// capi_build.cpp -- the C ABI (include/hnsw_slim_amd.h): index construction (serial, batched on the host or a device, resumed), the
// four file-to-file graph conversions (Slim and SlimQ, host and device), brute force, and the exact search over a resident index's rows.
#include "capi_internal.hpp"

#include "bf_engine.hpp"
#include "build_engine.hpp"
#include "exact_engine.hpp"
#include "exact_screen_engine.hpp"
#include "exact_screen_margin.hpp"
#include "exact_screen_f16q_engine.hpp"
#include "exact_screen_f8q_engine.hpp"
#include "exact_screen_q8_engine.hpp"
#include "exact_wide_engine.hpp"
#include "exact_range_engine.hpp"
#include "exact_range_screen_engine.hpp"
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

// Rows of format `fmt` (ROWS_*: fp32, or u8 / fp16 in natural order) as fp32: both widenings are exact.  dst: 4-byte aligned.
template <class T>
static void widen_to(const void *src, size_t first, size_t count, float *dst) {
  const T *s = static_cast<const T *>(src) + first;
  for (size_t i = 0; i < count; i++) dst[i] = (float)s[i];
}
static void rows_as_f32(const void *src, int fmt, size_t first, size_t count, float *dst) {
  if (fmt == ROWS_U8) widen_to<uint8_t>(src, first, count, dst);
  else if (fmt == ROWS_F16) widen_to<_Float16>(src, first, count, dst);
  else memcpy(dst, static_cast<const float *>(src) + first, 4 * count);
}

// The device build's lists into the image VanillaGraph::save writes: rows (fp32, whatever format they were built from) and labels as
// begin_insert lays them out, the level-0 lists in front of them, the upper lists per node, entry point and top level as the schedule ends.
static void image_from_lists(VanillaGraph &g, const void *base, int fmt, const uint64_t *labels, const std::vector<int> &lv, const std::vector<BatchStep> &steps,
                             const std::vector<uint32_t> &l0, const std::vector<uint32_t> &lu, const std::vector<uint32_t> &upb, int threads) {
  const size_t n = g.max_elements, s0 = g.maxM0 + 1, su = g.maxM + 1;
  parallel_for(n, threads, 1024, [&](size_t i, int) {
    char *e = g.el((uint32_t)i);
    memcpy(e, l0.data() + i * s0, g.size_links0);
    rows_as_f32(base, fmt, i * g.dim, g.dim, reinterpret_cast<float *>(e + g.offsetData));   // (every offset of an element is a multiple of 4)
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
static hs_status batched_build_on_device(VanillaGraph &g, bool rq, const void *base, int fmt, const uint64_t *labels, size_t n, size_t seed,
                                         const hs_batch_build_opts *opts, hs_batch_build_stats &st) {
  const std::vector<int> lv = draw_levels(n, g.mult, seed);
  const std::vector<BatchStep> steps = batch_schedule(lv.data(), n, opts->grow_div, opts->batch_max);
  GpuBuildInput in;
  in.base = base; in.rows = fmt; in.n = (uint32_t)n; in.dim = (uint32_t)g.dim; in.metric = (int)g.metric;
  in.M = (uint32_t)g.M; in.maxM = (uint32_t)g.maxM; in.maxM0 = (uint32_t)g.maxM0; in.efc = (uint32_t)g.efC;
  in.levels = lv.data(); in.steps = &steps; in.scratch_ids = (uint32_t)opts->scratch_ids; in.rq = rq;
  std::vector<uint32_t> l0, lu, upb;
  uint64_t flagged = 0;
  const hipError_t e = gpu_batch_build(in, opts->device, l0, lu, upb, flagged, &st.kernel_ms);
  if (e != hipSuccess) return fail(HS_ERR_DEVICE, std::string("batched build: ") + hipGetErrorString(e));
  image_from_lists(g, base, fmt, labels, lv, steps, l0, lu, upb, std::max(1, (int)opts->threads));
  st.used_gpu = 1; st.batches = steps.size(); st.flagged_rows = flagged;
  return HS_OK;
}

// hs_build_hnsw_batched and hs_build_hnsw_batched_rows: the refusals of their arguments, then the build from rows of format `fmt`
// (throws what the builders throw: the two entries guard).  The device reads the rows as they lie at `base`; the host twin reads
// fp32 rows, the caller's or their widening.
static hs_status batched_args_ok(const void *base, size_t n, size_t dim, int metric, size_t M, const char *branching_factor,
                                 const hs_batch_build_opts *opts, const char *out_path) {
  if (!base || !out_path || !branching_factor || n == 0) return fail(HS_ERR_INVALID, "bad argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  if (M == 0) return fail(HS_ERR_INVALID, "M must be > 0");
  if (n > 0x7FFFFFF0u) return fail(HS_ERR_INVALID, "too many rows");
  if (batch_opts_ok(opts) != HS_OK) return HS_ERR_INVALID;
  if (opts->device >= 0 && device_ok(opts->device, false) != HS_OK) return HS_ERR_DEVICE;
  return HS_OK;
}
static hs_status batched_build_file(const void *base, int fmt, const uint64_t *labels, size_t n, size_t dim, int metric, size_t M,
                                    size_t ef_construction, const char *branching_factor, size_t seed, const hs_batch_build_opts *opts,
                                    const char *out_path, hs_batch_build_stats *stats) {
  const auto t0 = std::chrono::steady_clock::now();
  hs_batch_build_stats st{};
  VanillaGraph g;
  bool on_device = false;
  if (opts->device >= 0) {
    g.init(n, dim, (Metric)metric, M, ef_construction, branching_factor);
    on_device = gpu_build_supported((uint32_t)dim, (uint32_t)g.M, (uint32_t)g.efC, (uint32_t)opts->scratch_ids);
  }
  if (on_device) {
    const hs_status s = batched_build_on_device(g, false, base, fmt, labels, n, seed, opts, st);
    if (s != HS_OK) return s;
  } else {
    std::vector<float> wide;
    if (fmt != ROWS_F32) {
      wide.resize(n * dim);
      rows_as_f32(base, fmt, 0, n * dim, wide.data());
    }
    const float *rows = fmt != ROWS_F32 ? wide.data() : static_cast<const float *>(base);
    BatchBuildStats bs;
    batch_build_host(g, rows, n, dim, (Metric)metric, M, ef_construction, branching_factor, seed, std::max(1, (int)opts->threads), labels, opts->grow_div,
                     opts->batch_max, &bs);
    st.batches = bs.batches;
  }
  g.save(out_path);
  st.total_ms = ms_since(t0);
  if (stats) *stats = st;
  return HS_OK;
}
hs_status hs_build_hnsw_batched(const float *base, const uint64_t *labels, size_t n, size_t dim, int metric, size_t M, size_t ef_construction,
                                const char *branching_factor, size_t seed, const hs_batch_build_opts *opts, const char *out_path,
                                hs_batch_build_stats *stats) {
  const hs_status ok = batched_args_ok(base, n, dim, metric, M, branching_factor, opts, out_path);
  if (ok != HS_OK) return ok;
  return guarded([&] {
    return batched_build_file(base, ROWS_F32, labels, n, dim, metric, M, ef_construction, branching_factor, seed, opts, out_path, stats);
  });
}
// The same build from u8 / fp16 rows in natural order: on a device the narrow instantiations of the two row-reading
// kernels; the file is hs_build_hnsw_batched's for the widened rows, byte for byte.
hs_status hs_build_hnsw_batched_rows(const void *base, int row_format, const uint64_t *labels, size_t n, size_t dim, int metric, size_t M,
                                     size_t ef_construction, const char *branching_factor, size_t seed, const hs_batch_build_opts *opts,
                                     const char *out_path, hs_batch_build_stats *stats) {
  if (row_format != ROWS_F16 && row_format != ROWS_U8) return fail(HS_ERR_INVALID, "bad row format (HS_ROWS_U8 or HS_ROWS_F16)");
  const hs_status ok = batched_args_ok(base, n, dim, metric, M, branching_factor, opts, out_path);
  if (ok != HS_OK) return ok;
  return guarded([&] {
    if (row_format == ROWS_F16) {   // NaN and +-inf (exponent all ones) are outside the format's contract, as for an index's narrow copy
      const uint16_t *w = static_cast<const uint16_t *>(base);
      for (size_t i = 0; i < n * dim; i++)
        if ((w[i] & 0x7C00u) == 0x7C00u) {
          float v;
          rows_as_f32(base, ROWS_F16, i, 1, &v);
          return fail(HS_ERR_UNSUPPORTED, unfit_message(i / dim, i % dim, v, ROWS_F16));
        }
    }
    return batched_build_file(base, row_format, labels, n, dim, metric, M, ef_construction, branching_factor, seed, opts, out_path, stats);
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
    return batched_build_on_device(g, true, base, ROWS_F32, nullptr, n, seed, opts, st);
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
                              size_t k, const void *out_labels64, const void *out_dists, bool wide = false) {
  // (the wide entries' limit needs no index: refused first, so that it is reachable without one)
  if (wide && (k == 0 || k > kWideMaxK)) return fail(HS_ERR_UNSUPPORTED, "exact search (wide) supports 1 <= k <= 1024");
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (!queries || !out_labels64 || !out_dists) return fail(HS_ERR_INVALID, "null argument");
  if ((fs != nullptr) != (filter_of_query != nullptr)) return fail(HS_ERR_INVALID, "a filter set and filter_of_query go together: both or neither");
  if (ix->info.kind == HS_KIND_SLIMQ) return fail(HS_ERR_UNSUPPORTED, "exact search on a SlimQ index is not supported (its rows are RaBitQ records)");
  if (ix->info.dim > 4096) return fail(HS_ERR_UNSUPPORTED, "exact search supports dim <= 4096");
  // up to 64 the wide entries are the scan's; above, every dim <= 4096 has a tile that fits (xw_tile: 72 KB for two queries of dim 4096, k = 1024)
  if (!wide || k <= 64) {
    if (k == 0 || k > 64) return fail(HS_ERR_UNSUPPORTED, "exact search supports 1 <= k <= 64");
    if (exact_lds_bytes((uint32_t)ix->info.dim, (uint32_t)k) > kLdsPerCU)
      return fail(HS_ERR_UNSUPPORTED, "exact search: a tile of 8 queries of dim " + std::to_string(ix->info.dim) + " with k = " + std::to_string(k) + " does not fit the on-chip memory");
  }
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
// screened: through exact_screen.hip where its envelope holds (dim % 16 == 0 and a tile that fits the on-chip memory), the scan otherwise.
static hs_status exact_dev(hs_index *ix, const hs_filter_set *fs, const float *d_q, size_t nq, size_t k, const uint32_t *d_foq,
                           const uint32_t *d_order, uint64_t *l64, float *dd, uint32_t *cnt, hipStream_t stream, bool want_screen = false) {
  HIP_TRY(hipSetDevice(ix->device));
  hs_index::StreamWs *w = ix->stream_ws(stream);
  const bool screened = want_screen && xs_supported((uint32_t)ix->info.dim, (uint32_t)k);
  if (w->counters.n < 48) {   // (as search_dev_group: sticky until hs_search_check reads and clears them)
    HIP_TRY(w->counters.ensure(48));
    HIP_TRY(hipMemsetAsync(w->counters.p, 0, 48 * sizeof(uint32_t), stream));
  }
  // the narrow copy where the index has one: fewer bytes, the same bits; the only rows of an fp32-free index
  const int fmt = ix->row_fmt;
  const void *rows = fmt != ROWS_F32 ? (const void *)ix->narrow.p : nullptr;
  const size_t dim = ix->info.dim;
  ix->last_kernel = screened ? xs_kernel_name(fmt)
                    : (dim & 15) ? "hs::exact_scan_general_kernel" : fmt == ROWS_U8 ? "hs::exact_scan_kernel_u8" : fmt == ROWS_I8 ? "hs::exact_scan_kernel_i8" : fmt == ROWS_BF16 ? "hs::exact_scan_kernel_bf16" : fmt == ROWS_F8 ? "hs::exact_scan_kernel_f8" : fmt == ROWS_F16 ? "hs::exact_scan_kernel_f16" : "hs::exact_scan_kernel";
  const size_t gq = std::min(kExactGroupQueries, nq);
  if (screened) {
    HIP_TRY(w->xs_norms.ensure((size_t)ix->dev.n + gq));
    HIP_TRY(w->xs_state.ensure(kXsStateWords + 2 * gq));
    size_t cand = 16;   // the largest any group of the call needs: a full group and the last one
    for (size_t m : {gq, nq - (nq - 1) / kExactGroupQueries * kExactGroupQueries}) {
      uint32_t gx, rpb;
      cand = std::max(cand, xs_plan(ix->dev.n, (uint32_t)m, (uint32_t)k, &gx, &rpb));
    }
    HIP_TRY(w->xs_cand.ensure(cand));
    HIP_TRY(launch_exact_screen_norms(ix->dev, rows, fmt, w->xs_norms.p, stream));
  }
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
    if (!screened) {
      HIP_TRY(launch_exact_search(ix->dev, rows, fmt, a, fs ? &fa : nullptr, stream));
      continue;
    }
    ScreenArgs sa{};
    sa.x = a;
    sa.first_group = off == 0;
    xs_plan(ix->dev.n, (uint32_t)m, (uint32_t)k, &sa.grid_x, &sa.rows_per_block);
    sa.xnorm2 = w->xs_norms.p; sa.qnorm2 = w->xs_norms.p + ix->dev.n;
    sa.cand = w->xs_cand.p;
    sa.state = w->xs_state.p; sa.qflag = w->xs_state.p + kXsStateWords; sa.fb_order = sa.qflag + gq;
    HIP_TRY(launch_exact_screen(ix->dev, rows, fmt, sa, fs ? &fa : nullptr, stream));
  }
  if (want_screen) {   // (the plain entries leave the last screened call's stats alone)
    ix->xs_last = screened ? w : nullptr;
    ix->xs_last_nq = nq;
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

// ---- 64 < k <= 1024 (exact_wide.hip) --------------------------------------------------------------------------------------------
// exact_dev's arguments; k <= 64 is exact_dev's own call.
static hs_status exact_wide_dev(hs_index *ix, const hs_filter_set *fs, const float *d_q, size_t nq, size_t k, const uint32_t *d_foq,
                                const uint32_t *d_order, uint64_t *l64, float *dd, uint32_t *cnt, hipStream_t stream) {
  if (k <= 64) return exact_dev(ix, fs, d_q, nq, k, d_foq, d_order, l64, dd, cnt, stream);
  HIP_TRY(hipSetDevice(ix->device));
  hs_index::StreamWs *w = ix->stream_ws(stream);
  if (w->counters.n < 48) {   // (as exact_dev)
    HIP_TRY(w->counters.ensure(48));
    HIP_TRY(hipMemsetAsync(w->counters.p, 0, 48 * sizeof(uint32_t), stream));
  }
  const int fmt = ix->row_fmt;
  const void *rows = fmt != ROWS_F32 ? (const void *)ix->narrow.p : nullptr;
  const size_t dim = ix->info.dim;
  const uint32_t qt = xw_tile((uint32_t)dim, (uint32_t)k);
  ix->last_kernel = xw_kernel_name((uint32_t)dim, fmt);
  for (size_t off = 0; off < nq; off += kExactGroupQueries) {
    const size_t m = std::min(kExactGroupQueries, nq - off);
    ExactArgs a{};
    const size_t bytes = xw_plan(ix->dev.n, (uint32_t)m, (uint32_t)k, qt, &a.grid_x, &a.rows_per_block);
    HIP_TRY(w->xruns.ensure(std::max<size_t>(bytes, 16)));
    a.queries = d_q + off * dim; a.nq = (uint32_t)m; a.k = (uint32_t)k; a.order = d_order ? d_order + off : nullptr;
    a.partial = w->xruns.p;
    a.out_labels = l64 + off * k; a.out_dists = dd + off * k; a.out_counts = cnt ? cnt + off : nullptr;
    FilterArgs fa{};
    if (fs) fa = FilterArgs{fs->bits.p, d_foq + off, w->counters.p + 12, (uint32_t)fs->row_words, (uint32_t)fs->nf};
    HIP_TRY(launch_exact_wide(ix->dev, rows, fmt, a, fs ? &fa : nullptr, stream));
  }
  return HS_OK;
}

hs_status hs_index_exact_search_wide_dev(hs_index *ix, const hs_filter_set *fs, const float *d_queries, size_t nq, size_t k,
                                         const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                         uint32_t *d_out_counts, void *stream) {
  return guarded([&] {
    hs_status s = exact_use_ok(ix, fs, d_queries, d_filter_of_query, nq, k, d_out_labels64, d_out_dists, true);
    if (s != HS_OK || nq == 0) return s;
    return exact_wide_dev(ix, fs, d_queries, nq, k, d_filter_of_query, nullptr, d_out_labels64, d_out_dists, d_out_counts, (hipStream_t)stream);
  });
}

// ---- byte queries over byte rows (exact_screen_q8.hip) ------------------------------------------------------------------------
// What the byte-query entries refuse beyond exact_use_ok.
static hs_status exact_q8_use_ok(const hs_index *ix, int query_format) {
  if (query_format != HS_ROWS_U8 && query_format != HS_ROWS_I8) return fail(HS_ERR_INVALID, kQ8QueryFormatRefusal);
  if (ix->row_fmt == ROWS_F32 || !ix->narrow.p) return fail(HS_ERR_INVALID, kQ8NoNarrowRefusal);
  if (ix->row_fmt != query_format) return fail(HS_ERR_INVALID, kQ8FormatMismatchRefusal);
  return HS_OK;
}

// exact_dev's arguments with the queries as bytes of the rows' format.  A shape the integer kernel does not take is widened and handed
// to the fp32 screen.
static hs_status exact_q8_dev(hs_index *ix, const hs_filter_set *fs, const void *d_q, int qfmt, size_t nq, size_t k, const uint32_t *d_foq,
                              const uint32_t *d_order, uint64_t *l64, float *dd, uint32_t *cnt, hipStream_t stream) {
  HIP_TRY(hipSetDevice(ix->device));
  hs_index::StreamWs *w = ix->stream_ws(stream);
  const size_t dim = ix->info.dim;
  const int fmt = ix->row_fmt;
  if (!xq_supported(fmt, (uint32_t)dim, (uint32_t)k)) {
    HIP_TRY(w->xq_wide.ensure(nq * dim));
    HIP_TRY(launch_exact_q8_widen(d_q, qfmt, nq * dim, w->xq_wide.p, stream));
    return exact_dev(ix, fs, w->xq_wide.p, nq, k, d_foq, d_order, l64, dd, cnt, stream, true);
  }
  if (w->counters.n < 48) {   // (as exact_dev)
    HIP_TRY(w->counters.ensure(48));
    HIP_TRY(hipMemsetAsync(w->counters.p, 0, 48 * sizeof(uint32_t), stream));
  }
  const void *rows = ix->narrow.p;
  ix->last_kernel = xq_kernel_name(fmt);
  const size_t gq = std::min(kExactGroupQueries, nq);
  const size_t row_bytes = ((size_t)ix->dev.n * sizeof(XqRow) + 15) / 16 * 16;
  HIP_TRY(w->xq_info.ensure(row_bytes + gq * sizeof(XqQuery)));
  HIP_TRY(w->xq_packed.ensure(gq * dim));
  HIP_TRY(w->xq_wide.ensure(gq * dim));
  HIP_TRY(w->xs_state.ensure(kXsStateWords + 2 * gq));
  size_t cand = 16;   // the largest any group of the call needs: a full group and the last one
  for (size_t m : {gq, nq - (nq - 1) / kExactGroupQueries * kExactGroupQueries}) {
    uint32_t gx, rpb;
    cand = std::max(cand, xs_plan(ix->dev.n, (uint32_t)m, (uint32_t)k, &gx, &rpb));
  }
  HIP_TRY(w->xs_cand.ensure(cand));
  XqRow *rinfo = reinterpret_cast<XqRow *>(w->xq_info.p);
  HIP_TRY(launch_exact_q8_rownorms(ix->dev, rows, fmt, rinfo, stream));
  for (size_t off = 0; off < nq; off += kExactGroupQueries) {
    const size_t m = std::min(kExactGroupQueries, nq - off);
    ScreenArgs sa{};
    const size_t bytes = bf_partial_bytes(ix->dev.n, (uint32_t)m, (uint32_t)k, &sa.x.grid_x, &sa.x.rows_per_block);
    HIP_TRY(w->xruns.ensure(std::max<size_t>(bytes, 16)));
    sa.x.queries = w->xq_wide.p; sa.x.nq = (uint32_t)m; sa.x.k = (uint32_t)k; sa.x.order = d_order ? d_order + off : nullptr;
    sa.x.partial = w->xruns.p;
    sa.x.out_labels = l64 + off * k; sa.x.out_dists = dd + off * k; sa.x.out_counts = cnt ? cnt + off : nullptr;
    FilterArgs fa{};
    if (fs) fa = FilterArgs{fs->bits.p, d_foq + off, w->counters.p + 12, (uint32_t)fs->row_words, (uint32_t)fs->nf};
    sa.first_group = off == 0;
    xs_plan(ix->dev.n, (uint32_t)m, (uint32_t)k, &sa.grid_x, &sa.rows_per_block);
    sa.cand = w->xs_cand.p;
    sa.state = w->xs_state.p; sa.qflag = w->xs_state.p + kXsStateWords; sa.fb_order = sa.qflag + gq;
    XqArgs qa{};
    qa.queries = static_cast<const uint8_t *>(d_q) + off * dim;
    qa.packed = w->xq_packed.p; qa.wide = w->xq_wide.p;
    qa.qinfo = reinterpret_cast<XqQuery *>(w->xq_info.p + row_bytes); qa.rinfo = rinfo;
    HIP_TRY(launch_exact_screen_q8(ix->dev, rows, fmt, sa, qa, fs ? &fa : nullptr, stream));
  }
  ix->xs_last = w;
  ix->xs_last_nq = nq;
  return HS_OK;
}

// ---- fp16 queries over fp16 rows (exact_screen_f16q.hip), bf16 queries over bf16 rows (exact_screen_bf16q.hip), fp8 queries over
// fp8 rows (exact_screen_f8q.hip) -------------------------------------------------------------------------------------------------
// exact_host's codes for "the queries are halves" / "bf16 words" / "E4M3 bytes": not row formats of the byte-query entry, which keeps
// refusing all three.
static constexpr int kQueriesF16 = -16, kQueriesBF16 = -17, kQueriesF8 = -8;
static bool half_queries(int qfmt) { return qfmt == kQueriesF16 || qfmt == kQueriesBF16 || qfmt == kQueriesF8; }
// the launch entries of the three objects (exact_screen_f16q_engine.hpp, exact_screen_f8q_engine.hpp: one interface)
struct HalfScreen {
  int rows;
  size_t width;   // bytes per query element
  const char *refusal;
  decltype(&xh_supported) supported;
  decltype(&xh_kernel_name) kernel_name;
  decltype(&launch_exact_f16q_rowinfo) rowinfo;
  decltype(&launch_exact_f16q_widen) widen;
  decltype(&launch_exact_screen_f16q) screen;
};
static const HalfScreen &half_screen(int qfmt) {
  static const HalfScreen f16{ROWS_F16, 2, kF16QNoCopyRefusal, xh_supported, xh_kernel_name, launch_exact_f16q_rowinfo, launch_exact_f16q_widen, launch_exact_screen_f16q};
  static const HalfScreen bf16{ROWS_BF16, 2, kBF16QNoCopyRefusal, xb_supported, xb_kernel_name, launch_exact_bf16q_rowinfo, launch_exact_bf16q_widen, launch_exact_screen_bf16q};
  static const HalfScreen f8{ROWS_F8, 1, kF8QNoCopyRefusal, xf_supported, xf_kernel_name, launch_exact_f8q_rowinfo, launch_exact_f8q_widen, launch_exact_screen_f8q};
  return qfmt == kQueriesBF16 ? bf16 : qfmt == kQueriesF8 ? f8 : f16;
}

// What the fp16-query entries refuse beyond exact_use_ok.  No index of dim % 16 != 0 can hold a narrow copy (hs_index_set_row_format):
// such a call is handed over whatever rows the index has.
static hs_status exact_f16q_use_ok(const hs_index *ix, int qfmt = kQueriesF16) {
  const HalfScreen &hsc = half_screen(qfmt);
  if ((ix->info.dim & 15) == 0 && (ix->row_fmt != hsc.rows || !ix->narrow.p)) return fail(HS_ERR_INVALID, hsc.refusal);
  return HS_OK;
}

// exact_dev's arguments with the queries as halves (qfmt = kQueriesBF16: as bf16 words).  A shape the 16-bit kernel does not take is
// widened and handed to the route the fp32 queries take.
static hs_status exact_f16q_dev(hs_index *ix, const hs_filter_set *fs, const void *d_q, size_t nq, size_t k, const uint32_t *d_foq,
                                const uint32_t *d_order, uint64_t *l64, float *dd, uint32_t *cnt, hipStream_t stream, int qfmt = kQueriesF16) {
  const HalfScreen &hsc = half_screen(qfmt);
  HIP_TRY(hipSetDevice(ix->device));
  hs_index::StreamWs *w = ix->stream_ws(stream);
  const size_t dim = ix->info.dim;
  if (!hsc.supported(ix->row_fmt, (uint32_t)dim, (uint32_t)k)) {
    HIP_TRY(w->xq_wide.ensure(nq * dim));
    HIP_TRY(hsc.widen(d_q, nq * dim, w->xq_wide.p, stream));
    return exact_dev(ix, fs, w->xq_wide.p, nq, k, d_foq, d_order, l64, dd, cnt, stream, true);
  }
  if (w->counters.n < 48) {   // (as exact_dev)
    HIP_TRY(w->counters.ensure(48));
    HIP_TRY(hipMemsetAsync(w->counters.p, 0, 48 * sizeof(uint32_t), stream));
  }
  const void *rows = ix->narrow.p;
  ix->last_kernel = hsc.kernel_name();
  const size_t gq = std::min(kExactGroupQueries, nq);
  const size_t row_bytes = ((size_t)ix->dev.n * sizeof(XhInfo) + 15) / 16 * 16;
  HIP_TRY(w->xq_info.ensure(row_bytes + gq * sizeof(XhInfo)));
  HIP_TRY(w->xq_packed.ensure(gq * dim * 2));
  HIP_TRY(w->xq_wide.ensure(gq * dim));
  HIP_TRY(w->xs_state.ensure(kXsStateWords + 2 * gq));
  size_t cand = 16;   // the largest any group of the call needs: a full group and the last one
  for (size_t m : {gq, nq - (nq - 1) / kExactGroupQueries * kExactGroupQueries}) {
    uint32_t gx, rpb;
    cand = std::max(cand, xs_plan(ix->dev.n, (uint32_t)m, (uint32_t)k, &gx, &rpb));
  }
  HIP_TRY(w->xs_cand.ensure(cand));
  XhInfo *rinfo = reinterpret_cast<XhInfo *>(w->xq_info.p);
  HIP_TRY(hsc.rowinfo(ix->dev, rows, rinfo, stream));
  for (size_t off = 0; off < nq; off += kExactGroupQueries) {
    const size_t m = std::min(kExactGroupQueries, nq - off);
    ScreenArgs sa{};
    const size_t bytes = bf_partial_bytes(ix->dev.n, (uint32_t)m, (uint32_t)k, &sa.x.grid_x, &sa.x.rows_per_block);
    HIP_TRY(w->xruns.ensure(std::max<size_t>(bytes, 16)));
    sa.x.queries = w->xq_wide.p; sa.x.nq = (uint32_t)m; sa.x.k = (uint32_t)k; sa.x.order = d_order ? d_order + off : nullptr;
    sa.x.partial = w->xruns.p;
    sa.x.out_labels = l64 + off * k; sa.x.out_dists = dd + off * k; sa.x.out_counts = cnt ? cnt + off : nullptr;
    FilterArgs fa{};
    if (fs) fa = FilterArgs{fs->bits.p, d_foq + off, w->counters.p + 12, (uint32_t)fs->row_words, (uint32_t)fs->nf};
    sa.first_group = off == 0;
    xs_plan(ix->dev.n, (uint32_t)m, (uint32_t)k, &sa.grid_x, &sa.rows_per_block);
    sa.cand = w->xs_cand.p;
    sa.state = w->xs_state.p; sa.qflag = w->xs_state.p + kXsStateWords; sa.fb_order = sa.qflag + gq;
    XhArgs qa{};
    qa.queries = static_cast<const unsigned char *>(d_q) + off * dim * hsc.width;
    qa.packed = reinterpret_cast<uint16_t *>(w->xq_packed.p); qa.wide = w->xq_wide.p;
    qa.qinfo = reinterpret_cast<XhInfo *>(w->xq_info.p + row_bytes); qa.rinfo = rinfo;
    HIP_TRY(hsc.screen(ix->dev, rows, sa, qa, fs ? &fa : nullptr, stream));
  }
  ix->xs_last = w;
  ix->xs_last_nq = nq;
  return HS_OK;
}

// qfmt: the element type of `queries` -- ROWS_F32; ROWS_U8 / ROWS_I8 for the byte-query entry, kQueriesF16 / kQueriesBF16 / kQueriesF8 for the
// fp16-, bf16- and fp8-query entries (all always screened).
static hs_status exact_host(hs_index *ix, const hs_filter_set *fs, const void *queries, int qfmt, size_t nq, size_t k, const uint32_t *filter_of_query,
                            uint64_t *out_labels64, float *out_dists, uint32_t *out_counts, bool screened, bool wide = false) {
  return guarded([&] {
    hs_status s = exact_use_ok(ix, fs, queries, filter_of_query, nq, k, out_labels64, out_dists, wide);
    if (s == HS_OK && qfmt != ROWS_F32) s = half_queries(qfmt) ? exact_f16q_use_ok(ix, qfmt) : exact_q8_use_ok(ix, qfmt);
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
    HIP_TRY(w->al64.ensure(nq * k)); HIP_TRY(w->adist.ensure(nq * k)); HIP_TRY(w->acnt.ensure(nq));
    if (qfmt == ROWS_F32) {
      HIP_TRY(w->aq.ensure(nq * dim));
      HIP_TRY(hipMemcpyAsync(w->aq.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, nullptr));
    } else {
      const size_t qbytes = nq * dim * (half_queries(qfmt) ? half_screen(qfmt).width : 1);
      HIP_TRY(w->xq_in.ensure(qbytes));
      HIP_TRY(hipMemcpyAsync(w->xq_in.p, queries, qbytes, hipMemcpyHostToDevice, nullptr));
    }
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
    const uint32_t *d_foq = fs ? w->afoq.p : nullptr, *d_order = fs ? w->xorder.p : nullptr;
    s = wide                  ? exact_wide_dev(ix, fs, w->aq.p, nq, k, d_foq, d_order, w->al64.p, w->adist.p, w->acnt.p, nullptr)
        : qfmt == ROWS_F32    ? exact_dev(ix, fs, w->aq.p, nq, k, d_foq, d_order, w->al64.p, w->adist.p, w->acnt.p, nullptr, screened)
        : half_queries(qfmt) ? exact_f16q_dev(ix, fs, w->xq_in.p, nq, k, d_foq, d_order, w->al64.p, w->adist.p, w->acnt.p, nullptr, qfmt)
                              : exact_q8_dev(ix, fs, w->xq_in.p, qfmt, nq, k, d_foq, d_order, w->al64.p, w->adist.p, w->acnt.p, nullptr);
    if (s != HS_OK) return s;
    HIP_TRY(hipMemcpyAsync(out_labels64, w->al64.p, nq * k * 8, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpyAsync(out_dists, w->adist.p, nq * k * 4, hipMemcpyDeviceToHost, nullptr));
    if (out_counts) HIP_TRY(hipMemcpyAsync(out_counts, w->acnt.p, nq * 4, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return HS_OK;
  });
}

hs_status hs_index_exact_search(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, size_t k,
                                const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts) {
  return exact_host(ix, fs, queries, ROWS_F32, nq, k, filter_of_query, out_labels64, out_dists, out_counts, false);
}

hs_status hs_index_exact_search_wide(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, size_t k,
                                     const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts) {
  return exact_host(ix, fs, queries, ROWS_F32, nq, k, filter_of_query, out_labels64, out_dists, out_counts, false, true);
}

// ---- every row within a radius (exact_range.hip) ---------------------------------------------------------------------------------
static hs_status range_use_ok(const hs_index *ix, const hs_filter_set *fs, const void *queries, const void *radius, const void *filter_of_query,
                              size_t nq, size_t cap, const void *out_offsets, const void *out_labels64, const void *out_dists) {
  // (what needs no index comes first, so that it is reachable without one)
  if (!radius || !out_offsets) return fail(HS_ERR_INVALID, "null argument (radius, out_offsets)");
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (cap && (!out_labels64 || !out_dists)) return fail(HS_ERR_INVALID, "null argument");
  // the rest is the scan's at k = 1 (the outputs were looked at above: cap == 0 may come without them)
  return exact_use_ok(ix, fs, queries, filter_of_query, nq, 1, out_offsets, out_offsets);
}

// The call's workspace on `stream` and the arguments both passes share; a.cap and the outputs are the caller's to set.
static hs_status range_args(hs_index *ix, const hs_filter_set *fs, const float *d_q, const float *d_radius, size_t nq, const uint32_t *d_foq,
                            const uint32_t *d_order, uint64_t *d_offsets, hipStream_t stream, RangeArgs &a, FilterArgs &fa) {
  hs_index::StreamWs *w = ix->stream_ws(stream);
  if (w->counters.n < 48) {   // (as exact_dev)
    HIP_TRY(w->counters.ensure(48));
    HIP_TRY(hipMemsetAsync(w->counters.p, 0, 48 * sizeof(uint32_t), stream));
  }
  ix->last_kernel = xr_kernel_name((uint32_t)ix->info.dim, ix->row_fmt);
  a = RangeArgs{};
  a.queries = d_q; a.radius = d_radius; a.nq = (uint32_t)nq; a.order = d_order;
  xr_plan(ix->dev.n, (uint32_t)nq, &a.chunks, &a.rows_per_chunk);
  HIP_TRY(w->xr_counts.ensure(std::max<size_t>(nq * a.chunks, 1)));
  HIP_TRY(w->xr_bases.ensure(std::max<size_t>(nq * a.chunks, 1)));
  a.counts = w->xr_counts.p; a.bases = w->xr_bases.p; a.out_offsets = d_offsets;
  a.over = w->counters.p + 13;
  fa = FilterArgs{};
  if (fs) fa = FilterArgs{fs->bits.p, d_foq, w->counters.p + 12, (uint32_t)fs->row_words, (uint32_t)fs->nf};
  return HS_OK;
}
// the narrow copy where the index has one (as exact_dev)
static const void *range_rows(const hs_index *ix) { return ix->row_fmt != ROWS_F32 ? (const void *)ix->narrow.p : nullptr; }

// The screened route's workspace on the call's stream behind range_args: norms, state words, flags, fallback order, cursors, lists.
static hs_status range_screen_args(hs_index *ix, size_t nq, hipStream_t stream, const RangeArgs &a, RangeScreenArgs &sa) {
  hs_index::StreamWs *w = ix->stream_ws(stream);
  HIP_TRY(w->xs_norms.ensure((size_t)ix->dev.n + nq));
  HIP_TRY(w->xs_state.ensure(kXsStateWords + 3 * nq));
  HIP_TRY(w->xrs_lists.ensure(xrs_list_words((uint32_t)nq)));
  sa = RangeScreenArgs{};
  sa.r = a;
  sa.xnorm2 = w->xs_norms.p; sa.qnorm2 = w->xs_norms.p + ix->dev.n;
  xrs_plan(ix->dev.n, (uint32_t)nq, &sa.grid_y, &sa.rows_per_block);
  sa.state = w->xs_state.p; sa.qflag = w->xs_state.p + kXsStateWords; sa.fb_order = sa.qflag + nq; sa.cursor = sa.fb_order + nq;
  sa.lists = w->xrs_lists.p;
  ix->last_kernel = xrs_kernel_name(ix->row_fmt);
  return HS_OK;
}
// want_screen: through exact_range_screen.hip where its envelope holds (dim % 16 == 0), the two passes of exact_range.hip otherwise.
static bool range_screened(hs_index *ix, size_t nq, hipStream_t stream, bool want_screen) {
  const bool screened = want_screen && nq != 0 && xrs_supported((uint32_t)ix->info.dim);
  if (want_screen) {   // (the plain entries leave the last screened call's stats alone)
    ix->xs_last = screened ? ix->stream_ws(stream) : nullptr;
    ix->xs_last_nq = nq;
  }
  return screened;
}

static hs_status range_dev(hs_index *ix, const hs_filter_set *fs, const float *d_queries, size_t nq, const float *d_radius,
                           const uint32_t *d_filter_of_query, size_t cap, uint64_t *d_out_offsets, uint64_t *d_out_labels64,
                           float *d_out_dists, void *stream, bool want_screen) {
  return guarded([&] {
    hs_status s = range_use_ok(ix, fs, d_queries, d_radius, d_filter_of_query, nq, cap, d_out_offsets, d_out_labels64, d_out_dists);
    if (s != HS_OK) return s;
    HIP_TRY(hipSetDevice(ix->device));
    RangeArgs a;
    FilterArgs fa;
    s = range_args(ix, fs, d_queries, d_radius, nq, d_filter_of_query, nullptr, d_out_offsets, (hipStream_t)stream, a, fa);
    if (s != HS_OK) return s;
    a.cap = cap; a.out_labels = d_out_labels64; a.out_dists = d_out_dists;
    if (range_screened(ix, nq, (hipStream_t)stream, want_screen)) {
      RangeScreenArgs sa;
      s = range_screen_args(ix, nq, (hipStream_t)stream, a, sa);
      if (s != HS_OK) return s;
      HIP_TRY(launch_exact_range_screen_count(ix->dev, range_rows(ix), ix->row_fmt, sa, fs ? &fa : nullptr, (hipStream_t)stream));
      HIP_TRY(launch_exact_range_screen_fill(ix->dev, range_rows(ix), ix->row_fmt, sa, fs ? &fa : nullptr, (hipStream_t)stream));
      return HS_OK;
    }
    HIP_TRY(launch_exact_range_count(ix->dev, range_rows(ix), ix->row_fmt, a, fs ? &fa : nullptr, (hipStream_t)stream));
    HIP_TRY(launch_exact_range_fill(ix->dev, range_rows(ix), ix->row_fmt, a, fs ? &fa : nullptr, (hipStream_t)stream));
    return HS_OK;
  });
}

static hs_status range_host(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, const float *radius,
                            const uint32_t *filter_of_query, size_t cap, uint64_t *out_offsets, uint64_t *out_labels64, float *out_dists,
                            bool want_screen) {
  return guarded([&] {
    hs_status s = range_use_ok(ix, fs, queries, radius, filter_of_query, nq, cap, out_offsets, out_labels64, out_dists);
    if (s != HS_OK) return s;
    if (fs)
      for (size_t i = 0; i < nq; i++)
        if (filter_of_query[i] >= fs->nf)
          return fail(HS_ERR_INVALID, "query " + std::to_string(i) + " names filter " + std::to_string(filter_of_query[i]) + " of a set of " + std::to_string(fs->nf));
    if (nq == 0) {
      out_offsets[0] = 0;
      return HS_OK;
    }
    if (device_ok(ix->device, true) != HS_OK) return HS_ERR_DEVICE;
    HIP_TRY(hipSetDevice(ix->device));
    hs_index::StreamWs *w = ix->stream_ws(nullptr);
    const size_t dim = ix->info.dim;
    HIP_TRY(w->aq.ensure(nq * dim)); HIP_TRY(w->xr_radius.ensure(nq)); HIP_TRY(w->xr_off.ensure(nq + 1));
    HIP_TRY(hipMemcpyAsync(w->aq.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipMemcpyAsync(w->xr_radius.p, radius, nq * sizeof(float), hipMemcpyHostToDevice, nullptr));
    std::vector<uint32_t> order;   // (outlives the asynchronous copy: the call synchronises before it returns)
    if (fs) {
      // queries of one filter into the same tiles: a tile skips the rows that none of its filters allows
      order.resize(nq);
      for (size_t i = 0; i < nq; i++) order[i] = (uint32_t)i;
      std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return filter_of_query[x] < filter_of_query[y]; });
      HIP_TRY(w->afoq.ensure(nq)); HIP_TRY(w->xorder.ensure(nq));
      HIP_TRY(hipMemcpyAsync(w->afoq.p, filter_of_query, nq * 4, hipMemcpyHostToDevice, nullptr));
      HIP_TRY(hipMemcpyAsync(w->xorder.p, order.data(), nq * 4, hipMemcpyHostToDevice, nullptr));
    }
    RangeArgs a;
    FilterArgs fa;
    s = range_args(ix, fs, w->aq.p, w->xr_radius.p, nq, fs ? w->afoq.p : nullptr, fs ? w->xorder.p : nullptr, w->xr_off.p, nullptr, a, fa);
    if (s != HS_OK) return s;
    const bool screened = range_screened(ix, nq, nullptr, want_screen);
    RangeScreenArgs sa;
    if (screened) {
      s = range_screen_args(ix, nq, nullptr, a, sa);
      if (s != HS_OK) return s;
      HIP_TRY(launch_exact_range_screen_count(ix->dev, range_rows(ix), ix->row_fmt, sa, fs ? &fa : nullptr, nullptr));
    } else {
      HIP_TRY(launch_exact_range_count(ix->dev, range_rows(ix), ix->row_fmt, a, fs ? &fa : nullptr, nullptr));
    }
    HIP_TRY(hipMemcpyAsync(out_offsets, w->xr_off.p, (nq + 1) * 8, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    const uint64_t total = out_offsets[nq];
    if (total > cap)   // refused up front: the fill is not launched
      return fail(HS_ERR_CAPACITY, "exact range: " + std::to_string(total) + " results, cap " + std::to_string(cap) + " (out_offsets is written: call again with cap >= the total)");
    if (total == 0) return HS_OK;
    HIP_TRY(w->al64.ensure(total)); HIP_TRY(w->adist.ensure(total));
    if (screened) {
      sa.r.cap = total; sa.r.out_labels = w->al64.p; sa.r.out_dists = w->adist.p;
      HIP_TRY(launch_exact_range_screen_fill(ix->dev, range_rows(ix), ix->row_fmt, sa, fs ? &fa : nullptr, nullptr));
    } else {
      a.cap = total; a.out_labels = w->al64.p; a.out_dists = w->adist.p;
      HIP_TRY(launch_exact_range_fill(ix->dev, range_rows(ix), ix->row_fmt, a, fs ? &fa : nullptr, nullptr));
    }
    HIP_TRY(hipMemcpyAsync(out_labels64, w->al64.p, total * 8, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpyAsync(out_dists, w->adist.p, total * 4, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return HS_OK;
  });
}

hs_status hs_index_exact_range_dev(hs_index *ix, const hs_filter_set *fs, const float *d_queries, size_t nq, const float *d_radius,
                                   const uint32_t *d_filter_of_query, size_t cap, uint64_t *d_out_offsets, uint64_t *d_out_labels64,
                                   float *d_out_dists, void *stream) {
  return range_dev(ix, fs, d_queries, nq, d_radius, d_filter_of_query, cap, d_out_offsets, d_out_labels64, d_out_dists, stream, false);
}
hs_status hs_index_exact_range(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, const float *radius,
                               const uint32_t *filter_of_query, size_t cap, uint64_t *out_offsets, uint64_t *out_labels64, float *out_dists) {
  return range_host(ix, fs, queries, nq, radius, filter_of_query, cap, out_offsets, out_labels64, out_dists, false);
}
// ---- the same answers by screen, re-rank and fallback (exact_range_screen.hip) -----------------------------------------------
hs_status hs_index_exact_range_screened_dev(hs_index *ix, const hs_filter_set *fs, const float *d_queries, size_t nq, const float *d_radius,
                                            const uint32_t *d_filter_of_query, size_t cap, uint64_t *d_out_offsets, uint64_t *d_out_labels64,
                                            float *d_out_dists, void *stream) {
  return range_dev(ix, fs, d_queries, nq, d_radius, d_filter_of_query, cap, d_out_offsets, d_out_labels64, d_out_dists, stream, true);
}
hs_status hs_index_exact_range_screened(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, const float *radius,
                                        const uint32_t *filter_of_query, size_t cap, uint64_t *out_offsets, uint64_t *out_labels64,
                                        float *out_dists) {
  return range_host(ix, fs, queries, nq, radius, filter_of_query, cap, out_offsets, out_labels64, out_dists, true);
}

// ---- the same answers by screen, re-rank and fallback (exact_screen.hip) -------------------------------------------------------
hs_status hs_index_exact_search_screened(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, size_t k,
                                         const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts) {
  return exact_host(ix, fs, queries, ROWS_F32, nq, k, filter_of_query, out_labels64, out_dists, out_counts, true);
}
hs_status hs_index_exact_search_screened_dev(hs_index *ix, const hs_filter_set *fs, const float *d_queries, size_t nq, size_t k,
                                             const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                             uint32_t *d_out_counts, void *stream) {
  return guarded([&] {
    hs_status s = exact_use_ok(ix, fs, d_queries, d_filter_of_query, nq, k, d_out_labels64, d_out_dists);
    if (s != HS_OK || nq == 0) return s;
    return exact_dev(ix, fs, d_queries, nq, k, d_filter_of_query, nullptr, d_out_labels64, d_out_dists, d_out_counts, (hipStream_t)stream, true);
  });
}
hs_status hs_index_exact_screen_stats(hs_index *ix, uint64_t *screened, uint64_t *fell_back, uint64_t *reranked_rows) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  return guarded([&] {
    uint32_t st[kXsStateWords] = {};
    if (ix->xs_last) {
      HIP_TRY(hipSetDevice(ix->device));
      HIP_TRY(hipMemcpy(st, ix->xs_last->xs_state.p, sizeof(st), hipMemcpyDeviceToHost));
    }
    if (screened) *screened = ix->xs_last ? ix->xs_last_nq - st[1] : 0;
    if (fell_back) *fell_back = st[1];
    if (reranked_rows) *reranked_rows = (uint64_t)st[2] | ((uint64_t)st[3] << 32);
    return HS_OK;
  });
}
hs_status hs_debug_exact_screen_margin(int metric, size_t dim, float qnorm2, float xnorm2, float *out) {
  if (!out) return fail(HS_ERR_INVALID, "null argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0 || dim > 4096) return fail(HS_ERR_INVALID, "dim: 1 to 4096");
  *out = exact_screen_margin(metric == HS_METRIC_IP, (uint32_t)dim, qnorm2, xnorm2);
  return HS_OK;
}

// ---- the same answers for byte queries, screened on the integer matrix cores (exact_screen_q8.hip) -----------------------------
hs_status hs_index_exact_search_q8(hs_index *ix, const hs_filter_set *fs, const void *queries, int query_format, size_t nq, size_t k,
                                   const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts) {
  if (query_format == HS_ROWS_F32) return fail(HS_ERR_INVALID, kQ8QueryFormatRefusal);   // (exact_host reads it as "fp32 queries")
  return exact_host(ix, fs, queries, query_format, nq, k, filter_of_query, out_labels64, out_dists, out_counts, true);
}
hs_status hs_index_exact_search_q8_dev(hs_index *ix, const hs_filter_set *fs, const void *d_queries, int query_format, size_t nq, size_t k,
                                       const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                       uint32_t *d_out_counts, void *stream) {
  return guarded([&] {
    hs_status s = exact_use_ok(ix, fs, d_queries, d_filter_of_query, nq, k, d_out_labels64, d_out_dists);
    if (s == HS_OK) s = exact_q8_use_ok(ix, query_format);
    if (s != HS_OK || nq == 0) return s;
    return exact_q8_dev(ix, fs, d_queries, query_format, nq, k, d_filter_of_query, nullptr, d_out_labels64, d_out_dists, d_out_counts, (hipStream_t)stream);
  });
}
hs_status hs_debug_exact_screen_q8_interval(int metric, size_t dim, int32_t value, uint32_t qnorm2, uint32_t xnorm2, float *out_a, float *out_e) {
  if (!out_a || !out_e) return fail(HS_ERR_INVALID, "null argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0 || dim > 4096) return fail(HS_ERR_INVALID, "dim: 1 to 4096");
  *out_e = exact_screen_q8_interval(metric == HS_METRIC_IP, (uint32_t)dim, value, qnorm2, xnorm2, out_a);
  return HS_OK;
}
hs_status hs_debug_exact_q8_pack_order(size_t dim, uint32_t *out) {
  if (!out) return fail(HS_ERR_INVALID, "null argument");
  if (dim == 0 || dim > 4096 || (dim & 15)) return fail(HS_ERR_INVALID, "dim: a multiple of 16, at most 4096");
  for (size_t p = 0; p < dim; p++) out[p] = narrow_elem((uint32_t)p, (uint32_t)dim);
  return HS_OK;
}

// ---- the same answers for fp16 queries, screened on the half-precision matrix cores (exact_screen_f16q.hip) -------------------
hs_status hs_index_exact_search_f16(hs_index *ix, const hs_filter_set *fs, const void *queries, size_t nq, size_t k,
                                    const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts) {
  return exact_host(ix, fs, queries, kQueriesF16, nq, k, filter_of_query, out_labels64, out_dists, out_counts, true);
}
hs_status hs_index_exact_search_f16_dev(hs_index *ix, const hs_filter_set *fs, const void *d_queries, size_t nq, size_t k,
                                        const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                        uint32_t *d_out_counts, void *stream) {
  return guarded([&] {
    hs_status s = exact_use_ok(ix, fs, d_queries, d_filter_of_query, nq, k, d_out_labels64, d_out_dists);
    if (s == HS_OK) s = exact_f16q_use_ok(ix);
    if (s != HS_OK || nq == 0) return s;
    return exact_f16q_dev(ix, fs, d_queries, nq, k, d_filter_of_query, nullptr, d_out_labels64, d_out_dists, d_out_counts, (hipStream_t)stream);
  });
}
// ---- and for bf16 queries over bf16 rows, on the bf16 matrix cores (exact_screen_bf16q.hip) ------------------------------------
hs_status hs_index_exact_search_bf16(hs_index *ix, const hs_filter_set *fs, const void *queries, size_t nq, size_t k,
                                     const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts) {
  return exact_host(ix, fs, queries, kQueriesBF16, nq, k, filter_of_query, out_labels64, out_dists, out_counts, true);
}
hs_status hs_index_exact_search_bf16_dev(hs_index *ix, const hs_filter_set *fs, const void *d_queries, size_t nq, size_t k,
                                         const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                         uint32_t *d_out_counts, void *stream) {
  return guarded([&] {
    hs_status s = exact_use_ok(ix, fs, d_queries, d_filter_of_query, nq, k, d_out_labels64, d_out_dists);
    if (s == HS_OK) s = exact_f16q_use_ok(ix, kQueriesBF16);
    if (s != HS_OK || nq == 0) return s;
    return exact_f16q_dev(ix, fs, d_queries, nq, k, d_filter_of_query, nullptr, d_out_labels64, d_out_dists, d_out_counts, (hipStream_t)stream, kQueriesBF16);
  });
}
// ---- and for fp8 (E4M3) queries over fp8 rows, on the fp8 matrix cores (exact_screen_f8q.hip) --------------------------------------
hs_status hs_index_exact_search_f8(hs_index *ix, const hs_filter_set *fs, const void *queries, size_t nq, size_t k,
                                   const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts) {
  return exact_host(ix, fs, queries, kQueriesF8, nq, k, filter_of_query, out_labels64, out_dists, out_counts, true);
}
hs_status hs_index_exact_search_f8_dev(hs_index *ix, const hs_filter_set *fs, const void *d_queries, size_t nq, size_t k,
                                       const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                       uint32_t *d_out_counts, void *stream) {
  return guarded([&] {
    hs_status s = exact_use_ok(ix, fs, d_queries, d_filter_of_query, nq, k, d_out_labels64, d_out_dists);
    if (s == HS_OK) s = exact_f16q_use_ok(ix, kQueriesF8);
    if (s != HS_OK || nq == 0) return s;
    return exact_f16q_dev(ix, fs, d_queries, nq, k, d_filter_of_query, nullptr, d_out_labels64, d_out_dists, d_out_counts, (hipStream_t)stream, kQueriesF8);
  });
}
hs_status hs_debug_exact_screen_f16_margin(int metric, size_t dim, float qnorm2, float xnorm2, uint32_t q_subnormals, uint32_t x_subnormals, float *out) {
  if (!out) return fail(HS_ERR_INVALID, "null argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0 || dim > 4096) return fail(HS_ERR_INVALID, "dim: 1 to 4096");
  *out = exact_screen_f16_margin(metric == HS_METRIC_IP, (uint32_t)dim, qnorm2, xnorm2, q_subnormals, x_subnormals);
  return HS_OK;
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
