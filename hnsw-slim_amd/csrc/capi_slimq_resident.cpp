// capi_slimq_resident.cpp -- the C ABI (include/hnsw_slim_amd.h): a resident HNSW-SlimQ index from rows or a graph with no file on the
// way -- the in-memory graph handle, convertFromHNSW of it into a file and / or a resident index, the whole chain from rows, saveIndex
// of a resident index's host image, and the debug views of its three record arrays beside their host statement (slimq_tiles.hpp).
#include "slimq_chain.hpp"
#include "slimq_tiles.hpp"

namespace {

// what hs_graph_convert_slimq is refused for, before any work
hs_status convert_args_ok(const hs_graph *g, const hs_slimq_params *p, int convert_device, const char *out_path, int index_device, hs_index **out_index) {
  if (!g || !p) return fail(HS_ERR_INVALID, "bad argument");
  if (!out_path && !out_index) return fail(HS_ERR_INVALID, "hs_graph_convert_slimq: a file, an index or both -- neither was asked for");
  hs_status st = slimq_records_args_ok((int)g->g.metric, g->g.dim, p->centroids, p->num_cluster);
  if (st != HS_OK) return st;
  if (convert_device < -1) return fail(HS_ERR_INVALID, "device: -1 (the host path) or a HIP device");
  if (convert_device >= 0 && (st = slimq_device_ok(convert_device)) != HS_OK) return st;
  if (out_index) {
    if (index_device < 0) return fail(HS_ERR_INVALID, "index_device: a HIP device");
    if (device_ok(index_device, true) != HS_OK) return HS_ERR_DEVICE;
  }
  return HS_OK;
}

// The chain on in-memory objects: graph passes, records, then the file and / or the resident index.  resident_ms (nullable): packing,
// uploads, tile kernels and the dataset upload.  rows (nullable): the graph's rows as one contiguous array, where the caller has one.
// (Throws what the converters throw: the two entries that call it guard.)
hs_status convert_graph(const RqGraph &g, const hs_slimq_params *p, int convert_device, int threads, const char *out_path, int index_device,
                        int with_dataset, const float *rows, hs_index **out_index, hs_slimq_convert_stats *stats, double *resident_ms,
                        double *tile_kernel_ms) {
  const auto t0 = std::chrono::steady_clock::now();
  hs_slimq_convert_stats out{};
  const int metric = (int)g.metric;
  std::unique_ptr<SlimQGraph> q(new SlimQGraph());
  {
    SlimGraph s;
    hs_status st = slimq_graph_step(s, g, slim_params(p->threshold_level, p->top_degree_percent0, p->top_degree_percent, p->top_degree_M0, p->low_degree_m0,
                                                      p->top_degree_M, p->low_degree_m),
                                    convert_device, threads, &out.graph_used_gpu, &out.graph_kernel_ms);
    if (st != HS_OK) return st;
    out.graph_ms = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    st = slimq_records_step(*q, s, metric, p->centroids, p->num_cluster, p->cluster_ids, p->flip_seed, convert_device, threads, &out.records_used_gpu,
                            &out.records_kernel_ms);
    if (st != HS_OK) return st;
    out.records_ms = ms_since(t1);
    if (out_path) q->save(out_path);
  }
  if (out_index) {
    const auto t2 = std::chrono::steady_clock::now();
    hs_index *ix = nullptr;
    hs_status st = slimq_make_resident(std::move(q), index_device, &ix);
    if (st != HS_OK) return st;
    if (with_dataset && g.count) {
      st = rows ? slimq_set_dataset_pitched(ix, rows, g.dim * sizeof(float), g.count, g.dim)
                : slimq_set_dataset_pitched(ix, g.vec(0), g.size_per_el, g.count, g.dim);
      if (st != HS_OK) { hs_index_free(ix); return st; }
    }
    if (resident_ms) *resident_ms = ms_since(t2);
    if (tile_kernel_ms) *tile_kernel_ms = ix->tile_kernel_ms;
    *out_index = ix;
  }
  out.total_ms = ms_since(t0);
  if (stats) *stats = out;
  return HS_OK;
}

}  // namespace

hs_status hs_build_rabitq_hnsw_batched_mem(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction, size_t seed,
                                           const hs_batch_build_opts *opts, hs_graph **out, hs_batch_build_stats *stats) {
  if (!out) return fail(HS_ERR_INVALID, "bad argument");
  hs_status s = rq_batched_args_ok(base, n, dim, metric, M, opts);
  if (s != HS_OK) return s;
  return guarded([&] {
    const auto t0 = std::chrono::steady_clock::now();
    hs_batch_build_stats st{};
    std::unique_ptr<hs_graph> g(new hs_graph());
    s = rq_batched_build_into(g->g, base, n, dim, metric, M, ef_construction, seed, opts, st);
    if (s != HS_OK) return s;
    st.total_ms = ms_since(t0);
    if (stats) *stats = st;
    *out = g.release();
    return HS_OK;
  });
}

hs_status hs_graph_load(const char *path, int metric, size_t dim, hs_graph **out) {
  if (!path || !out) return fail(HS_ERR_INVALID, "bad argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  return guarded([&] {
    std::unique_ptr<hs_graph> g(new hs_graph());
    g->g.load(path, (Metric)metric, dim);
    *out = g.release();
    return HS_OK;
  });
}

hs_status hs_graph_save(const hs_graph *g, const char *path) {
  if (!g || !path) return fail(HS_ERR_INVALID, "bad argument");
  return guarded([&] {
    g->g.save(path);
    return HS_OK;
  });
}

hs_status hs_graph_info(const hs_graph *g, uint64_t *n, uint64_t *dim, int *metric, uint64_t *M, uint64_t *ef_construction, int *maxlevel) {
  if (!g) return fail(HS_ERR_INVALID, "bad argument");
  if (n) *n = g->g.count;
  if (dim) *dim = g->g.dim;
  if (metric) *metric = (int)g->g.metric;
  if (M) *M = g->g.M;
  if (ef_construction) *ef_construction = g->g.efC;
  if (maxlevel) *maxlevel = g->g.maxlevel;
  return HS_OK;
}

void hs_graph_free(hs_graph *g) { delete g; }

hs_status hs_graph_convert_slimq(const hs_graph *g, const hs_slimq_params *p, int convert_device, int threads, const char *out_path,
                                 int index_device, int with_dataset, hs_index **out_index, hs_slimq_convert_stats *stats) {
  const hs_status st = convert_args_ok(g, p, convert_device, out_path, index_device, out_index);
  if (st != HS_OK) return st;
  return guarded([&] { return convert_graph(g->g, p, convert_device, threads, out_path, index_device, with_dataset, nullptr, out_index, stats, nullptr, nullptr); });
}

hs_status hs_slimq_index_from_rows(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction, size_t seed,
                                   const hs_batch_build_opts *opts, const hs_slimq_params *p, int threads, int with_dataset,
                                   hs_index **out_index, hs_slimq_pipeline_stats *stats) {
  if (!out_index || !p) return fail(HS_ERR_INVALID, "bad argument");
  hs_status s = rq_batched_args_ok(base, n, dim, metric, M, opts);
  if (s != HS_OK) return s;
  if (opts->device < 0) return fail(HS_ERR_INVALID, "hs_slimq_index_from_rows: opts->device is the HIP device the index will live on");
  if ((s = slimq_records_args_ok(metric, dim, p->centroids, p->num_cluster)) != HS_OK) return s;
  return guarded([&] {
    const auto t0 = std::chrono::steady_clock::now();
    hs_slimq_pipeline_stats out{};
    std::unique_ptr<hs_graph> g(new hs_graph());
    s = rq_batched_build_into(g->g, base, n, dim, metric, M, ef_construction, seed, opts, out.build);
    if (s != HS_OK) return s;
    out.build.total_ms = ms_since(t0);
    // (labels are row indexes and internal ids in this graph: `base` is the dataset by internal id)
    s = convert_graph(g->g, p, opts->device, threads, nullptr, opts->device, with_dataset, base, out_index, &out.convert, &out.resident_ms, &out.tile_kernel_ms);
    if (s != HS_OK) return s;
    out.total_ms = ms_since(t0);
    if (stats) *stats = out;
    return HS_OK;
  });
}

hs_status hs_slimq_index_save(const hs_index *ix, const char *path) {
  if (!ix || !path) return fail(HS_ERR_INVALID, "null argument");
  if (!ix->host_slimq) return fail(HS_ERR_INVALID, "not a SlimQ index");
  return guarded([&] {
    ix->host_slimq->save(path);
    return HS_OK;
  });
}

// hands `v` (or its length alone) to a debug caller
static hs_status give_words(const uint32_t *host, const uint32_t *dev, size_t len, uint32_t *out, size_t cap_words, size_t *words) {
  if (words) *words = len;
  if (!out || len == 0) return HS_OK;
  if (cap_words < len) return fail(HS_ERR_CAPACITY, "hs_debug_slimq_arrays: the array holds " + std::to_string(len) + " words");
  if (host) memcpy(out, host, len * 4);
  else HIP_TRY(hipMemcpy(out, dev, len * 4, hipMemcpyDeviceToHost));
  return HS_OK;
}

hs_status hs_debug_slimq_arrays(const hs_index *ix, int which, uint32_t *out, size_t cap_words, size_t *words, uint32_t *stride, uint32_t *row_words) {
  if (!ix || which < 0 || which > 2) return fail(HS_ERR_INVALID, "bad argument");
  if (ix->info.kind != HS_KIND_SLIMQ) return fail(HS_ERR_INVALID, "not a SlimQ index");
  const DevSlimQ &d = ix->sq;
  const size_t n = ix->info.n;
  const uint32_t *src = nullptr;
  size_t len = 0;
  uint32_t st = 0, rw = 0;
  if (which == 0) { src = d.rec; len = n * d.rec_words; st = 1; rw = d.rec_words; }
  if (which == 1 && d.ftile) { src = d.ftile; st = ix->dev.tile_stride; rw = d.rec_words; len = n * st * rw; }
  if (which == 2 && d.uptile) { src = d.uptile; st = d.up_stride; rw = d.rec_words + 4; len = ix->up_ptr.n * (size_t)st * rw; }
  if (stride) *stride = st;
  if (row_words) *row_words = rw;
  return guarded([&] {
    if (len) HIP_TRY(hipSetDevice(ix->device));
    return give_words(nullptr, src, len, out, cap_words, words);
  });
}

hs_status hs_debug_slimq_arrays_host(const char *slimq_path, int metric, size_t dim, int fused, int which, uint32_t *out, size_t cap_words,
                                     size_t *words, uint32_t *stride, uint32_t *row_words) {
  if (!slimq_path || which < 0 || which > 2) return fail(HS_ERR_INVALID, "bad argument");
  return guarded([&] {
    SlimQGraph q;
    q.load(BinSource(slimq_path), metric, dim);
    if (q.rot.trunc < 64) return fail(HS_ERR_UNSUPPORTED, "SlimQ supports dim >= 64");
    PackedIndex p;
    p.n = q.count; p.dim = dim;
    p.pack_chal([&](size_t i) { return (int)q.level[i]; }, [&](size_t i) { return (size_t)q.total(i); },
                [&](size_t i) -> const std::vector<char> & { return q.blobs[i]; });
    const uint32_t rw = slimq_rec_words(q.padded);
    const std::vector<uint32_t> rec = slimq_pack_records(q.factors.data(), q.cluster.data(), q.code.data(), q.count, q.padded);
    std::vector<uint32_t> arr;
    uint32_t st = 0, w = 0;
    if (which == 0) { st = 1; w = rw; }
    if (which == 1 && fused && (st = tile_stride_for(p.max_deg0)) != 0) {
      w = rw;
      arr = slimq_ftile_host(rec, rw, q.count, p.row_ptr0.data(), p.cols.data(), st);
    }
    if (which == 2 && fused && (st = slimq_up_stride(p.up_ptr)) != 0) {
      w = rw + 4;
      arr = slimq_uptile_host(rec, rw, q.count, q.level.data(), p.up_base, p.up_ptr, p.cols.data(), st);
    }
    if (stride) *stride = st;
    if (row_words) *row_words = w;
    return give_words(which == 0 ? rec.data() : arr.data(), nullptr, which == 0 ? rec.size() : arr.size(), out, cap_words, words);
  });
}
