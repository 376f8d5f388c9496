// capi_convert_slimq.cpp -- the C ABI (include/hnsw_slim_amd.h): HierarchicalNSWSlimQ::convertFromHNSW with its two steps on a
// device (convert_slimq.hip) -- the graph passes, the RaBitQ records -- each beside its host form, and the two chained in memory.
// (The file-to-file graph passes, hs_convert_slimq_graph_gpu, stand with the other three converters of that frame in capi_build.cpp.)
#include "capi_internal.hpp"

#include "host_rq_graph.hpp"
#include "rabitq_host.hpp"
#include "slim_convert_gpu.hpp"
#include "slimq_chain.hpp"

// (the functions from here to the first entry are shared with capi_build.cpp and capi_slimq_resident.cpp: slimq_chain.hpp)
// what every records entry is refused for before a file is read (the refusals of hs_convert_slimq)
hs_status slimq_records_args_ok(int metric, size_t dim, const float *centroids, size_t num_cluster) {
  if (!centroids || num_cluster == 0) return fail(HS_ERR_INVALID, "bad argument");
  if (dim < 64 || dim >= 4096) return fail(HS_ERR_UNSUPPORTED, "SlimQ supports 64 <= dim < 4096");
  if (num_cluster > 0xFFFFFFFFull) return fail(HS_ERR_INVALID, "too many clusters");
  return metric_ok(metric);
}
hs_status slimq_device_ok(int device) {
  if (device < 0) return fail(HS_ERR_INVALID, "device: a HIP device");
  return device_ok(device, false);
}

// The graph passes of a step into `s`: `on_device` ran them when it returns true; when it returns false without an error text the shape
// is outside the device path and `on_host` runs them.
template <class OnDevice, class OnHost>
static hs_status graph_step(bool try_device, OnDevice &&on_device, OnHost &&on_host, int *used_gpu, double *kernel_ms) {
  bool ok = false;
  double ms = 0.0;
  if (try_device) {
    std::string err;
    ok = on_device(&ms, &err);
    if (!ok && !err.empty()) return fail(HS_ERR_DEVICE, err);
  }
  if (!ok) on_host();
  if (used_gpu) *used_gpu = ok ? 1 : 0;
  if (kernel_ms) *kernel_ms = ok ? ms : 0.0;
  return HS_OK;
}
// Slim's graph passes: on `device`, or on the host when the shape is outside the device path.
hs_status slim_graph_step(SlimGraph &s, const VanillaGraph &g, const SlimParams &p, int device, int threads, int *used_gpu, double *kernel_ms) {
  return graph_step(true, [&](double *ms, std::string *err) { return convert_gpu(s, g, p, device, threads, ms, err); },
                    [&] { s.convert(g, p, threads); }, used_gpu, kernel_ms);
}
// SlimQ's graph passes: on `device`, or on the host when device < 0 or the shape is outside the device path.
hs_status slimq_graph_step(SlimGraph &s, const VanillaGraph &g, const SlimParams &p, int device, int threads, int *used_gpu, double *kernel_ms) {
  return graph_step(device >= 0, [&](double *ms, std::string *err) { return convert_slimq_gpu(s, g, p, device, threads, ms, err); },
                    [&] { convert_slimq_graph(s, g, p, threads); }, used_gpu, kernel_ms);
}
// The records of `s` into `q` (SlimQGraph::from_slim): on `device`, or on the host when device < 0.
hs_status slimq_records_step(SlimQGraph &q, const SlimGraph &s, int metric, const float *centroids, size_t num_cluster, const uint32_t *cluster_ids,
                       uint64_t flip_seed, int device, int threads, int *used_gpu, double *kernel_ms) {
  if (cluster_ids)
    for (size_t i = 0; i < s.count; i++)
      if (cluster_ids[i] >= num_cluster) return fail(HS_ERR_INVALID, "cluster id out of range");
  double ms = 0.0;
  if (device < 0) {
    q.from_slim(s, metric, centroids, num_cluster, cluster_ids, flip_seed, threads);
  } else {
    q.take_slim(s, metric, num_cluster, flip_seed);
    RqQuantInput in;
    in.rows = s.count ? s.vec(0) : nullptr; in.row_stride = s.size_per_el / 4; in.n = s.count; in.dim = s.dim; in.metric = metric;
    in.flips = q.rot.flip.data(); in.cent_raw = centroids; in.ncl = num_cluster; in.cluster_ids = cluster_ids;
    const hipError_t e = gpu_rq_quantize(in, device, q.centroids.data(), nullptr, q.cluster.data(), q.code.data(), q.factors.data(), &ms);
    if (e != hipSuccess) return fail(HS_ERR_DEVICE, std::string("GPU quantise: ") + hipGetErrorString(e));
  }
  if (used_gpu) *used_gpu = device >= 0 ? 1 : 0;
  if (kernel_ms) *kernel_ms = ms;
  return HS_OK;
}

hs_status hs_convert_slimq_gpu(const char *slim_path, int metric, size_t dim, const float *centroids, size_t num_cluster,
                               const uint32_t *cluster_ids, uint64_t flip_seed, int device, int threads, const char *out_path, int *used_gpu,
                               double *kernel_ms) {
  if (!slim_path || !out_path) return fail(HS_ERR_INVALID, "bad argument");
  hs_status st = slimq_records_args_ok(metric, dim, centroids, num_cluster);
  if (st == HS_OK) st = slimq_device_ok(device);
  if (st != HS_OK) return st;
  return guarded([&] {
    SlimGraph s;
    s.load(slim_path, (Metric)metric, dim);
    SlimQGraph q;
    const hs_status rs = slimq_records_step(q, s, metric, centroids, num_cluster, cluster_ids, flip_seed, device, threads, used_gpu, kernel_ms);
    if (rs != HS_OK) return rs;
    q.save(out_path);
    return HS_OK;
  });
}

hs_status hs_convert_hnsw_to_slimq(const char *hnsw_path, int metric, size_t dim, int threshold_level, float top_degree_percent0,
                                   float top_degree_percent, size_t top_degree_M0, size_t low_degree_m0, size_t top_degree_M,
                                   size_t low_degree_m, const float *centroids, size_t num_cluster, const uint32_t *cluster_ids,
                                   uint64_t flip_seed, int device, int threads, const char *out_path, hs_slimq_convert_stats *stats) {
  if (!hnsw_path || !out_path) return fail(HS_ERR_INVALID, "bad argument");
  hs_status st = slimq_records_args_ok(metric, dim, centroids, num_cluster);
  if (st != HS_OK) return st;
  if (device < -1) return fail(HS_ERR_INVALID, "device: -1 (the host path) or a HIP device");
  if (device >= 0 && (st = slimq_device_ok(device)) != HS_OK) return st;
  return guarded([&] {
    const auto t0 = std::chrono::steady_clock::now();
    hs_slimq_convert_stats out{};
    SlimGraph s;
    {
      VanillaGraph g;
      g.load(hnsw_path, (Metric)metric, dim);
      const hs_status gs = slimq_graph_step(s, g, slim_params(threshold_level, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0, top_degree_M, low_degree_m),
                                            device, threads, &out.graph_used_gpu, &out.graph_kernel_ms);
      if (gs != HS_OK) return gs;
    }
    out.graph_ms = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    SlimQGraph q;
    const hs_status rs = slimq_records_step(q, s, metric, centroids, num_cluster, cluster_ids, flip_seed, device, threads, &out.records_used_gpu, &out.records_kernel_ms);
    if (rs != HS_OK) return rs;
    out.records_ms = ms_since(t1);
    q.save(out_path);
    out.total_ms = ms_since(t0);
    if (stats) *stats = out;
    return HS_OK;
  });
}

hs_status hs_debug_rq_quantize_rows(size_t dim, int metric, const uint8_t *flips, const float *rows, size_t n, const float *centroids_raw,
                                    size_t num_cluster, const uint32_t *cluster_ids, int device, float *out_rotated, uint32_t *out_cluster,
                                    uint64_t *out_codes, float *out_factors) {
  if (!flips || !rows || !out_cluster || !out_codes || !out_factors) return fail(HS_ERR_INVALID, "bad argument");
  hs_status st = slimq_records_args_ok(metric, dim, centroids_raw, num_cluster);
  if (st != HS_OK) return st;
  if (device < -1) return fail(HS_ERR_INVALID, "device: -1 (the host recipe) or a HIP device");
  if (n > 0xFFFFFFFFull) return fail(HS_ERR_INVALID, "too many rows");
  if (cluster_ids)
    for (size_t i = 0; i < n; i++)
      if (cluster_ids[i] >= num_cluster) return fail(HS_ERR_INVALID, "cluster id out of range");
  if (device >= 0 && (st = slimq_device_ok(device)) != HS_OK) return st;
  return guarded([&] {
    Rotator rot;
    rot.init(dim);
    memcpy(rot.flip.data(), flips, rot.flip.size());
    std::vector<float> cent_rot(num_cluster * rot.padded);
    if (device < 0) {
      rq_quantize_rows_host(rot, metric, rows, dim, n, centroids_raw, num_cluster, cluster_ids, 1, cent_rot.data(), out_rotated, out_cluster, out_codes,
                            out_factors);
    } else {
      RqQuantInput in;
      in.rows = rows; in.row_stride = dim; in.n = n; in.dim = dim; in.metric = metric;
      in.flips = rot.flip.data(); in.cent_raw = centroids_raw; in.ncl = num_cluster; in.cluster_ids = cluster_ids;
      const hipError_t e = gpu_rq_quantize(in, device, cent_rot.data(), out_rotated, out_cluster, out_codes, out_factors, nullptr);
      if (e != hipSuccess) return fail(HS_ERR_DEVICE, std::string("GPU quantise: ") + hipGetErrorString(e));
    }
    return HS_OK;
  });
}
