// slimq_chain.hpp -- what the in-memory SlimQ chain (capi_slimq_resident.cpp) shares with the file-based entries it is made of: the
// graph handle, the batched rabitqlib build into a graph object (capi_build.cpp) and the two conversion steps on in-memory objects
// (capi_convert_slimq.cpp).  Read by the .cpp files only.
#pragma once
#include "capi_internal.hpp"
#include "host_rq_graph.hpp"

// An HNSW graph in host memory: what saveIndex (hnswalg.h:748-779) would write.
struct hs_graph {
  hs::RqGraph g;
};

#pragma GCC visibility push(hidden)
// capi_build.cpp: hs_build_rabitq_hnsw_batched without its file -- the refusals, then the build into `g` (stats without total_ms)
hs_status rq_batched_args_ok(const float *base, size_t n, size_t dim, int metric, size_t M, const hs_batch_build_opts *opts);
hs_status rq_batched_build_into(RqGraph &g, const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction, size_t seed,
                                const hs_batch_build_opts *opts, hs_batch_build_stats &st);
// capi_convert_slimq.cpp
hs_status slimq_records_args_ok(int metric, size_t dim, const float *centroids, size_t num_cluster);
hs_status slimq_device_ok(int device);
// Slim's graph passes into `s`: on `device`, or on the host when the shape is outside the device path.
hs_status slim_graph_step(SlimGraph &s, const VanillaGraph &g, const SlimParams &p, int device, int threads, int *used_gpu, double *kernel_ms);
// SlimQ's graph passes into `s`: on `device`, or on the host when device < 0 or the shape is outside the device path.
hs_status slimq_graph_step(SlimGraph &s, const VanillaGraph &g, const SlimParams &p, int device, int threads, int *used_gpu, double *kernel_ms);
// The records of `s` into `q` (SlimQGraph::from_slim): on `device`, or on the host when device < 0.
hs_status slimq_records_step(SlimQGraph &q, const SlimGraph &s, int metric, const float *centroids, size_t num_cluster, const uint32_t *cluster_ids,
                             uint64_t flip_seed, int device, int threads, int *used_gpu, double *kernel_ms);
#pragma GCC visibility pop
