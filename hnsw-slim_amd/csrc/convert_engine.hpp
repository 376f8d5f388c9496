// convert_engine.hpp -- interface between slim_convert_gpu.hpp (convert_gpu, convert_diff_gpu) and convert_gpu.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace hs {

// One task per (node, level) list of the vanilla graph: level-0 lists first (task v = node v), then the upper-level lists in
// node order (task n + upb[v] + l - 1 = level l of node v).
struct ConvertInput {
  const float *vec = nullptr;   // n x dim, row-major (host)
  uint32_t n = 0, dim = 0;
  int metric = 0;
  std::vector<uint32_t> t_node, t_level, t_off, t_size;   // per task: node, level, slice of `lists`
  std::vector<uint32_t> t_mlim;                           // degree budget of the first pruning (hnswalg_slim.h:957-961, 969-973)
  std::vector<uint32_t> t_limit;                          // capacity of the level (maxM0 / maxM, :1037)
  std::vector<uint32_t> lists;                            // concatenated source lists
  std::vector<uint32_t> upb;                              // n: index of the node's first upper-level task
  // slots per task of the pruned and final lists: 32 when every capacity (t_limit) and budget (t_mlim) of the call is at most 32,
  // 64 when one is above (none may exceed 64)
  uint32_t keep = 32;
};

// Phases 1-3 of convertFromHNSW on device `device`: fin[t * in.keep .. + fin_cnt[t]) = the final list of task t (after the reverse-edge
// union and the re-prune, before the hierarchical filter).  needs_host: some list exceeded the on-chip buffers -- the caller
// falls back to the CPU conversion.  kernel_ms (nullable): device time of the kernels.
hipError_t gpu_convert_lists(const ConvertInput &in, int device, std::vector<uint32_t> &fin, std::vector<uint32_t> &fin_cnt, bool &needs_host,
                             double *kernel_ms);

// The same three phases as HierarchicalNSWSlimQ::convertFromHNSW runs them (convert_slimq.hip): every distance rabitqlib's raw
// distance, the prune SlimQ's own PruneByHeuristic.  The caller has checked gpu_convert_slimq_fits(in.dim) -- the node's row and a
// union of kCvUnionCap ids fit the kernels' LDS -- and that no source list is longer than in.n.
bool gpu_convert_slimq_fits(uint32_t dim);
hipError_t gpu_convert_slimq_lists(const ConvertInput &in, int device, std::vector<uint32_t> &fin, std::vector<uint32_t> &fin_cnt, bool &needs_host,
                                   double *kernel_ms);

// The RaBitQ records of n rows (convert_slimq.hip): row r = rows + r * row_stride (floats; the rows of a Slim element array are read
// in place), zero-padded to padded = dim rounded up to 64 and rotated with the four flip rounds of `flips` (4 * padded / 8 bytes), its
// cluster = cluster_ids[r] or, without cluster_ids, the nearest raw centroid, then rq_quantize_data against the rotated centroid.
// Rows are uploaded kRqChunkBytes at a time.  64 <= dim < 4096, ncl >= 1, cluster ids below ncl: the caller's checks.
static constexpr size_t kRqChunkBytes = size_t(256) << 20;
struct RqQuantInput {
  const float *rows = nullptr;
  size_t row_stride = 0, n = 0, dim = 0;
  int metric = 0;
  const uint8_t *flips = nullptr;
  const float *cent_raw = nullptr;   // ncl x dim
  size_t ncl = 0;
  const uint32_t *cluster_ids = nullptr;
};
// out_cent_rot: ncl x padded; out_rot (nullable): n x padded; out_cluster: n; out_code: n x padded / 64; out_fac: n x 3 (all host).
// kernel_ms (nullable): device time of the kernels, summed over the chunks.
hipError_t gpu_rq_quantize(const RqQuantInput &in, int device, float *out_cent_rot, float *out_rot, uint32_t *out_cluster, uint64_t *out_code,
                           float *out_fac, double *kernel_ms);

// What the diff kernel of convert_diff.hip compares the new lists against and what it hands back.  In: the resident Slim
// index's own adjacency (level-0 tiles + upper-level CSR), labels and fp32 rows as they are BEFORE the call, the resident HNSW
// index's labels, the per-node levels of the HNSW index.  Out, each ascending (compacted on the device): the changed old nodes and
// the new nodes by the rules of hnswalg_slim.h:1360-1378 short of the label lookup (the caller applies it to the few nodes it can
// concern), the nodes whose image changed in any way, and those of them whose row or label differs; flags (one byte per node:
// bit 0 lists differ, bit 1 has neighbours, bit 2 row or label differs) only when want_flags.
struct DiffDev {
  const uint32_t *s_tile0 = nullptr, *s_up_base = nullptr, *s_up_ptr = nullptr, *s_cols = nullptr;
  const uint64_t *s_labels = nullptr, *h_labels = nullptr;
  const float *s_vec = nullptr;
  uint32_t s_stride = 0, prev_count = 0, n_up = 0;   // n_up: entries of s_up_ptr
  int32_t threshold_level = 0;
  std::vector<uint32_t> levels;   // n
  bool want_flags = false;
  std::vector<uint32_t> old_ids, new_ids, dirty, stale;
  std::vector<uint8_t> flags;
};

// The list passes of convertFromHNSWWithDiff (hnswalg_slim.h:1189-1303; convert_diff.hip) with the rows read from `d_vec`, n x dim
// fp32 already on `device` (in.vec is not read): both prunes are hnsw->getNeighborsByHeuristic2 (hnswalg.h:481-523) -- candidates by
// (distance ascending, id descending), lists below their budget untouched -- and a re-pruned list is the pop order of the heap
// the heuristic returns.  fin / fin_cnt / needs_host as gpu_convert_lists; n_reprune: the lists that were re-pruned.
// diff (nullable): then the per-node diff kernel and the compaction run on the final lists while they are still on the device.
// kernel_ms: from the first kernel to the last -- the list kernels and, with `diff`, the diff and compaction kernels -- which
// includes the two host round trips between them (the reverse-edge prefix sum; the upload of the levels and the scratch of the diff).
hipError_t gpu_convert_diff_lists(const ConvertInput &in, const float *d_vec, int device, std::vector<uint32_t> &fin, std::vector<uint32_t> &fin_cnt,
                                  bool &needs_host, uint32_t &n_reprune, double *kernel_ms, DiffDev *diff = nullptr);

}  // namespace hs
