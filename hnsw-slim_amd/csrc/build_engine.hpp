// build_engine.hpp -- interface between capi_build.cpp (hs_build_hnsw_batched), capi_update.cpp (hs_index_add_points_batched) and build_gpu.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "host_batch_build.hpp"

namespace hs {

static constexpr uint32_t kBgMaxM = 31;          // maxM0 + 1 candidates of a full level-0 list fit one wavefront
static constexpr uint32_t kRqMaxM = 32;          // rabitqlib's builder: maxM0 + 1 = 65 candidates, two per lane
static constexpr uint32_t kBgMaxEfc = 512;
static constexpr uint32_t kBgScratchIds = 4096;  // default on-chip share of one row: visited ids (candidates: half of it)

struct GpuBuildInput {
  const float *base = nullptr;   // n x dim (host)
  uint32_t n = 0, dim = 0;
  int metric = 0;
  uint32_t M = 0, maxM = 0, maxM0 = 0, efc = 0;   // as VanillaGraph::init leaves them
  const int *levels = nullptr;                    // n
  const std::vector<BatchStep> *steps = nullptr;
  uint32_t scratch_ids = 0;                       // 0: kBgScratchIds; else a power of two >= 64
  bool rq = false;                                // rabitqlib's builder: RqGraph's rules, labels are the row index
};

// Whether the device path serves the shape (otherwise the host twin builds it): M, ef_construction, and the on-chip memory of a row.
bool gpu_build_supported(uint32_t dim, uint32_t M, uint32_t efc, uint32_t scratch_ids);

// The same for rabitqlib's builder (GpuBuildInput::rq): M from 2 to 32.
bool gpu_rq_build_supported(uint32_t dim, uint32_t M, uint32_t efc, uint32_t scratch_ids);
// rabitq_raw_dist (rq_dist.hpp) as the kernels of that builder compute it: out[i] = the distance of rows a[i] and b[i] (host arrays).
hipError_t gpu_rq_raw_dist(const float *a, const float *b, size_t n_pairs, uint32_t dim, int metric, int device, float *out);

// Batched addPoint on `device`.  Out: the level-0 lists (n x (maxM0 + 1) words, hnswlib's [u16 count][u16][ids] form), the upper
// lists ((maxM + 1) words each, node i's level l at slot upb[i] + l - 1), upb (n + 1 prefix sums of the levels), the rows that
// were searched again with their scratch in device memory, the device time from the first kernel to the last.
hipError_t gpu_batch_build(const GpuBuildInput &in, int device, std::vector<uint32_t> &lists0, std::vector<uint32_t> &lists_up,
                           std::vector<uint32_t> &upb, uint64_t &flagged_rows, double *kernel_ms);

// Batched addPoint continued on a resident index: n0 nodes are in the graph, `count` rows follow.
struct GpuAddInput {
  float *d_vec = nullptr;          // the index's resident fp32 rows on `device`: stride dim, room for n0 + count rows
  const float *rows = nullptr;     // count x dim (host); copied to d_vec + n0 * dim before anything else
  uint32_t n0 = 0, count = 0, dim = 0;
  int metric = 0;
  uint32_t M = 0, maxM = 0, maxM0 = 0, efc = 0;   // the file header's
  const uint32_t *lev = nullptr;                  // n0 + count levels
  const std::vector<BatchStep> *steps = nullptr;  // batch_schedule_from
  uint32_t scratch_ids = 0;
  // build_form_lists of the host image: n0 + count + 1 prefix sums, the seeded level-0 and upper slots
  const std::vector<uint32_t> *upb = nullptr, *lists0 = nullptr, *lists_up = nullptr;
};
// What came back: the tasks of the old nodes (< n0) that received an id, ascending -- task t < n is the level-0 list of node t,
// task n + j the upper slot j (n = n0 + count) -- and `slots`: (maxM0 + 1) words per entry, first one per changed task in that
// order, then the level-0 slots of the new nodes, then their upper slots (each upper slot in the first maxM + 1 words of its entry).
struct GpuAddOutput {
  std::vector<uint32_t> tasks, slots;
  uint64_t flagged_rows = 0;
  double kernel_ms = 0.0;
};
hipError_t gpu_batch_add(const GpuAddInput &in, int device, GpuAddOutput &out);

}  // namespace hs
