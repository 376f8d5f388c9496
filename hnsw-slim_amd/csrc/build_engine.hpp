// build_engine.hpp -- interface between capi_build.cpp (hs_build_hnsw_batched) and build_gpu.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "host_batch_build.hpp"

namespace hs {

static constexpr uint32_t kBgMaxM = 31;          // maxM0 + 1 candidates of a full level-0 list fit one wavefront
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
};

// Whether the device path serves the shape (otherwise the host twin builds it): M, ef_construction, and the on-chip memory of a row.
bool gpu_build_supported(uint32_t dim, uint32_t M, uint32_t efc, uint32_t scratch_ids);

// Batched addPoint on `device`.  Out: the level-0 lists (n x (maxM0 + 1) words, hnswlib's [u16 count][u16][ids] form), the upper
// lists ((maxM + 1) words each, node i's level l at slot upb[i] + l - 1), upb (n + 1 prefix sums of the levels), the rows that
// were searched again with their scratch in device memory, the device time from the first kernel to the last.
hipError_t gpu_batch_build(const GpuBuildInput &in, int device, std::vector<uint32_t> &lists0, std::vector<uint32_t> &lists_up,
                           std::vector<uint32_t> &upb, uint64_t &flagged_rows, double *kernel_ms);

}  // namespace hs
