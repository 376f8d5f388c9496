// segment_copy.hpp -- launchers of the two copy kernels of a search queue (segment_copy.hip): rows of many submissions into one
// contiguous query array, and each row's results back to its own submission's buffers.  The segment table is search_queue.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include "search_queue.hpp"

namespace hs {

// Segments up to this many have their row prefix searched in LDS, more in global memory (a launch rarely coalesces more).
constexpr uint32_t kSegLds = 256;

// The launch's arrays in device memory: what the search reads (q, foq) and writes (the rest); null = not part of this launch.
struct LaunchArrays {
  float *q;          // total x dim
  uint32_t *foq;     // total
  uint32_t *l32;     // total x k
  uint64_t *l64;     // total x k
  float *dd;         // total x k
  uint32_t *cnt;     // total
  uint32_t *stats;   // total x 4
};

// first_row: n_seg + 1 words, entries: n_seg records; both device-visible (page-locked host memory as the device addresses it).
hipError_t launch_gather_rows(const uint32_t *first_row, const SegEntry *entries, uint32_t n_seg, uint32_t total, uint32_t dim,
                              float *q, uint32_t *foq, hipStream_t stream);
hipError_t launch_scatter_results(const uint32_t *first_row, const SegEntry *entries, uint32_t n_seg, uint32_t total, uint32_t k,
                                  const LaunchArrays &a, hipStream_t stream);

}  // namespace hs
