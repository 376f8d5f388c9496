// exact_range_engine.hpp -- launch interface of the exact range search over the rows of a resident index (exact_range.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine.hpp"

namespace hs {

static constexpr uint32_t kRangeGridTarget = 2048;   // workgroups a launch aims at: eight per CU of a 256-CU part
static constexpr uint32_t kRangeMaxChunks = 64;      // row chunks per query at most
static constexpr uint32_t kRangeMinChunkRows = 1024;
static constexpr uint32_t kRangeSortLds = 2048;      // entries of a segment the sort holds in LDS: 24 KB, six workgroups per CU

// One call: nq queries against the rows the index holds; query i keeps the candidates with dist <= radius[i].
struct RangeArgs {
  const float *queries;     // nq x dim (device)
  const float *radius;      // nq
  uint32_t nq;
  const uint32_t *order;    // nullable: a permutation of [0, nq) -- tile slot s serves query order[s]; outputs stay at the query's own position
  const uint32_t *live;     // nullable (device): with `order`, only its first *live slots name queries (0xFFFFFFFF behind them) and only
                            // those queries' counts and results are written; tiles beyond them return at once.  Null: every tile runs
  uint32_t chunks, rows_per_chunk;   // xr_plan
  uint32_t *counts;         // nq x chunks: hits of (query, chunk)
  uint64_t *bases;          // nq x chunks: where the hits of (query, chunk) start in the outputs
  uint64_t *out_offsets;    // nq + 1
  uint64_t cap;             // entries out_labels / out_dists hold
  uint64_t *out_labels;
  float *out_dists;
  uint32_t *over;           // raised when out_offsets[nq] > cap
};

// Dynamic LDS of a scan workgroup: the tile's queries as fp32, and per slot its segment base and end (two u64), its radius, its
// query, its filter row and its counter.
inline size_t xr_lds_bytes(uint32_t dim) { return (((size_t)8 * dim * 4 + 15) & ~(size_t)15) + 8 * 32; }
// Launch plan of nq queries over n rows: *chunks row chunks of *rows_per_chunk rows (a multiple of 256).  Chunks exist only to fill
// the machine when there are few tiles: tiles * chunks <= kRangeGridTarget unless one chunk already exceeds it.
inline void xr_plan(uint32_t n, uint32_t nq, uint32_t *chunks, uint32_t *rows_per_chunk) {
  const uint32_t tiles = (nq + 7) / 8;
  uint32_t c = tiles == 0 || tiles >= kRangeGridTarget ? 1 : kRangeGridTarget / tiles;
  if (c > kRangeMaxChunks) c = kRangeMaxChunks;
  const uint32_t by_rows = (n + kRangeMinChunkRows - 1) / kRangeMinChunkRows;
  if (c > by_rows) c = by_rows;
  if (c < 1) c = 1;
  uint32_t rpc = (uint32_t)((((uint64_t)n + c - 1) / c + 255) / 256 * 256);
  if (rpc == 0) rpc = 256;
  *chunks = n ? (uint32_t)(((uint64_t)n + rpc - 1) / rpc) : 1;
  *rows_per_chunk = rpc;
}

// Candidates, rows / fmt and the filter's bad counter are launch_exact_search's (exact_engine.hpp).  Nothing synchronises.
// The count pass and the exclusive scan: a.counts, a.bases and a.out_offsets are written in full, whatever a.cap is.  a.nq == 0
// writes out_offsets[0] = 0.
hipError_t launch_exact_range_count(const DevIndex &ix, const void *rows, int fmt, const RangeArgs &a, const FilterArgs *f, hipStream_t stream);
// The fill pass and the segment sort, after launch_exact_range_count on the same stream: results of query i at
// [out_offsets[i], out_offsets[i + 1]) of a.out_labels / a.out_dists, ascending by (dist, label).  Both kernels read
// out_offsets[nq] on the device: above a.cap they write nothing but *a.over.
hipError_t launch_exact_range_fill(const DevIndex &ix, const void *rows, int fmt, const RangeArgs &a, const FilterArgs *f, hipStream_t stream);
// hs_last_kernel's name for the scan of an index of this dim and row format
const char *xr_kernel_name(uint32_t dim, int fmt);

}  // namespace hs
