// exact_wide_engine.hpp -- launch interface of the exact k-NN scan for 64 < k <= 1024 (exact_wide.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine.hpp"
#include "exact_engine.hpp"

namespace hs {

static constexpr uint32_t kWideMaxK = 1024;      // the largest result set any kernel of this project returns
static constexpr uint32_t kWideBuf = 256;        // B: entries of a query's unsorted append buffer
static constexpr uint32_t kWideGridTarget = 512; // workgroups a launch aims at: two per CU of a 256-CU part
static constexpr uint32_t kWideMaxChunks = 64;   // row chunks per query at most
static constexpr uint32_t kWideMinChunkRows = 1024;

// The kept list of a query has KP = max(128, k rounded up to a power of two) entries.
inline uint32_t xw_kp(uint32_t k) {
  uint32_t kp = 128;
  while (kp < k) kp <<= 1;
  return kp;
}
// Dynamic LDS of a scan workgroup with a tile of qt queries: the queries as fp32, per query KP kept + B buffered entries of 16
// bytes, and four words (buffer fill, threshold, the slot's query, its filter row).
//     k          KP    list bytes / query   tile   LDS at dim 128   workgroups per CU (160 KB)
//     65 .. 128   128        6 KB             8        52 KB              3
//    129 .. 256   256        8 KB             8        68 KB              2
//    257 .. 512   512       12 KB             4        50 KB              3
//    513 .. 1024 1024       20 KB             2        41 KB              3
inline size_t xw_lds_bytes(uint32_t dim, uint32_t k, uint32_t qt) {
  return (((size_t)qt * dim * 4 + 15) & ~(size_t)15) + (size_t)qt * (xw_kp(k) + kWideBuf) * 16 + (size_t)qt * 16;
}
// Tile width for (dim, k): the widest of 8 / 4 / 2 queries that leaves room for two workgroups per CU (80 KB each); where none does
// (large dim), the widest that fits the CU at all; 0 when not even two queries fit.
inline uint32_t xw_tile(uint32_t dim, uint32_t k) {
  for (uint32_t qt = 8; qt >= 2; qt >>= 1)
    if (xw_lds_bytes(dim, k, qt) <= 80 * 1024) return qt;
  for (uint32_t qt = 8; qt >= 2; qt >>= 1)
    if (xw_lds_bytes(dim, k, qt) <= 160 * 1024) return qt;
  return 0;
}
// Launch plan of nq queries over n rows: *chunks row chunks of *rows_per_chunk rows (a multiple of 256).  Chunks exist only to fill
// the machine when there are few tiles: chunks = kWideGridTarget / tiles rounded down, so tiles * chunks <= kWideGridTarget; one
// chunk from kWideGridTarget / 2 + 1 tiles on, and then the scan writes the outputs itself.  Returns the bytes of the partial-run
// workspace, nq * chunks * k * 16 (0 for one chunk).  nq <= qt * tiles and qt <= 8, so with several chunks that is at most
// 8 * tiles * chunks * k * 16 <= 8 * kWideGridTarget * k * 16 = 64 KiB * k (64 MiB at k = 1024; a quarter of that there, as the tile
// is 2), whatever nq is.
inline size_t xw_plan(uint32_t n, uint32_t nq, uint32_t k, uint32_t qt, uint32_t *chunks, uint32_t *rows_per_chunk) {
  const uint32_t tiles = (nq + qt - 1) / qt;
  uint32_t c = tiles == 0 || tiles >= kWideGridTarget ? 1 : kWideGridTarget / tiles;   // (rounded down: the bound above)
  if (c > kWideMaxChunks) c = kWideMaxChunks;
  const uint32_t by_rows = (n + kWideMinChunkRows - 1) / kWideMinChunkRows;
  if (c > by_rows) c = by_rows;
  if (c < 1) c = 1;
  uint32_t rpc = (uint32_t)((((uint64_t)n + c - 1) / c + 255) / 256 * 256);
  if (rpc == 0) rpc = 256;
  c = n ? (uint32_t)(((uint64_t)n + rpc - 1) / rpc) : 1;
  *chunks = c;
  *rows_per_chunk = rpc;
  return c > 1 ? (size_t)nq * c * k * 16 : 0;
}

// exact_engine.hpp's call with 64 < a.k <= kWideMaxK: a.grid_x = chunks and a.rows_per_block = rows per chunk as xw_plan gives them,
// a.partial of xw_plan's bytes.  Candidates, order, outputs and the filter's bad counter are launch_exact_search's.  Nothing
// synchronises.
hipError_t launch_exact_wide(const DevIndex &ix, const void *rows, int fmt, const ExactArgs &a, const FilterArgs *f, hipStream_t stream);
// hs_last_kernel's name for the scan of an index of this dim and row format
const char *xw_kernel_name(uint32_t dim, int fmt);

}  // namespace hs
