// exact_range_screen_engine.hpp -- launch interface of the screened exact range search (exact_range_screen.hip): the
// fp32 MFMA screen of exact_screen.hip against a fixed threshold, the caller's radius; a re-rank of the survivors in the recipe's
// arithmetic that keeps r <= radius and counts; and, for the queries the screen cannot decide, exact_range.hip's own two passes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hnsw_slim_amd.h"
#include "exact_range_engine.hpp"
#include "exact_screen_engine.hpp"

namespace hs {

static constexpr uint32_t kXrsList = HS_EXACT_RANGE_SCREEN_LIST;   // survivors a query's list holds; one more and the query falls back

// One call.  r: the range search's arguments -- queries, radii, `order` (the screen's tile slots, nullable), the count matrix, its scan
// and the outputs; r.chunks / r.rows_per_chunk (xr_plan) are the geometry of the fallback and the width of the count matrix.
struct RangeScreenArgs {
  RangeArgs r;
  float *xnorm2, *qnorm2;   // ix.n and r.nq words
  uint32_t grid_y, rows_per_block;   // xrs_plan: row chunks of the screen
  uint32_t *state;          // kXsStateWords (exact_screen_engine.hpp): [0] = [1] = flagged queries, [2..3] = listed rows re-ranked (u64)
  uint32_t *qflag;          // r.nq words: the query falls back
  uint32_t *fb_order;       // r.nq words: the flagged queries first, 0xFFFFFFFF behind them
  uint32_t *cursor;         // r.nq words: survivors of the query so far; it keeps counting past kXrsList
  uint32_t *lists;          // r.nq x 2 kXrsList words: the survivors' row ids; after the re-rank the kept row ids, then their distances
};

inline size_t xrs_list_words(uint32_t nq) { return (size_t)nq * 2 * kXrsList; }
// dim % 16 == 0 and dim <= 4096; anything else is exact_range.hip's.
bool xrs_supported(uint32_t dim);
// Positions of the query tile staged in LDS at a time: dim up to xrs_whole_dim(), else slices of 128.
uint32_t xrs_slice(uint32_t dim);
uint32_t xrs_whole_dim();
// Row chunks of the screen, a multiple of 64 rows each.
void xrs_plan(uint32_t n, uint32_t nq, uint32_t *grid_y, uint32_t *rows_per_block);
const char *xrs_kernel_name(int fmt);

// rows / fmt, candidates and the filter's bad counter as launch_exact_range_count.  Nothing synchronises, nothing is read back.
// Clearing, norms, screen, re-rank and count, the count pass of the flagged queries, the exclusive scan: a.r.counts, a.r.bases and
// a.r.out_offsets are complete behind it, whatever a.r.cap is.  a.r.nq >= 1.
hipError_t launch_exact_range_screen_count(const DevIndex &ix, const void *rows, int fmt, const RangeScreenArgs &a, const FilterArgs *f, hipStream_t stream);
// The copy of the kept entries, the fill pass of the flagged queries, the segment sort -- after launch_exact_range_screen_count on the
// same stream.  Every kernel reads out_offsets[nq] on the device: above a.r.cap they write nothing but *a.r.over.
hipError_t launch_exact_range_screen_fill(const DevIndex &ix, const void *rows, int fmt, const RangeScreenArgs &a, const FilterArgs *f, hipStream_t stream);

}  // namespace hs
