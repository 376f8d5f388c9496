// exact_engine.hpp -- launch interface of the exact k-NN scan over the rows of a resident index (exact_search.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine.hpp"

namespace hs {

// One call: nq queries against the rows the index holds.  Geometry and workspace are the exhaustive scan's (bf_engine.hpp
// bf_partial_bytes: `partial` of that many bytes, grid_x row chunks of rows_per_block rows, a multiple of 64).
struct ExactArgs {
  const float *queries;    // nq x dim (device)
  uint32_t nq, k;          // 1 <= k <= 64
  const uint32_t *order;   // nullable: a permutation of [0, nq) -- tile slot s serves query order[s]; outputs stay at the query's own position
  void *partial;
  uint32_t grid_x, rows_per_block;
  uint64_t *out_labels;    // nq x k, ascending (dist, label); ~0 / +inf beyond out_counts[q]
  float *out_dists;
  uint32_t *out_counts;    // nullable
};

// Dynamic LDS of the scan kernels: the query tile, a sorted k-list per (wave, query), their sizes, the tile's slots.
size_t exact_lds_bytes(uint32_t dim, uint32_t k);
// Candidates of query i: internal ids j < ix.n that are not marked deleted (ix.has_deleted) and, with f != null, whose bit is set in
// row f->of_query[i] (FilterArgs, engine.hpp; a filter index >= f->nf: count 0, padding outputs, *f->bad raised once).
// rows / fmt: ROWS_F32 reads ix.vec (rows ignored; dim % 16 != 0 takes the one-lane-per-row recipes), ROWS_U8 / ROWS_F16 read `rows`,
// the index's narrow copy (dim % 16 == 0).  Labels come from ix.labels.  Nothing synchronises: the scan and the merge are enqueued.
hipError_t launch_exact_search(const DevIndex &ix, const void *rows, int fmt, const ExactArgs &a, const FilterArgs *f, hipStream_t stream);

}  // namespace hs
