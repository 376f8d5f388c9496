// update_records.hpp -- the host half of the one write path for changed nodes of a resident index (capi_resident.cpp): the staging
// buffer that index_update.hip's record kernel consumes, built from a PackedIndex made without rows.  Needs no HIP
// (csrc/update_records_test.cpp runs it stand-alone); the layout is described at the top of index_update.hip.
#pragma once
#include <algorithm>
#include <cstring>
#include <iterator>

#include "packed_index.hpp"

namespace hs {

struct UpdateRecords {
  std::vector<uint32_t> stage;   // header nrec x 4 | tiles nrec x stride | rows (nrec - first_row) x row_words, the rows only when asked for
  uint32_t nrec = 0, first_row = 0;   // records [first_row, nrec) carry a row
  uint32_t row_words = 0;             // dim rounded up to a multiple of 4
};

// `changed`: the ids whose level-0 list, label or mark changed; `row_ids`: the ids that also carry a row (in `changed` or not).
// Both in any order, with repeats: every id becomes one record, the list-only records first and the row records after, both
// ascending.  row_of(id) is the fp32 row of the host image; with_rows = false leaves the rows section out (the kernel then reads
// them from rows already on the device).  `stride` is the tile stride in ids (a multiple of 16, at least the longest list).
// Returns false, `out` untouched, when an id is not below `limit`.
template <class RowOf>
bool build_update_records(const PackedIndex &p, uint32_t stride, size_t limit, std::vector<uint32_t> changed, std::vector<uint32_t> row_ids,
                          bool with_rows, RowOf row_of, UpdateRecords &out) {
  auto distinct = [](std::vector<uint32_t> &v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
  };
  distinct(changed);
  distinct(row_ids);
  std::vector<uint32_t> ids;
  std::set_difference(changed.begin(), changed.end(), row_ids.begin(), row_ids.end(), std::back_inserter(ids));
  const size_t first_row = ids.size(), nrow = row_ids.size(), nrec = first_row + nrow;
  ids.insert(ids.end(), row_ids.begin(), row_ids.end());
  for (uint32_t id : ids)
    if (id >= limit) return false;
  const size_t dim = p.dim, row_words = (dim + 3) / 4 * 4, rows_at = nrec * (4 + (size_t)stride);
  out.stage.assign(rows_at + (with_rows ? nrow * row_words : 0), 0);
  out.nrec = (uint32_t)nrec; out.first_row = (uint32_t)first_row; out.row_words = (uint32_t)row_words;
  uint32_t *tiles = out.stage.data() + nrec * 4;
  std::fill(tiles, tiles + nrec * stride, 0xFFFFFFFFu);
  for (size_t r = 0; r < nrec; r++) {
    const uint32_t id = ids[r];
    uint32_t *h = out.stage.data() + r * 4;
    h[0] = id; h[1] = p.deleted[id]; h[2] = (uint32_t)p.labels[id]; h[3] = (uint32_t)(p.labels[id] >> 32);
    std::copy(p.cols.begin() + p.row_ptr0[id], p.cols.begin() + p.row_ptr0[id + 1], tiles + r * stride);
  }
  if (with_rows)
    for (size_t i = 0; i < nrow; i++) memcpy(out.stage.data() + rows_at + i * row_words, row_of(row_ids[i]), 4 * dim);
  return true;
}

}  // namespace hs
