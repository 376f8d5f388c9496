// index_update.hpp -- launch interface of index_update.hip (in-place updates of a resident vanilla index), shared with the C ABI
// (capi_update.cpp).  The staging-buffer layout is described at the top of index_update.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hs {

constexpr uint32_t kUpdateBlock = 256;   // four records per workgroup, one wavefront each

struct UpdateArgs {
  const uint32_t *stage;   // the uploaded staging buffer (device)
  uint32_t nrec, first_row;   // records [first_row, nrec) carry a row
  uint32_t stride;         // tile stride in ids (16 / 32 / 48 / 64); ignored when tile0 is null
  uint32_t dim, row_words; // row_words = dim rounded up to a multiple of 4
  uint32_t cap_rows;       // rows every per-node array below is allocated for
  int32_t fmt;             // hs_row_format of `narrow`
  uint32_t *tile0;         // nullable (an index whose degree exceeds 64 has no tiles)
  float *vec;              // nullable (an index without resident fp32 rows)
  void *narrow;            // nullable (an index in HS_ROWS_F32 format)
  uint64_t *labels;
  uint8_t *deleted;
  const float *src_vec;    // nullable; when set, the row of a record is read from src_vec + id * dim (rows already on the device:
                           // hs_slim_convert_diff takes them from the resident HNSW index) and the buffer holds no rows section
};

hipError_t launch_index_update(const UpdateArgs &a, hipStream_t stream);
hipError_t launch_mark_scatter(const uint32_t *d_stage, uint32_t count, uint32_t n, uint8_t *d_deleted, hipStream_t stream);

}  // namespace hs
