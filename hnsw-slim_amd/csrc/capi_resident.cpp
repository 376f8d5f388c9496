// capi_resident.cpp -- what every call that changes a resident index shares: the ONE write path for changed nodes (hs_index_patch,
// hs_index_add_points, hs_index_upsert_points, hs_slim_convert_diff: records built by update_records.hpp, written by
// index_update.hip), hs_info.device_bytes derived from the index's state, and the delete-mark counters.
#include "capi_internal.hpp"

#include "index_update.hpp"
#include "update_records.hpp"

void set_delete_marks(hs_index *ix, size_t num_deleted, bool has_deleted) {
  ix->num_deleted = num_deleted;
  ix->dev.has_deleted = has_deleted;
  ix->info.has_deleted = has_deleted;
}

// Every per-node array is allocated for the row capacity; base_bytes counts the fp32 rows per element (it always has), so an index
// with far more capacity than rows would go below zero without its fp32 rows: it stops there.
void refresh_device_bytes(hs_index *ix) {
  const size_t rows = std::max<size_t>(ix->cap_rows, ix->info.n) * ix->info.dim;
  size_t total = ix->base_bytes;
  if (ix->row_fmt != ROWS_F32) total += rows * narrow_width(ix->row_fmt);
  if (!ix->f32_resident) total -= std::min(total, rows * 4);
  ix->info.device_bytes = total;
}

hs_status write_changed(hs_index *ix, PackedIndex &p, const std::function<const float *(uint32_t)> &row_of, const std::vector<uint32_t> &changed,
                        const std::vector<uint32_t> &row_ids, const float *src_vec) {
  const size_t dim = p.dim;
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipDeviceSynchronize());   // no search may be in flight on this index while it is rewritten
  const uint32_t stride = tile_stride_for(p.max_deg0);
  if (stride != ix->dev.tile_stride || !ix->dev.tile0) {   // a list outgrew the tile stride: re-tile everything, rows from the host image
    p.vec.resize(p.n * dim);
    for (size_t i = 0; i < p.n; i++) memcpy(&p.vec[i * dim], row_of((uint32_t)i), 4 * dim);
    p.rows_on_device = false;
    hs_status us = upload(ix, p);   // (an index without fp32 rows: rebuilds the narrow copy from those rows, in chunks)
    if (us != HS_OK || ix->row_fmt == ROWS_F32 || !ix->f32_resident) return us;
    return build_narrow(ix, ix->row_fmt, ix->narrow);   // the fp32 rows were re-allocated: the narrow copy is rebuilt whole
  }
  const size_t cap = std::max(ix->cap_rows, p.n);
  UpdateRecords rec;
  if (!build_update_records(p, stride, p.n, changed, row_ids, !src_vec, row_of, rec))
    return fail(HS_ERR_INVALID, "internal: changed node outside the index");
  if (rec.nrec) {
    HIP_TRY(ix->upd_stage.ensure(rec.stage.size()));
    HIP_TRY(hipMemcpy(ix->upd_stage.p, rec.stage.data(), rec.stage.size() * 4, hipMemcpyHostToDevice));
    UpdateArgs a{};
    a.stage = ix->upd_stage.p; a.nrec = rec.nrec; a.first_row = rec.first_row; a.stride = stride;
    a.dim = (uint32_t)dim; a.row_words = rec.row_words; a.cap_rows = (uint32_t)cap;
    a.fmt = ix->row_fmt; a.tile0 = ix->tile0.p;
    a.vec = ix->f32_resident ? ix->vec.p : nullptr;
    a.narrow = ix->row_fmt != ROWS_F32 ? (void *)ix->narrow.p : nullptr;
    a.labels = ix->labels.p; a.deleted = ix->deleted.p;
    a.src_vec = src_vec;
    HIP_TRY(launch_index_update(a, nullptr));
  }
  hs_status s = upload_small(ix, p);
  if (s != HS_OK) return s;
  HIP_TRY(hipDeviceSynchronize());
  return HS_OK;
}
