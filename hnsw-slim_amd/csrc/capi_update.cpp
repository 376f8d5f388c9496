// capi_update.cpp -- the C ABI (include/hnsw_slim_amd.h): a resident vanilla index that changes -- addPoint on its host image with
// the changed rows written in place on the device (index_update.hip), markDelete / unmarkDelete, saveIndex, getDataByLabel.
#include "capi_internal.hpp"

#include "index_update.hpp"

// label_lookup_ and num_deleted_ (hnswalg.h:61, loadIndex :866-888), from the arrays every index keeps on the host
static void ensure_update_state(hs_index *ix) {
  if (ix->label_map_built) return;
  ix->label_to_id.clear();
  ix->label_to_id.reserve(ix->host_labels.size());
  for (size_t i = 0; i < ix->host_labels.size(); i++) ix->label_to_id[ix->host_labels[i]] = (uint32_t)i;
  ix->num_deleted = 0;
  for (uint8_t d : ix->host_deleted) ix->num_deleted += d != 0;
  ix->label_map_built = true;
}

hs_status hs_index_seed_levels(hs_index *ix, size_t seed, size_t drawn) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (!ix->host_vanilla) return fail(HS_ERR_INVALID, "index not growable: load a vanilla index with max_elements > its element count");
  ix->host_vanilla->seed_levels(seed, drawn);
  return HS_OK;
}

size_t hs_index_capacity(const hs_index *ix) {
  if (!ix) return 0;
  return ix->host_vanilla ? ix->host_vanilla->max_elements : std::max<size_t>(ix->cap_rows, ix->info.n);
}

size_t hs_index_deleted_count(const hs_index *ix) {
  if (!ix) return 0;
  if (ix->label_map_built) return ix->num_deleted;
  size_t c = 0;
  for (uint8_t d : ix->host_deleted) c += d != 0;
  return c;
}

hs_status hs_index_add_points(hs_index *ix, const float *rows, const uint64_t *labels, size_t count, int threads) {
  if (!ix || (count && (!rows || !labels))) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind != HS_KIND_HNSW) return fail(HS_ERR_UNSUPPORTED, "addPoint is supported on a vanilla (HS_KIND_HNSW) index only");
  // everything is validated before anything changes
  const size_t n0 = ix->info.n, dim = ix->info.dim;
  if (count && (!ix->host_vanilla || n0 + count > ix->host_vanilla->max_elements))
    return fail(HS_ERR_CAPACITY, "The number of elements exceeds the specified limit");   // hnswalg.h:1274-1277
  if (count == 0) return HS_OK;
  ensure_update_state(ix);
  {
    std::unordered_map<uint64_t, size_t> seen;
    seen.reserve(count);
    for (size_t i = 0; i < count; i++) {
      if (ix->label_to_id.count(labels[i]))
        return fail(HS_ERR_UNSUPPORTED, "label " + std::to_string(labels[i]) + " (row " + std::to_string(i) + ") already exists: updatePoint is not supported");
      auto ins = seen.emplace(labels[i], i);
      if (!ins.second)
        return fail(HS_ERR_INVALID, "label " + std::to_string(labels[i]) + " appears twice in the call (rows " + std::to_string(ins.first->second) + " and " + std::to_string(i) + ")");
    }
  }
  if (ix->row_fmt != ROWS_F32)
    for (size_t i = 0; i < count; i++) {
      const size_t j = first_unfit(rows + i * dim, dim, ix->row_fmt);
      if (j < dim) return fail(HS_ERR_UNSUPPORTED, "add refused: " + unfit_message(i, j, rows[i * dim + j], ix->row_fmt));
    }
  VanillaGraph &g = *ix->host_vanilla;
  std::vector<uint32_t> touched;
  PackedIndex p;
  try {
    g.touched0 = &touched;
    g.resume(rows, labels, count, threads);
    g.touched0 = nullptr;
    p.from_vanilla(g, false);
  } catch (std::bad_alloc &) {
    g.touched0 = nullptr;
    return fail(HS_ERR_NOMEM, "Not enough memory: addPoint failed to allocate linklist");
  } catch (std::exception &e) {
    g.touched0 = nullptr;
    return from_exception(e);
  }
  for (size_t i = 0; i < count; i++) ix->label_to_id[labels[i]] = (uint32_t)(n0 + i);
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipDeviceSynchronize());   // no search may be in flight on this index while it is rewritten
  const uint32_t stride = tile_stride_for(p.max_deg0);
  if (stride != ix->dev.tile_stride || !ix->dev.tile0) {   // a list outgrew the tile stride: re-tile everything (as hs_index_patch)
    p.vec.resize(p.n * dim);
    for (size_t i = 0; i < p.n; i++) memcpy(&p.vec[i * dim], g.vec((uint32_t)i), 4 * dim);
    p.rows_on_device = false;
    hs_status us = upload(ix, p);
    if (us != HS_OK || ix->row_fmt == ROWS_F32 || !ix->f32_resident) return us;
    return build_narrow(ix, ix->row_fmt, ix->narrow);
  }
  // the changed nodes as records: existing nodes whose level-0 list was written, then the new nodes
  std::sort(touched.begin(), touched.end());
  touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
  std::vector<uint32_t> ids;
  for (uint32_t t : touched)
    if (t < n0) ids.push_back(t);
  const uint32_t first_new = (uint32_t)ids.size();
  for (size_t i = 0; i < count; i++) ids.push_back((uint32_t)(n0 + i));
  const size_t nrec = ids.size(), row_words = (dim + 3) / 4 * 4;
  std::vector<uint32_t> stage(nrec * (4 + (size_t)stride) + count * row_words, 0);
  uint32_t *tiles = stage.data() + nrec * 4;
  std::fill(tiles, tiles + nrec * stride, 0xFFFFFFFFu);
  for (size_t r = 0; r < nrec; r++) {
    const uint32_t id = ids[r];
    uint32_t *h = stage.data() + r * 4;
    h[0] = id; h[1] = p.deleted[id]; h[2] = (uint32_t)p.labels[id]; h[3] = (uint32_t)(p.labels[id] >> 32);
    std::copy(p.cols.begin() + p.row_ptr0[id], p.cols.begin() + p.row_ptr0[id + 1], tiles + r * stride);
  }
  for (size_t i = 0; i < count; i++) memcpy(stage.data() + nrec * (4 + (size_t)stride) + i * row_words, rows + i * dim, 4 * dim);
  HIP_TRY(ix->upd_stage.ensure(stage.size()));
  HIP_TRY(hipMemcpy(ix->upd_stage.p, stage.data(), stage.size() * 4, hipMemcpyHostToDevice));
  UpdateArgs a{};
  a.stage = ix->upd_stage.p; a.nrec = (uint32_t)nrec; a.first_new = first_new; a.stride = stride;
  a.dim = (uint32_t)dim; a.row_words = (uint32_t)row_words; a.cap_rows = (uint32_t)std::max(ix->cap_rows, n0);
  a.fmt = ix->row_fmt; a.tile0 = ix->tile0.p;
  a.vec = ix->f32_resident ? ix->vec.p : nullptr;
  a.narrow = ix->row_fmt != ROWS_F32 ? (void *)ix->narrow.p : nullptr;
  a.labels = ix->labels.p; a.deleted = ix->deleted.p;
  HIP_TRY(launch_index_update(a, nullptr));
  ix->host_labels = p.labels;
  ix->host_deleted = p.deleted;
  hs_status s = upload_small(ix, p);
  if (s != HS_OK) return s;
  HIP_TRY(hipDeviceSynchronize());
  return HS_OK;
}

hs_status hs_index_mark_deleted(hs_index *ix, const uint64_t *labels, size_t count, int on) {
  if (!ix || (count && !labels)) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind != HS_KIND_HNSW) return fail(HS_ERR_UNSUPPORTED, "markDelete is supported on a vanilla (HS_KIND_HNSW) index only");
  if (count == 0) return HS_OK;
  if (count > 0xFFFFFFFFu) return fail(HS_ERR_INVALID, "too many labels");
  ensure_update_state(ix);
  // all or nothing: the marks of the call are played against a copy first (a label named twice meets its own first mark)
  std::vector<uint32_t> stage(count + (count + 3) / 4, 0);
  uint8_t *marks = reinterpret_cast<uint8_t *>(stage.data() + count);
  std::unordered_map<uint32_t, uint8_t> pending;
  for (size_t i = 0; i < count; i++) {
    auto it = ix->label_to_id.find(labels[i]);
    if (it == ix->label_to_id.end()) return fail(HS_ERR_INVALID, "Label not found");   // hnswalg.h:929-931, 974-976
    const uint32_t id = it->second;
    auto pd = pending.find(id);
    const bool cur = pd != pending.end() ? pd->second != 0 : ix->host_deleted[id] != 0;
    if (on && cur) return fail(HS_ERR_INVALID, "The requested to delete element is already deleted");        // :955-956
    if (!on && !cur) return fail(HS_ERR_INVALID, "The requested to undelete element is not deleted");         // :998-999
    pending[id] = on ? 1 : 0;
    stage[i] = id;
    marks[i] = on ? 1 : 0;
  }
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipDeviceSynchronize());   // no search may be in flight on this index while its marks change
  HIP_TRY(ix->upd_stage.ensure(stage.size()));
  HIP_TRY(hipMemcpy(ix->upd_stage.p, stage.data(), stage.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(launch_mark_scatter(ix->upd_stage.p, (uint32_t)count, (uint32_t)ix->info.n, ix->deleted.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  for (const auto &kv : pending) {
    const bool was = ix->host_deleted[kv.first] != 0, now = kv.second != 0;
    if (was == now) continue;   // (marked and unmarked again inside one call cannot happen: `on` is one value per call)
    ix->host_deleted[kv.first] = kv.second;
    if (ix->host_vanilla) ix->host_vanilla->set_deleted(kv.first, now);
    if (now) ix->num_deleted++; else ix->num_deleted--;
  }
  // bare_bone_search = !num_deleted_ && !isIdAllowed (hnswalg.h:1421), in both directions
  ix->dev.has_deleted = ix->num_deleted > 0;
  ix->info.has_deleted = ix->num_deleted > 0;
  return HS_OK;
}

hs_status hs_index_save(const hs_index *ix, const char *path) {
  if (!ix || !path) return fail(HS_ERR_INVALID, "null argument");
  if (!ix->host_vanilla) return fail(HS_ERR_INVALID, "index holds no host image to save: load a vanilla index with max_elements > its element count");
  try {
    ix->host_vanilla->save(path);
  } catch (std::exception &e) {
    return from_exception(e);
  }
  return HS_OK;
}

hs_status hs_index_get_row(hs_index *ix, uint64_t label, float *out) {
  if (!ix || !out) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind == HS_KIND_SLIMQ) return fail(HS_ERR_UNSUPPORTED, "getDataByLabel: a SlimQ index holds RaBitQ records, not rows");
  ensure_update_state(ix);
  auto it = ix->label_to_id.find(label);
  if (it == ix->label_to_id.end() || ix->host_deleted[it->second]) return fail(HS_ERR_INVALID, "Label not found");   // hnswalg.h:902-904
  const size_t id = it->second, dim = ix->info.dim;
  HIP_TRY(hipSetDevice(ix->device));
  if (ix->f32_resident) {
    HIP_TRY(hipMemcpy(out, ix->vec.p + id * dim, dim * 4, hipMemcpyDeviceToHost));
    return HS_OK;
  }
  // an index without fp32 rows: its narrow row, widened (exact) out of the lane-major layout
  const size_t w = narrow_width(ix->row_fmt);
  std::vector<uint8_t> raw(dim * w);
  HIP_TRY(hipMemcpy(raw.data(), ix->narrow.p + id * dim * w, dim * w, hipMemcpyDeviceToHost));
  for (size_t j = 0; j < dim; j++) {
    const size_t o = narrow_slot((uint32_t)j, (uint32_t)dim);
    if (ix->row_fmt == ROWS_U8) out[j] = (float)raw[o];
    else { _Float16 h; memcpy(&h, raw.data() + 2 * o, 2); out[j] = (float)h; }
  }
  return HS_OK;
}
