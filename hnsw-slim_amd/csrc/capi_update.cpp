// capi_update.cpp -- the C ABI (include/hnsw_slim_amd.h): a resident vanilla index that changes -- addPoint on its host image, for
// new labels (hs_index_add_points) and as the reference's upsert with replace_deleted (hs_index_upsert_points), with the changed
// rows written in place on the device (write_changed, capi_resident.cpp); markDelete / unmarkDelete, resizeIndex, saveIndex, getDataByLabel; and
// the host-only replay of an operation list (hs_hnsw_replay).
#include "capi_internal.hpp"

#include <unordered_set>

#include "host_update.hpp"
#include "index_update.hpp"

// label_lookup_ (hnswalg.h:61, loadIndex :866-888), from the labels every index keeps on the host
static void ensure_update_state(hs_index *ix) {
  if (ix->label_map_built) return;
  ix->label_to_id.clear();
  ix->label_to_id.reserve(ix->host_labels.size());
  for (size_t i = 0; i < ix->host_labels.size(); i++) ix->label_to_id[ix->host_labels[i]] = (uint32_t)i;
  ix->label_map_built = true;
}

// the reference's exception texts with the statuses the header documents
static hs_status update_exception(const std::exception &e) {
  if (std::string(e.what()) == "The number of elements exceeds the specified limit") return fail(HS_ERR_CAPACITY, e.what());
  return from_exception(e);
}

hs_status hs_index_seed_levels(hs_index *ix, size_t seed, size_t drawn) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (!ix->host_vanilla) return fail(HS_ERR_INVALID, "index not growable: load a vanilla index with max_elements > its element count");
  seed_levels(*ix->host_vanilla, seed, drawn);
  return HS_OK;
}

size_t hs_index_capacity(const hs_index *ix) {
  if (!ix) return 0;
  return ix->host_vanilla ? ix->host_vanilla->max_elements : std::max<size_t>(ix->cap_rows, ix->info.n);
}

size_t hs_index_deleted_count(const hs_index *ix) { return ix ? ix->num_deleted : 0; }

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
    resume(g, rows, labels, count, threads);
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
  std::vector<uint32_t> row_ids(count);
  for (size_t i = 0; i < count; i++) row_ids[i] = (uint32_t)(n0 + i);
  return write_changed(ix, p, [&g](uint32_t i) { return g.vec(i); }, touched, row_ids);
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
  // applied in call order (every id occurs once: `on` is one value per call and a repeated label is refused above), which is the
  // order deleted_elements receives them in when replacement is allowed (hnswalg.h:949-952, 992-995)
  for (size_t i = 0; i < count; i++) {
    const uint32_t id = stage[i];
    ix->host_deleted[id] = on ? 1 : 0;
    if (ix->host_vanilla) { if (on) mark(*ix->host_vanilla, id); else unmark(*ix->host_vanilla, id); }
  }
  // bare_bone_search = !num_deleted_ && !isIdAllowed (hnswalg.h:1421), in both directions
  const size_t nd = on ? ix->num_deleted + count : ix->num_deleted - count;
  set_delete_marks(ix, nd, nd > 0);
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

// ---- upsert, replace_deleted, resizeIndex -------------------------------------------------------------------------------------
hs_status hs_index_set_replace_deleted(hs_index *ix, int on) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (ix->info.kind != HS_KIND_HNSW) return fail(HS_ERR_UNSUPPORTED, "replace_deleted is supported on a vanilla (HS_KIND_HNSW) index only");
  if (!ix->host_vanilla) return fail(HS_ERR_INVALID, "index holds no host image to update: load a vanilla index with max_elements > its element count");
  set_allow_replace(*ix->host_vanilla, on != 0);
  return HS_OK;
}

// What hs_index_upsert_points would do, played on overlays of the label map, the marks and a copy of deleted_elements (a copy of a
// libstdc++ unordered_set keeps the bucket count and the element order, so `*begin()` of the copy is the original's at every step).
// Returns HS_OK when every point of the call will be accepted.
static hs_status check_upserts(const hs_index *ix, const float *rows, const uint64_t *labels, const uint8_t *flags, size_t count) {
  const VanillaGraph &g = *ix->host_vanilla;
  const size_t dim = ix->info.dim;
  std::unordered_map<uint64_t, int64_t> label_ov;    // label -> internal id, -1: left the map
  std::unordered_map<uint32_t, uint64_t> id_label;   // labels written by the call
  std::unordered_map<uint32_t, bool> mark_ov;
  std::unordered_set<uint32_t> vacant;
  bool vacant_copied = false;
  size_t n = g.count;
  auto find = [&](uint64_t lab) -> int64_t {
    auto o = label_ov.find(lab);
    if (o != label_ov.end()) return o->second;
    auto b = ix->label_to_id.find(lab);
    return b == ix->label_to_id.end() ? -1 : (int64_t)b->second;
  };
  auto marked = [&](uint32_t id) {
    auto o = mark_ov.find(id);
    return o != mark_ov.end() ? o->second : (id < g.count && g.deleted(id));
  };
  for (size_t i = 0; i < count; i++) {
    const bool flag = flags && flags[i];
    if (flag && !g.allow_replace) return fail(HS_ERR_INVALID, "Replacement of deleted elements is disabled in constructor");   // hnswalg.h:1027-1030
    if (ix->row_fmt != ROWS_F32) {
      const size_t j = first_unfit(rows + i * dim, dim, ix->row_fmt);
      if (j < dim) return fail(HS_ERR_UNSUPPORTED, "add refused: " + unfit_message(i, j, rows[i * dim + j], ix->row_fmt));
    }
    if (flag && !vacant_copied) { vacant = g.deleted_elements; vacant_copied = true; }
    if (flag && !vacant.empty()) {
      const uint32_t id = *vacant.begin();
      vacant.erase(id);
      auto il = id_label.find(id);
      label_ov[il != id_label.end() ? il->second : g.label(id)] = -1;
      label_ov[labels[i]] = id;
      id_label[id] = labels[i];
      mark_ov[id] = false;
      continue;
    }
    const int64_t id = find(labels[i]);
    if (id >= 0) {
      if (g.allow_replace && marked((uint32_t)id))   // :1257-1263
        return fail(HS_ERR_INVALID, "Can't use addPoint to update deleted elements if replacement of deleted elements is enabled.");
      mark_ov[(uint32_t)id] = false;
      continue;
    }
    if (n >= g.max_elements) return fail(HS_ERR_CAPACITY, "The number of elements exceeds the specified limit");   // :1274-1277
    label_ov[labels[i]] = (int64_t)n;
    id_label[(uint32_t)n] = labels[i];
    n++;
  }
  return HS_OK;
}

hs_status hs_index_upsert_points(hs_index *ix, const float *rows, const uint64_t *labels, const uint8_t *replace_flags, size_t count) {
  if (!ix || (count && (!rows || !labels))) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind != HS_KIND_HNSW) return fail(HS_ERR_UNSUPPORTED, "addPoint is supported on a vanilla (HS_KIND_HNSW) index only");
  if (count && !ix->host_vanilla) {
    if (replace_flags && std::any_of(replace_flags, replace_flags + count, [](uint8_t f) { return f != 0; }))
      return fail(HS_ERR_INVALID, "index holds no host image to update: load a vanilla index with max_elements > its element count");
    return fail(HS_ERR_CAPACITY, "The number of elements exceeds the specified limit");   // an index loaded without room, as hs_index_add_points
  }
  if (count == 0) return HS_OK;
  ensure_update_state(ix);
  hs_status cs = check_upserts(ix, rows, labels, replace_flags, count);
  if (cs != HS_OK) return cs;
  VanillaGraph &g = *ix->host_vanilla;
  const size_t dim = ix->info.dim;
  std::vector<uint32_t> touched, row_ids;
  PackedIndex p;
  try {
    g.touched0 = &touched;
    VanillaGraph::Visited vl;
    for (size_t i = 0; i < count; i++)
      row_ids.push_back(upsert(g, rows + i * dim, labels[i], replace_flags && replace_flags[i], ix->label_to_id, vl));
    g.touched0 = nullptr;
    p.from_vanilla(g, false);
  } catch (std::bad_alloc &) {
    g.touched0 = nullptr;
    return fail(HS_ERR_NOMEM, "Not enough memory: addPoint failed to allocate linklist");
  } catch (std::exception &e) {
    g.touched0 = nullptr;
    return update_exception(e);
  }
  return write_changed(ix, p, [&g](uint32_t i) { return g.vec(i); }, touched, row_ids);
}

// device-to-device move of the first `used` values of a per-node array into an allocation of `cap` values
template <typename T>
static hipError_t grow_into(DevBuf<T> &fresh, const DevBuf<T> &old, size_t cap, size_t used) {
  hipError_t e = fresh.alloc(std::max<size_t>(cap, 1));
  if (e != hipSuccess) return e;
  return used && old.p ? hipMemcpy(fresh.p, old.p, used * sizeof(T), hipMemcpyDeviceToDevice) : hipSuccess;
}
template <typename T>
static void take(DevBuf<T> &dst, DevBuf<T> &fresh) {
  std::swap(dst.p, fresh.p);
  std::swap(dst.n, fresh.n);
  fresh.release();
}

hs_status hs_index_resize(hs_index *ix, size_t new_max_elements) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (ix->info.kind != HS_KIND_HNSW) return fail(HS_ERR_UNSUPPORTED, "resizeIndex is supported on a vanilla (HS_KIND_HNSW) index only");
  if (new_max_elements < ix->info.n) return fail(HS_ERR_INVALID, "Cannot resize, max element is less than the current number of elements");   // hnswalg.h:690-692
  if (!ix->host_vanilla) return fail(HS_ERR_INVALID, "index holds no host image to resize: load a vanilla index with max_elements > its element count");
  if (new_max_elements > 0xFFFFFFFFull) return fail(HS_ERR_INVALID, "max_elements beyond 32-bit internal ids");
  VanillaGraph &g = *ix->host_vanilla;
  const size_t n = ix->info.n, dim = ix->info.dim, old_max = g.max_elements;
  const size_t have = std::max(ix->cap_rows, n);
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipDeviceSynchronize());   // no search may be in flight on this index while its arrays move
  const bool grow = new_max_elements > have;
  const size_t w = ix->row_fmt != ROWS_F32 ? narrow_width(ix->row_fmt) : 0;
  const uint32_t stride = ix->dev.tile_stride;
  DevBuf<float> vec;
  DevBuf<uint8_t> narrow, deleted;
  DevBuf<uint32_t> tile0, up_base;
  DevBuf<uint64_t> labels;
  if (grow) {
    // the new arrays first: a failure here leaves the index as it was
    const size_t cap = new_max_elements;
    hipError_t e = hipSuccess;
    if (e == hipSuccess && ix->f32_resident) e = grow_into(vec, ix->vec, cap * dim, n * dim);
    if (e == hipSuccess && w) e = grow_into(narrow, ix->narrow, std::max<size_t>(cap * dim * w, 16), n * dim * w);
    if (e == hipSuccess && ix->tile0.p) e = grow_into(tile0, ix->tile0, cap * stride, n * stride);
    if (e == hipSuccess) e = grow_into(labels, ix->labels, cap, n);
    if (e == hipSuccess) e = grow_into(deleted, ix->deleted, cap, n);
    if (e == hipSuccess) e = grow_into(up_base, ix->up_base, cap, std::min(n, ix->up_base.n));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(HS_ERR_NOMEM, "Not enough memory: resizeIndex failed to allocate the device arrays"); }
    HIP_TRY(e);
  }
  try {
    resize(g, new_max_elements);
  } catch (std::bad_alloc &) {
    return fail(HS_ERR_NOMEM, "Not enough memory: resizeIndex failed to allocate base layer");
  } catch (std::exception &e) {
    return from_exception(e);
  }
  if (grow) {
    if (ix->f32_resident) take(ix->vec, vec);
    if (w) take(ix->narrow, narrow);
    if (ix->tile0.p) take(ix->tile0, tile0);
    take(ix->labels, labels);
    take(ix->deleted, deleted);
    take(ix->up_base, up_base);
    DevIndex &d = ix->dev;
    d.vec = ix->vec.p; d.labels = ix->labels.p; d.deleted = ix->deleted.p; d.up_base = ix->up_base.p;
    d.tile0 = stride ? ix->tile0.p : nullptr;
    ix->cap_rows = new_max_elements;
    refresh_device_bytes(ix);
  }
  // indexSize() counts the level-0 link block and element_levels_ by max_elements (hnswalg.h:1533-1547)
  const size_t per = g.size_per_el - dim * 4 - 8 + sizeof(int);
  ix->info.index_size = ix->info.index_size + new_max_elements * per - old_max * per;
  return HS_OK;
}

// ---- host only: loadIndex, a list of operations, saveIndex --------------------------------------------------------------------
hs_status hs_hnsw_replay(const char *in_path, int metric, size_t dim, size_t max_elements, int allow_replace_deleted, const uint64_t *ops,
                         size_t n_ops, const float *rows, const char *out_path) {
  if (!in_path || !out_path || (n_ops && !ops)) return fail(HS_ERR_INVALID, "bad argument");
  if (metric != HS_METRIC_L2 && metric != HS_METRIC_IP) return fail(HS_ERR_INVALID, "bad metric");
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  try {
    VanillaGraph g;
    g.load(in_path, (Metric)metric, dim, max_elements);
    set_allow_replace(g, allow_replace_deleted != 0);
    std::unordered_map<uint64_t, uint32_t> lookup;   // label_lookup_ as loadIndex fills it (hnswalg.h:865-866)
    for (size_t i = 0; i < g.count; i++) lookup[g.label((uint32_t)i)] = (uint32_t)i;
    VanillaGraph::Visited vl;
    for (size_t o = 0; o < n_ops; o++) {
      const uint64_t kind = ops[4 * o], arg = ops[4 * o + 1], flag = ops[4 * o + 2], row = ops[4 * o + 3];
      if (kind == HS_OP_ADD) {
        if (!rows) return fail(HS_ERR_INVALID, "bad argument");
        upsert(g, rows + row * dim, arg, flag != 0, lookup, vl);
      } else if (kind == HS_OP_MARK || kind == HS_OP_UNMARK) {
        auto it = lookup.find(arg);
        if (it == lookup.end()) return fail(HS_ERR_INVALID, "Label not found");
        if (kind == HS_OP_MARK) mark(g, it->second); else unmark(g, it->second);
      } else if (kind == HS_OP_RESIZE) {
        resize(g, arg);
      } else {
        return fail(HS_ERR_INVALID, "bad operation kind " + std::to_string(kind));
      }
    }
    g.save(out_path);
  } catch (std::bad_alloc &) {
    return fail(HS_ERR_NOMEM, "Not enough memory");
  } catch (std::exception &e) {
    return update_exception(e);
  }
  return HS_OK;
}
