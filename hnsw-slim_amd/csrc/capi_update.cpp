// capi_update.cpp -- the C ABI (include/hnsw_slim_amd.h): a resident vanilla index that changes -- addPoint on its host image, for
// new labels (hs_index_add_points; in the batched order, on the index's device, hs_index_add_points_batched) and as the reference's
// upsert with replace_deleted (hs_index_upsert_points), with the changed
// rows written in place on the device (write_changed, capi_resident.cpp); markDelete / unmarkDelete, resizeIndex, saveIndex, getDataByLabel; and
// the host-only replay of an operation list (hs_hnsw_replay).
#include "capi_internal.hpp"

#include <unordered_set>

#include "build_engine.hpp"
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

static constexpr const char *kAddNomem = "Not enough memory: addPoint failed to allocate linklist";

// the reference's exception texts with the statuses the header documents
static hs_status update_exception(const std::exception &e) {
  if (std::string(e.what()) == "The number of elements exceeds the specified limit") return fail(HS_ERR_CAPACITY, e.what());
  return from_exception(e);
}

hs_status hs_index_seed_levels(hs_index *ix, size_t seed, size_t drawn) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (!ix->host_vanilla) return fail(HS_ERR_INVALID, "index not growable: load a vanilla index with max_elements > its element count");
  return guarded([&] {
    seed_levels(*ix->host_vanilla, seed, drawn);
    return HS_OK;
  });
}

size_t hs_index_capacity(const hs_index *ix) {
  if (!ix) return 0;
  return ix->host_vanilla ? ix->host_vanilla->max_elements : std::max<size_t>(ix->cap_rows, ix->info.n);
}

size_t hs_index_deleted_count(const hs_index *ix) { return ix ? ix->num_deleted : 0; }

// What hs_index_add_points and hs_index_add_points_batched refuse, all of it before anything changes: capacity, a label that exists or
// appears twice in the call, a row the narrow format cannot represent.  *empty: count == 0 passed the capacity check (nothing to do).
static hs_status check_new_points(hs_index *ix, const float *rows, const uint64_t *labels, size_t count, bool *empty) {
  const size_t n0 = ix->info.n, dim = ix->info.dim;
  *empty = false;
  if (count && (!ix->host_vanilla || n0 + count > ix->host_vanilla->max_elements))
    return fail(HS_ERR_CAPACITY, "The number of elements exceeds the specified limit");   // hnswalg.h:1274-1277
  if (count == 0) { *empty = true; return HS_OK; }
  ensure_update_state(ix);
  const hs_status ls = labels_new_ok([&](uint64_t label) { return ix->label_to_id.count(label) != 0; }, labels, count);
  if (ls != HS_OK) return ls;
  if (ix->row_fmt != ROWS_F32)
    for (size_t i = 0; i < count; i++) {
      const size_t j = first_unfit(rows + i * dim, dim, ix->row_fmt);
      if (j < dim) return fail(HS_ERR_UNSUPPORTED, "add refused: " + unfit_message(i, j, rows[i * dim + j], ix->row_fmt));
    }
  return HS_OK;
}

// After the host image took `count` new nodes from id n0 on: the label map, then the device through the one write path.
static hs_status publish_new_points(hs_index *ix, const uint64_t *labels, size_t n0, size_t count, const std::vector<uint32_t> &touched,
                                    const float *src_vec) {
  VanillaGraph &g = *ix->host_vanilla;
  PackedIndex p;
  p.from_vanilla(g, false);
  for (size_t i = 0; i < count; i++) ix->label_to_id[labels[i]] = (uint32_t)(n0 + i);
  std::vector<uint32_t> row_ids(count);
  for (size_t i = 0; i < count; i++) row_ids[i] = (uint32_t)(n0 + i);
  return write_changed(ix, p, [&g](uint32_t i) { return g.vec(i); }, touched, row_ids, src_vec);
}

hs_status hs_index_add_points(hs_index *ix, const float *rows, const uint64_t *labels, size_t count, int threads) {
  if (!ix || (count && (!rows || !labels))) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind != HS_KIND_HNSW) return fail(HS_ERR_UNSUPPORTED, "addPoint is supported on a vanilla (HS_KIND_HNSW) index only");
  return guarded(kAddNomem, [&] {
    // everything is validated before anything changes
    bool empty = false;
    const hs_status cs = check_new_points(ix, rows, labels, count, &empty);
    if (cs != HS_OK || empty) return cs;
    const size_t n0 = ix->info.n;
    VanillaGraph &g = *ix->host_vanilla;
    std::vector<uint32_t> touched;
    {
      g.touched0 = &touched;
      const Restore clear([&g] { g.touched0 = nullptr; });
      resume(g, rows, labels, count, threads);
    }
    return publish_new_points(ix, labels, n0, count, touched, nullptr);
  });
}

// ---- batched addPoint into a resident index (host_batch_build.hpp, on the device build_gpu.hip) -------------------------
// The device run: on success the host image holds the new nodes and the changed old lists, `touched` the level-0 lists that changed.
// Nothing of the host image changes before the download has arrived.
static hs_status batched_add_device(hs_index *ix, const float *rows, const uint64_t *labels, size_t count, const hs_batch_build_opts *opts,
                                    hs_batch_build_stats &st, std::vector<uint32_t> &touched) {
  VanillaGraph &g = *ix->host_vanilla;
  const size_t n0 = g.count, n = n0 + count, s0 = g.maxM0 + 1;
  const int threads = std::max(1, (int)opts->threads);
  // (the level generator is put back when the device fails or anything throws: the call then changed nothing)
  Restore undo([&g, gen0 = g.level_gen] { g.level_gen = gen0; });
  std::vector<int> lv(count);
  for (size_t i = 0; i < count; i++) lv[i] = draw_level(g);
  const std::vector<BatchStep> steps = batch_schedule_from(lv.data(), count, n0, g.enterpoint, g.maxlevel, opts->grow_div, opts->batch_max);
  std::vector<uint32_t> lev(n), upb, l0, lu;
  for (size_t i = 0; i < n0; i++) lev[i] = (uint32_t)g.levels[i];
  for (size_t i = 0; i < count; i++) lev[n0 + i] = (uint32_t)lv[i];
  build_form_lists(g, n0, n, lev.data(), threads, upb, l0, lu);
  GpuAddInput in;
  in.d_vec = ix->vec.p; in.rows = rows; in.n0 = (uint32_t)n0; in.count = (uint32_t)count; in.dim = (uint32_t)g.dim; in.metric = (int)g.metric;
  in.M = (uint32_t)g.M; in.maxM = (uint32_t)g.maxM; in.maxM0 = (uint32_t)g.maxM0; in.efc = (uint32_t)g.efC;
  in.lev = lev.data(); in.steps = &steps; in.scratch_ids = (uint32_t)opts->scratch_ids;
  in.upb = &upb; in.lists0 = &l0; in.lists_up = &lu;
  GpuAddOutput out;
  const hipError_t e = gpu_batch_add(in, ix->device, out);
  const size_t nchg = out.tasks.size(), nup0 = upb[n0];
  bool sane = e == hipSuccess && out.slots.size() == (nchg + count + (upb[n] - nup0)) * s0;
  for (size_t j = 0; sane && j < nchg; j++) sane = out.tasks[j] < n0 || (out.tasks[j] >= n && out.tasks[j] - n < nup0);
  if (!sane) {
    if (e != hipSuccess) return fail(HS_ERR_DEVICE, std::string("batched add: ") + hipGetErrorString(e));
    return fail(HS_ERR_DEVICE, "batched add: the device returned lists outside the index");
  }
  std::vector<uint32_t>().swap(l0);
  std::vector<uint32_t>().swap(lu);
  // the new nodes as begin_insert lays them out, their lists from the download
  const uint32_t *slot = out.slots.data();
  for (size_t i = 0; i < count; i++) {
    const uint32_t id = (uint32_t)(n0 + i);
    char *el = g.el(id);
    memset(el, 0, g.size_per_el);
    memcpy(el, slot + (nchg + i) * s0, g.size_links0);
    memcpy(el + g.offsetData, rows + i * g.dim, 4 * g.dim);
    memcpy(el + g.label_offset, &labels[i], 8);
    g.levels[id] = lv[i];
    if (lv[i]) {
      g.links[id].assign(g.size_links_up * lv[i] + 1, 0);
      for (int l = 1; l <= lv[i]; l++)
        memcpy(g.links[id].data() + (size_t)(l - 1) * g.size_links_up, slot + (nchg + count + (upb[id] - nup0) + l - 1) * s0, g.size_links_up);
    }
    touched.push_back(id);
  }
  // the old lists that received an id, whole slots (what stands behind the count is saved too).  A full list whose re-prune
  // turned the new id away and kept its order comes back with the bytes it had: it is left alone.
  ix->last_add_changed.clear();
  ix->last_add_downloaded = nchg;
  for (size_t j = 0; j < nchg; j++) {
    const uint32_t task = out.tasks[j];
    uint32_t u = task;
    if (task < n0) {
      if (memcmp(g.el(u), slot + j * s0, g.size_links0) == 0) continue;
      memcpy(g.el(u), slot + j * s0, g.size_links0);
      touched.push_back(u);
    } else {
      const uint32_t us = task - (uint32_t)n;   // upper slot: node u's level us - upb[u] + 1
      u = (uint32_t)(std::upper_bound(upb.begin(), upb.begin() + n0 + 1, us) - upb.begin() - 1);
      uint32_t *l = g.list_at(u, (int)(us - upb[u] + 1));
      if (memcmp(l, slot + j * s0, g.size_links_up) == 0) continue;
      memcpy(l, slot + j * s0, g.size_links_up);
    }
    ix->last_add_changed.push_back(u);
  }
  std::sort(ix->last_add_changed.begin(), ix->last_add_changed.end());
  ix->last_add_changed.erase(std::unique(ix->last_add_changed.begin(), ix->last_add_changed.end()), ix->last_add_changed.end());
  g.count = n;
  for (size_t i = 0; i < count; i++)   // (adopt_entry: a row above the top level becomes the entry point)
    if (lv[i] > g.maxlevel) { g.maxlevel = lv[i]; g.enterpoint = (uint32_t)(n0 + i); }
  st.used_gpu = 1; st.batches = steps.size(); st.flagged_rows = out.flagged_rows; st.kernel_ms = out.kernel_ms;
  undo.dismiss();
  return HS_OK;
}

hs_status hs_index_add_points_batched(hs_index *ix, const float *rows, const uint64_t *labels, size_t count, const hs_batch_build_opts *opts,
                                      hs_batch_build_stats *stats) {
  if (!ix || (count && (!rows || !labels))) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind != HS_KIND_HNSW) return fail(HS_ERR_UNSUPPORTED, "addPoint is supported on a vanilla (HS_KIND_HNSW) index only");
  hs_status cs = batch_opts_ok(opts);
  if (cs != HS_OK) return cs;
  return guarded(kAddNomem, [&] {
    if (opts->device != -1 && opts->device != ix->device)
      return fail(HS_ERR_INVALID, "device: -1 (the host twin) or the index's own device (" + std::to_string(ix->device) + ")");
    const auto t0 = std::chrono::steady_clock::now();
    hs_batch_build_stats st{};
    bool empty = false;
    cs = check_new_points(ix, rows, labels, count, &empty);
    if (cs != HS_OK) return cs;
    if (empty) { if (stats) *stats = st; return HS_OK; }
    if (ix->num_deleted > 0) return fail(HS_ERR_UNSUPPORTED, kBatchedAddMarksRefusal);
    VanillaGraph &g = *ix->host_vanilla;
    const size_t n0 = g.count;
    // the device takes the build's shapes, on an index that holds fp32 rows with room behind them; anything else is the host twin's
    const bool on_device = opts->device >= 0 && n0 > 0 && n0 + count <= 0x7FFFFFF0u && ix->f32_resident && ix->vec.p &&
                           ix->vec.n >= (n0 + count) * g.dim && g.maxM == g.M && g.maxM0 == 2 * g.M &&
                           gpu_build_supported((uint32_t)g.dim, (uint32_t)g.M, (uint32_t)g.efC, (uint32_t)opts->scratch_ids);
    std::vector<uint32_t> touched;
    ix->last_add_changed.clear();
    ix->last_add_downloaded = 0;
    if (on_device) {
      HIP_TRY(hipSetDevice(ix->device));
      HIP_TRY(hipDeviceSynchronize());   // no search may be in flight on this index while its rows grow
      cs = batched_add_device(ix, rows, labels, count, opts, st, touched);
      if (cs != HS_OK) return cs;
    } else {
      BatchBuildStats bs;
      g.touched0 = &touched;
      const Restore clear([&g] { g.touched0 = nullptr; });
      batch_add_host(g, rows, labels, count, std::max(1, (int)opts->threads), opts->grow_div, opts->batch_max, &bs);
      st.batches = bs.batches;
    }
    cs = publish_new_points(ix, labels, n0, count, touched, on_device ? ix->vec.p : nullptr);
    st.total_ms = ms_since(t0);
    if (stats) *stats = st;
    return cs;
  });
}

// Diagnostic: what the device path of the last hs_index_add_points_batched brought back beside the new nodes -- *lists_downloaded
// (nullable) old lists that received an id, and the old nodes (internal ids below the element count before the call, ascending)
// among them whose level-0 or upper list bytes changed.  Both empty after a call the host twin served.  ids nullable; at most `cap`
// are written, *count receives how many there are.
hs_status hs_debug_batched_add_changed(const hs_index *ix, uint32_t *ids, size_t cap, size_t *count, size_t *lists_downloaded) {
  if (!ix || !count) return fail(HS_ERR_INVALID, "null argument");
  *count = ix->last_add_changed.size();
  if (lists_downloaded) *lists_downloaded = ix->last_add_downloaded;
  if (ids) std::copy_n(ix->last_add_changed.begin(), std::min(cap, ix->last_add_changed.size()), ids);
  return HS_OK;
}

hs_status hs_index_mark_deleted(hs_index *ix, const uint64_t *labels, size_t count, int on) {
  if (!ix || (count && !labels)) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind != HS_KIND_HNSW) return fail(HS_ERR_UNSUPPORTED, "markDelete is supported on a vanilla (HS_KIND_HNSW) index only");
  if (count == 0) return HS_OK;
  if (count > 0xFFFFFFFFu) return fail(HS_ERR_INVALID, "too many labels");
  return guarded([&] {
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
  });
}

hs_status hs_index_save(const hs_index *ix, const char *path) {
  if (!ix || !path) return fail(HS_ERR_INVALID, "null argument");
  if (!ix->host_vanilla) return fail(HS_ERR_INVALID, "index holds no host image to save: load a vanilla index with max_elements > its element count");
  return guarded([&] {
    ix->host_vanilla->save(path);
    return HS_OK;
  });
}

hs_status hs_index_get_row(hs_index *ix, uint64_t label, float *out) {
  if (!ix || !out) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind == HS_KIND_SLIMQ) return fail(HS_ERR_UNSUPPORTED, "getDataByLabel: a SlimQ index holds RaBitQ records, not rows");
  return guarded([&] {
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
  });
}

// ---- upsert, replace_deleted, resizeIndex -------------------------------------------------------------------------------------
hs_status hs_index_set_replace_deleted(hs_index *ix, int on) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (ix->info.kind != HS_KIND_HNSW) return fail(HS_ERR_UNSUPPORTED, "replace_deleted is supported on a vanilla (HS_KIND_HNSW) index only");
  if (!ix->host_vanilla) return fail(HS_ERR_INVALID, "index holds no host image to update: load a vanilla index with max_elements > its element count");
  return guarded([&] {
    set_allow_replace(*ix->host_vanilla, on != 0);
    return HS_OK;
  });
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
  return guarded(kAddNomem, [&] {
    ensure_update_state(ix);
    hs_status cs = check_upserts(ix, rows, labels, replace_flags, count);
    if (cs != HS_OK) return cs;
    VanillaGraph &g = *ix->host_vanilla;
    const size_t dim = ix->info.dim;
    std::vector<uint32_t> touched, row_ids;
    {
      g.touched0 = &touched;
      const Restore clear([&g] { g.touched0 = nullptr; });
      VanillaGraph::Visited vl;
      for (size_t i = 0; i < count; i++)
        row_ids.push_back(upsert(g, rows + i * dim, labels[i], replace_flags && replace_flags[i], ix->label_to_id, vl));
    }
    PackedIndex p;
    p.from_vanilla(g, false);
    return write_changed(ix, p, [&g](uint32_t i) { return g.vec(i); }, touched, row_ids);
  }, update_exception);
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
  return guarded("Not enough memory: resizeIndex failed to allocate base layer", [&] {
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
    resize(g, new_max_elements);
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
  });
}

// ---- host only: loadIndex, a list of operations, saveIndex --------------------------------------------------------------------
hs_status hs_hnsw_replay(const char *in_path, int metric, size_t dim, size_t max_elements, int allow_replace_deleted, const uint64_t *ops,
                         size_t n_ops, const float *rows, const char *out_path) {
  if (!in_path || !out_path || (n_ops && !ops)) return fail(HS_ERR_INVALID, "bad argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  return guarded("Not enough memory", [&] {
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
    return HS_OK;
  }, update_exception);
}
