// capi_diff.cpp -- the C ABI (include/hnsw_slim_amd.h): the patch server's side of the update loop -- convertFromHNSWWithDiff on two
// resident indexes (hs_slim_convert_diff; list passes in convert_diff.hip, element assembly and classification in slim_diff.hpp / slim_convert_gpu.hpp,
// the changed nodes written in place by write_changed), the stream and genPatch (hs_slim_diff_stream, hs_slim_diff_next), and
// the host-only twin on files (hs_slim_convert_diff_files).
#include "capi_internal.hpp"

#include <fstream>
#include <functional>

#include "slim_convert_gpu.hpp"

struct hs_slim_diff {
  SlimDiff d;
  std::unique_ptr<SlimGraph> own;   // hs_slim_convert_diff_files: the Slim image the records are cut from
  const hs_index *made_on = nullptr;
  uint64_t gen = 0;                 // made_on->slim_gen when the diff was made
};

hs_status hs_slim_convert_diff(hs_index *slim, hs_index *hnsw, float top_degree_percent0, float top_degree_percent, size_t top_degree_M0,
                               size_t low_degree_m0, size_t top_degree_M, size_t low_degree_m, int threads, hs_slim_diff **out, int *used_gpu,
                               double *kernel_ms) {
  if (!slim || !hnsw || !out) return fail(HS_ERR_INVALID, "null argument");
  *out = nullptr;
  // everything is validated before anything changes
  if (slim->info.kind != HS_KIND_SLIM || !slim->host_slim)
    return fail(HS_ERR_INVALID, "convertFromHNSWWithDiff: the target must be a Slim index loaded with max_elements > its element count");
  if (hnsw->info.kind != HS_KIND_HNSW || !hnsw->host_vanilla)
    return fail(HS_ERR_INVALID, "convertFromHNSWWithDiff: the source must be a vanilla index loaded with max_elements > its element count");
  SlimGraph &s = *slim->host_slim;
  const VanillaGraph &g = *hnsw->host_vanilla;
  if (s.dim != g.dim || s.metric != g.metric) return fail(HS_ERR_INVALID, "convertFromHNSWWithDiff: the two indexes differ in metric or dim");
  if (s.maxM != g.maxM || s.maxM0 != g.maxM0) return fail(HS_ERR_INVALID, "convertFromHNSWWithDiff: the two indexes differ in maxM / maxM0");
  if (g.count < s.count) return fail(HS_ERR_INVALID, "convertFromHNSWWithDiff: the vanilla index holds fewer elements than the Slim index");
  if (g.count > slim->cap_rows) return fail(HS_ERR_CAPACITY, "convertFromHNSWWithDiff: the vanilla index's element count exceeds the Slim index's max_elements");
  return guarded("Not enough memory: convertFromHNSW failed to allocate linklist", [&] {
    const size_t dim = g.dim;
    // an index with narrow rows takes only rows its format represents: every row the call would write is checked before anything
    // changes -- on the device path the rows the diff kernel found to differ, on the host path after a compare of all rows
    std::string unfit;
    auto fits = [&](uint32_t i) {
      const size_t j = first_unfit(g.vec(i), dim, slim->row_fmt);
      if (j < dim) unfit = "convertFromHNSWWithDiff refused: " + unfit_message(i, j, g.vec(i)[j], slim->row_fmt);
      return j >= dim;
    };
    const std::function<bool(const std::vector<uint32_t> &)> accept = [&](const std::vector<uint32_t> &stale) {
      for (uint32_t i : stale)
        if (!fits(i)) return false;
      return true;
    };
    const SlimParams p = slim_params(0, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0, top_degree_M, low_degree_m);
    std::unique_ptr<hs_slim_diff> df(new hs_slim_diff());
    bool gpu = false, same_device = false;
    double ms = 0.0;
    if (!slim->slim_lookup_built) {
      for (size_t i = 0; i < s.count; i++) slim->slim_lookup.map[s.label((uint32_t)i)] = (uint32_t)i;
      slim->slim_lookup_built = true;
    }
    same_device = slim->device == hnsw->device && hnsw->f32_resident && hnsw->vec.p;
    // the device path compares with the Slim index's own resident adjacency, rows and labels: it needs its tiles and fp32 rows
    if (same_device && slim->dev.tile0 && slim->f32_resident && slim->vec.p && g.count) {
      HIP_TRY(hipSetDevice(slim->device));
      HIP_TRY(hipDeviceSynchronize());   // no search may be in flight on either index
      DiffDev dd;
      dd.s_tile0 = slim->tile0.p; dd.s_stride = slim->dev.tile_stride;
      dd.s_up_base = slim->up_base.p; dd.s_up_ptr = slim->up_ptr.p; dd.n_up = (uint32_t)slim->up_ptr.n; dd.s_cols = slim->cols.p;
      dd.s_labels = slim->labels.p; dd.h_labels = hnsw->labels.p; dd.s_vec = slim->vec.p;
      std::string err;
      bool refused = false;
      gpu = convert_diff_gpu(s, g, p, hnsw->vec.p, hnsw->device, threads, slim->slim_lookup, dd, df->d, &ms, &err,
                               slim->row_fmt != ROWS_F32 ? &accept : nullptr, &refused);
      if (refused) return fail(HS_ERR_UNSUPPORTED, unfit);
      if (!gpu && !err.empty()) return fail(HS_ERR_DEVICE, err);
    }
    if (!gpu) {
      if (slim->row_fmt != ROWS_F32)
        for (size_t i = 0; i < g.count; i++) {
          if (i < s.count && memcmp(s.vec((uint32_t)i), g.vec((uint32_t)i), 4 * dim) == 0) continue;
          if (!fits((uint32_t)i)) return fail(HS_ERR_UNSUPPORTED, unfit);
        }
      convert_diff(s, g, p, threads, slim->slim_lookup.map, df->d);
      slim->slim_lookup.mismatch_valid = false;
    }
    slim->slim_gen++;
    // a call that changed no node and no header field touches nothing on the device; otherwise `dirty` are the nodes whose tile, row
    // or label changed, `stale` those of them that carry a row -- copied from the HNSW index's resident rows when both share a device
    if (!df->d.dirty.empty() || slim->info.n != s.count || slim->info.enterpoint != s.enterpoint || slim->info.maxlevel != s.maxlevel ||
        (slim->info.has_deleted != 0) != s.has_deleted) {
      PackedIndex pk;
      pk.from_slim(s, false);
      hs_status ws = write_changed(slim, pk, [&s](uint32_t i) { return s.vec(i); }, df->d.dirty, df->d.stale, same_device ? hnsw->vec.p : nullptr);
      if (ws != HS_OK) return ws;
    }
    if (used_gpu) *used_gpu = gpu ? 1 : 0;
    if (kernel_ms) *kernel_ms = gpu ? ms : 0.0;
    df->made_on = slim;
    df->gen = slim->slim_gen;
    *out = df.release();
    return HS_OK;
  });
}

hs_status hs_slim_diff_info(const hs_slim_diff *d, size_t *count, size_t *n_old, size_t *n_new, size_t *n_reprune) {
  if (!d) return fail(HS_ERR_INVALID, "null argument");
  if (count) *count = d->d.count;
  if (n_old) *n_old = d->d.old_ids.size();
  if (n_new) *n_new = d->d.new_ids.size();
  if (n_reprune) *n_reprune = d->d.n_reprune;
  return HS_OK;
}

hs_status hs_slim_diff_ids(const hs_slim_diff *d, uint32_t *old_ids, uint32_t *new_ids) {
  if (!d) return fail(HS_ERR_INVALID, "null argument");
  if (old_ids) std::copy(d->d.old_ids.begin(), d->d.old_ids.end(), old_ids);
  if (new_ids) std::copy(d->d.new_ids.begin(), d->d.new_ids.end(), new_ids);
  return HS_OK;
}

// the Slim image the diff's records are cut from; null (with the error set) when the pair does not belong together
static const SlimGraph *diff_image(const hs_slim_diff *d, const hs_index *slim) {
  if (!d) { fail(HS_ERR_INVALID, "null argument"); return nullptr; }
  if (d->own) {
    if (slim) { fail(HS_ERR_INVALID, "this diff owns its Slim image: pass a null index"); return nullptr; }
    return d->own.get();
  }
  if (!slim || slim != d->made_on || !slim->host_slim || slim->slim_gen != d->gen || slim->host_slim->count != d->d.count) {
    fail(HS_ERR_INVALID, "the index is not the one this diff was made on (or it has changed since)");
    return nullptr;
  }
  return slim->host_slim.get();
}

static hs_status hand_out(const std::string &bytes, void *buf, size_t cap, size_t *len) {
  if (len) *len = bytes.size();
  if (bytes.size() > cap || (!buf && !bytes.empty())) return fail(HS_ERR_CAPACITY, "buffer too small: " + std::to_string(bytes.size()) + " bytes needed");
  if (!bytes.empty()) memcpy(buf, bytes.data(), bytes.size());
  return HS_OK;
}

hs_status hs_slim_diff_stream(const hs_slim_diff *d, const hs_index *slim, void *buf, size_t cap, size_t *len) {
  const SlimGraph *g = diff_image(d, slim);
  if (!g) return HS_ERR_INVALID;
  return guarded([&] { return hand_out(diff_stream(*g, d->d), buf, cap, len); });
}

hs_status hs_slim_diff_next(hs_slim_diff *d, const hs_index *slim, size_t limit, int to_add, void *buf, size_t cap, size_t *len,
                            size_t *old_written, size_t *new_written, int *finished) {
  const SlimGraph *g = diff_image(d, slim);
  if (!g) return HS_ERR_INVALID;
  return guarded([&] {
    size_t io = d->d.ind_old, in = d->d.ind_new, ow = 0, nw = 0;
    std::string bytes(24, '\0');
    const uint32_t fin = gen_patch(*g, d->d, io, in, bytes, ow, nw, limit, to_add != 0);
    const uint64_t h[3] = {d->d.count, ow, nw};
    memcpy(&bytes[0], h, 24);
    hs_status st = hand_out(bytes, buf, cap, len);
    if (st != HS_OK) return st;   // the cursors have not moved
    d->d.ind_old = io; d->d.ind_new = in;
    if (old_written) *old_written = ow;
    if (new_written) *new_written = nw;
    if (finished) *finished = (int)fin;
    return HS_OK;
  });
}

void hs_slim_diff_free(hs_slim_diff *d) { delete d; }

hs_status hs_slim_index_save(const hs_index *slim, const char *path) {
  if (!slim || !path) return fail(HS_ERR_INVALID, "null argument");
  if (slim->info.kind != HS_KIND_SLIM || !slim->host_slim)
    return fail(HS_ERR_INVALID, "index holds no Slim host image to save: load a Slim index with max_elements > its element count");
  return guarded([&] {
    slim->host_slim->save(path);
    return HS_OK;
  });
}

hs_status hs_slim_convert_diff_files(const char *old_slim_path, const char *hnsw_path, int metric, size_t dim, int threshold_level,
                                     float top_degree_percent0, float top_degree_percent, size_t top_degree_M0, size_t low_degree_m0,
                                     size_t top_degree_M, size_t low_degree_m, int threads, const char *out_slim_path,
                                     const char *out_stream_path, hs_slim_diff **out) {
  if (out) *out = nullptr;
  if (!hnsw_path || !out_slim_path) return fail(HS_ERR_INVALID, "bad argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  return guarded([&] {
    VanillaGraph g;
    g.load(hnsw_path, (Metric)metric, dim);
    std::unique_ptr<hs_slim_diff> df(new hs_slim_diff());
    df->own.reset(new SlimGraph());
    SlimGraph &s = *df->own;
    std::unordered_map<uint64_t, uint32_t> lookup;
    if (old_slim_path) {
      s.load(old_slim_path, (Metric)metric, dim);
      if (s.maxM != g.maxM || s.maxM0 != g.maxM0) return fail(HS_ERR_INVALID, "convertFromHNSWWithDiff: the two indexes differ in maxM / maxM0");
      if (g.count < s.count) return fail(HS_ERR_INVALID, "convertFromHNSWWithDiff: the vanilla index holds fewer elements than the Slim index");
      for (size_t i = 0; i < s.count; i++) lookup[s.label((uint32_t)i)] = (uint32_t)i;
    } else {
      SlimParams hp;
      hp.threshold_level = threshold_level;
      s.take_header(g, hp);
      s.count = 0;
    }
    convert_diff(s, g, slim_params(0, top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0, top_degree_M, low_degree_m), threads,
                   lookup, df->d);
    s.save(out_slim_path);
    if (out_stream_path) {
      const std::string bytes = diff_stream(s, df->d);
      std::ofstream o(out_stream_path, std::ios::binary);
      if (!o.is_open()) throw std::runtime_error("Cannot open file");
      o.write(bytes.data(), bytes.size());
    }
    if (out) *out = df.release();
    return HS_OK;
  });
}
