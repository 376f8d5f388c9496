// capi_index.cpp -- the C ABI (include/hnsw_slim_amd.h): an index's life on the device -- upload, the loaders, patching, the
// setters and getters, narrow rows and fp32 residency.
#include "capi_internal.hpp"

#include <cstdio>

static constexpr const char *kLoadNomem = "Not enough memory: loadIndex failed to allocate";

template <typename T>
static hipError_t upload_cap(DevBuf<T> &b, const std::vector<T> &v, size_t cap) {
  hipError_t e = b.alloc(std::max<size_t>(std::max(v.size(), cap), 1));
  if (e != hipSuccess) return e;
  return v.empty() ? hipSuccess : hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// ---- narrow rows ------------------------------------------------------------------------------------------------------------
template <typename T>
static size_t first_unfit(const float *x, size_t count) {
  for (size_t i = 0; i < count; i++)
    if (!narrow_fits<T>(x[i])) return i;
  return count;
}
size_t first_unfit(const float *x, size_t count, int fmt) {
  return fmt == ROWS_U8 ? first_unfit<uint8_t>(x, count) : fmt == ROWS_F16 ? first_unfit<_Float16>(x, count) : count;
}
static const char *row_format_name(int fmt) { return fmt == ROWS_U8 ? "HS_ROWS_U8" : fmt == ROWS_F16 ? "HS_ROWS_F16" : "HS_ROWS_F32"; }
std::string unfit_message(size_t row, size_t comp, float v, int fmt) {
  char val[64];
  snprintf(val, sizeof val, "%.9g", (double)v);
  return "row " + std::to_string(row) + " holds " + val + " (component " + std::to_string(comp) + "), which " + row_format_name(fmt) +
         " cannot represent exactly";
}
// bytes of the narrow copy: one value of the format per value of `vec`'s row capacity (documented in the header)
static size_t narrow_copy_bytes(const hs_index *ix, int fmt) {
  return std::max<size_t>(ix->cap_rows, ix->info.n) * ix->info.dim * narrow_width(fmt);
}
// Fills `out` (allocated here) with the narrow copy of all rows of ix->vec.  HS_ERR_UNSUPPORTED, `out` released, when a value does not fit.
hs_status build_narrow(hs_index *ix, int fmt, DevBuf<uint8_t> &out) {
  const size_t n = ix->info.n, dim = ix->info.dim;
  HIP_TRY(out.alloc(std::max<size_t>(narrow_copy_bytes(ix, fmt), 16)));
  HIP_TRY(ix->narrow_bad.ensure(1));
  uint32_t bad = 0xFFFFFFFFu;
  HIP_TRY(hipMemcpy(ix->narrow_bad.p, &bad, 4, hipMemcpyHostToDevice));
  HIP_TRY(launch_narrow_convert(ix->vec.p, out.p, fmt, 0, (uint32_t)n, (uint32_t)dim, ix->narrow_bad.p, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&bad, ix->narrow_bad.p, 4, hipMemcpyDeviceToHost));
  if (bad != 0xFFFFFFFFu) {
    out.release();
    std::vector<float> row(dim);
    HIP_TRY(hipMemcpy(row.data(), ix->vec.p + (size_t)bad * dim, dim * 4, hipMemcpyDeviceToHost));
    const size_t j = std::min(first_unfit(row.data(), dim, fmt), dim - 1);
    return fail(HS_ERR_UNSUPPORTED, unfit_message(bad, j, row[j], fmt));
  }
  return HS_OK;
}

// Host-side conversion (hs_rows_to_narrow, hs_index_load_narrow, an upload without fp32 rows): rows[n x dim] into
// the lane-major layout of the device copy, row by row while the rows fit.  Returns the first row that holds an unrepresentable
// value (nothing is written from that row on), n when there is none.
template <typename T>
static size_t rows_to_narrow_t(const float *rows, size_t n, size_t dim, T *out) {
  for (size_t r = 0; r < n; r++) {
    const float *x = rows + r * dim;
    if (first_unfit<T>(x, dim) < dim) return r;
    T *o = out + r * dim;
    for (size_t j = 0; j < dim; j++) o[narrow_slot((uint32_t)j, (uint32_t)dim)] = narrow_cast<T>(x[j]);
  }
  return n;
}
static size_t rows_to_narrow_host(const float *rows, size_t n, size_t dim, int fmt, void *out) {
  return fmt == ROWS_U8 ? rows_to_narrow_t<uint8_t>(rows, n, dim, static_cast<uint8_t *>(out))
                        : rows_to_narrow_t<_Float16>(rows, n, dim, static_cast<_Float16 *>(out));
}
// The narrow copy of an index WITHOUT resident fp32 rows, (re)built from host rows: allocated for `cap` rows, converted on the
// host and uploaded in chunks of at most kNarrowStageBytes -- the fp32 array never exists on the device.
static constexpr size_t kNarrowStageBytes = 64u << 20;
static hs_status upload_narrow_from_host(hs_index *ix, const float *rows, size_t n, size_t dim, size_t cap) {
  const int fmt = ix->row_fmt;
  const size_t w = narrow_width(fmt), row_bytes = dim * w;
  DevBuf<uint8_t> fresh;
  HIP_TRY(fresh.alloc(std::max<size_t>(cap * row_bytes, 16)));
  const size_t per = std::max<size_t>(kNarrowStageBytes / std::max<size_t>(row_bytes, 1), 1);
  std::vector<uint8_t> stage(std::min(per, std::max<size_t>(n, 1)) * row_bytes);
  for (size_t r0 = 0; r0 < n; r0 += per) {
    const size_t m = std::min(per, n - r0);
    const size_t bad = rows_to_narrow_host(rows + r0 * dim, m, dim, fmt, stage.data());
    if (bad < m) {
      const float *x = rows + (r0 + bad) * dim;
      const size_t j = std::min(first_unfit(x, dim, fmt), dim - 1);
      return fail(HS_ERR_UNSUPPORTED, unfit_message(r0 + bad, j, x[j], fmt));
    }
    HIP_TRY(hipMemcpy(fresh.p + r0 * row_bytes, stage.data(), m * row_bytes, hipMemcpyHostToDevice));
  }
  ix->narrow.release();
  std::swap(ix->narrow.p, fresh.p);
  std::swap(ix->narrow.n, fresh.n);
  return HS_OK;
}

const char *hs_last_error(void) { return g_err.c_str(); }

int hs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// the graph-structure arrays that are small next to the vectors and tiles: uploaded whole (also after every call that changed
// nodes, write_changed), and with them what the host keeps of `p`: the label / mark mirrors, the mark counters, hs_info
hs_status upload_small(hs_index *ix, const PackedIndex &p) {
  HIP_TRY(ix->row_ptr0.upload(p.row_ptr0));
  HIP_TRY(ix->cols.upload(p.cols));
  HIP_TRY(upload_cap(ix->up_base, p.up_base, ix->cap_rows));
  HIP_TRY(ix->up_ptr.upload(p.up_ptr));
  uint32_t up_stride = 0;
  const std::vector<uint32_t> ut = build_uptile(p, up_stride);
  if (up_stride) HIP_TRY(ix->uptile.upload(ut));
  DevIndex &d = ix->dev;
  d.row_ptr0 = ix->row_ptr0.p; d.cols = ix->cols.p; d.up_base = ix->up_base.p; d.up_ptr = ix->up_ptr.p;
  d.uptile = up_stride ? reinterpret_cast<const uint2 *>(ix->uptile.p) : nullptr; d.up_stride = up_stride;
  d.ep_base = ep_base_of(p);
  d.n = (uint32_t)p.n; d.dim = (uint32_t)p.dim; d.maxlevel = p.maxlevel; d.threshold_level = p.threshold_level;
  d.enterpoint = p.enterpoint; d.kind = p.kind; d.metric = p.metric;
  ix->host_labels = p.labels;
  ix->host_deleted = p.deleted;
  set_delete_marks(ix, p.deleted.size() - (size_t)std::count(p.deleted.begin(), p.deleted.end(), 0), p.has_deleted);
  ix->has_dup0 = p.repeats_id0();
  hs_info &i = ix->info;
  i.n = p.n; i.dim = p.dim; i.kind = p.kind; i.metric = p.metric; i.maxlevel = p.maxlevel;
  i.threshold_level = p.threshold_level; i.enterpoint = p.enterpoint;
  i.n_edges = p.cols.size(); i.max_degree0 = p.max_deg0; i.index_size = p.index_size;
  ix->base_bytes = p.row_values() * 4 + (p.row_ptr0.size() + p.cols.size() + p.up_base.size() + p.up_ptr.size()) * 4 +
                   p.labels.size() * 8 + p.deleted.size() + (size_t)p.n * ix->dev.tile_stride * 4;
  refresh_device_bytes(ix);
  return HS_OK;
}

hs_status upload(hs_index *ix, const PackedIndex &p) {
  HIP_TRY(hipSetDevice(ix->device));
  const size_t cap = std::max(ix->cap_rows, p.n);
  if (ix->f32_resident) {
    HIP_TRY(upload_cap(ix->vec, p.vec, cap * p.dim));
  } else {   // the rows go to the device in the narrow format only
    ix->vec.release();
    hs_status ns = upload_narrow_from_host(ix, p.vec.data(), p.n, p.dim, cap);
    if (ns != HS_OK) return ns;
  }
  // level-0 adjacency tiles (host_tiles.hpp)
  const uint32_t stride = tile_stride_for(p.max_deg0);
  if (stride) {
    HIP_TRY(upload_cap(ix->tile0, build_tile0(p, stride), cap * stride));
  }
  HIP_TRY(upload_cap(ix->labels, p.labels, cap));
  HIP_TRY(upload_cap(ix->deleted, p.deleted, cap));
  DevIndex &d = ix->dev;
  d.vec = ix->vec.p; d.labels = ix->labels.p; d.deleted = ix->deleted.p;
  d.tile0 = stride ? ix->tile0.p : nullptr; d.tile_stride = stride;
  return upload_small(ix, p);
}

// The end of every loader: the device test, a new index, `prepare` on it, the upload of `p`.
template <class Prepare>
static hs_status upload_new(const PackedIndex &p, int device, hs_index **out, Prepare &&prepare) {
  if (device_ok(device, true) != HS_OK) return HS_ERR_DEVICE;
  std::unique_ptr<hs_index> ix(new hs_index());
  ix->device = device;
  prepare(*ix);
  const hs_status s = upload(ix.get(), p);
  if (s != HS_OK) return s;
  *out = ix.release();
  return HS_OK;
}

// narrow_fmt != ROWS_F32 (hs_index_load_narrow): the index starts without fp32 rows, its rows uploaded in that format only.
// Throws what the loaders throw: the three exported loaders run it inside their guard.
static hs_status load_from(const BinSource &src, int kind, int metric, size_t dim, size_t max_elements, int device, hs_index **out,
                           int narrow_fmt = ROWS_F32) {
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  PackedIndex p;
  std::unique_ptr<SlimGraph> keep_slim;
  std::unique_ptr<VanillaGraph> keep_vanilla;
  if (kind == HS_KIND_HNSW) {
    std::unique_ptr<VanillaGraph> g(new VanillaGraph());
    g->load(src, (Metric)metric, dim, max_elements);
    p.from_vanilla(*g);
    if (max_elements > g->count) keep_vanilla = std::move(g);   // room for addPoint (hs_index_add_points), a file for hs_index_save
  } else if (kind == HS_KIND_SLIM) {
    std::unique_ptr<SlimGraph> g(new SlimGraph());
    g->load(src, (Metric)metric, dim);
    p.from_slim(*g);
    if (max_elements > g->count) keep_slim = std::move(g);   // room for patchFromStream (hnswalg_slim.h:760, 784)
  } else if (kind == HS_KIND_SLIMQ) {
    return load_slimq(src, metric, dim, device, out);
  } else {
    return fail(HS_ERR_INVALID, "bad index kind");
  }
  // only now: a hostile file is refused as such (the loaders ran index_check.hpp) on a machine without a device too
  return upload_new(p, device, out, [&](hs_index &ix) {
    if (keep_slim) { ix.cap_rows = max_elements; ix.host_slim = std::move(keep_slim); }
    if (keep_vanilla) { ix.cap_rows = max_elements; ix.host_vanilla = std::move(keep_vanilla); }
    if (narrow_fmt != ROWS_F32) { ix.row_fmt = narrow_fmt; ix.f32_resident = false; }
  });
}

// patchFromStream(std::istream &in, bool to_add) (hnswalg_slim.h:2292-2340) on a device-resident index.  Stream, as the
// reference's server assembles it (hnsw_slim_server_patch.cc:280-290 after its `finished` word; records by genPatch,
// hnswalg_slim.h:1427-1476):  u64 cur_element_count, u64 changed_old_cnt, u64 changed_new_cnt, then per changed node
//   u32 id | old node: 8 bytes {i32 level, u32 total_neighbor}; new node: 16 bytes {level, total, u64 label} |
//   u32 neighborsSize | the neighbour blob | new node and to_add: data_size bytes of vector.
// The host image takes the records exactly as the reference's does; on the device the changed nodes go through write_changed:
// the new nodes with their row as the image holds it (the stream's vector with to_add, zeros without), the old nodes as list-only
// records (a patch never carries their rows, so the resident row already equals the image's).
// As in the reference the stream carries no enter point / max level: they stay what they were.
hs_status hs_index_patch(hs_index *ix, const void *bytes, size_t len, int to_add) {
  if (!ix || !bytes) return fail(HS_ERR_INVALID, "null argument");
  if (!ix->host_slim) return fail(HS_ERR_INVALID, "index not patchable: load a Slim index with max_elements > its element count");
  SlimGraph &g = *ix->host_slim;
  const size_t spe = g.size_per_el, dim = g.dim;
  std::vector<uint32_t> changed, added;
  size_t new_count = 0;
  return guarded("Not enough memory: patchFromStream failed to allocate linklist", [&] {
    BinReader r(BinSource(bytes, len));
    new_count = r.pod<uint64_t>();
    const uint64_t n_old = r.pod<uint64_t>(), n_new = r.pod<uint64_t>();
    if (new_count > ix->cap_rows || new_count < g.count || n_old + n_new > (1ull << 32)) return fail(HS_ERR_CAPACITY, "patch exceeds max_elements");
    // stage the records first: a refused stream leaves the index untouched -- the device arrays AND the host image, byte for byte
    struct Rec { uint32_t id; char head[16]; std::vector<char> blob; std::vector<char> vec; bool is_new; };
    std::vector<Rec> recs((size_t)(n_old + n_new));
    for (size_t i = 0; i < recs.size(); i++) {
      Rec &rc = recs[i];
      rc.is_new = i >= n_old;
      rc.id = r.pod<uint32_t>();
      r.bytes(rc.head, rc.is_new ? 16 : 8);
      const uint32_t nsz = r.pod<uint32_t>();
      int32_t level; uint32_t total;
      memcpy(&level, rc.head, 4); memcpy(&total, rc.head + 4, 4);
      if (rc.id >= new_count || level < 0 || level > 64 || (nsz != 2 * (uint64_t)level + 4 * (uint64_t)total && !(nsz == 0 && total == 0)))
        return fail(HS_ERR_CORRUPT, kCorruptText);
      rc.blob.resize(nsz);
      if (nsz) r.bytes(rc.blob.data(), nsz);
      if (to_add && rc.is_new) { rc.vec.resize(dim * 4); r.bytes(rc.vec.data(), dim * 4); }
    }
    // an index with narrow rows takes only rows its format represents (hs_index_set_row_format): checked on the staged records
    if (ix->row_fmt != ROWS_F32)
      for (const Rec &rc : recs) {
        if (rc.vec.empty()) continue;
        std::vector<float> v(dim);
        memcpy(v.data(), rc.vec.data(), dim * 4);
        const size_t j = first_unfit(v.data(), dim, ix->row_fmt);
        if (j < dim) return fail(HS_ERR_UNSUPPORTED, "patch refused: " + unfit_message(rc.id, j, v[j], ix->row_fmt));
      }
    // The image as it would stand after the records, checked whole (index_check.hpp) before a byte of it changes: a staged record
    // answers for its node (the last one of an id, as the writes below), the image for every other, the zeroed element for a node
    // beyond the old count that has no record.  One pass over the lists, as the repacking below is.
    {
      static const std::vector<char> none;
      std::vector<int64_t> rec_of(new_count, -1);
      for (size_t i = 0; i < recs.size(); i++) rec_of[recs[i].id] = (int64_t)i;
      auto head = [&](size_t i, size_t at) -> uint32_t {
        uint32_t v = 0;
        if (rec_of[i] >= 0) memcpy(&v, recs[(size_t)rec_of[i]].head + at, 4);
        else if (i < g.count) memcpy(&v, g.el((uint32_t)i) + at, 4);
        return v;
      };
      auto blob_of = [&](size_t i) -> const std::vector<char> & {
        if (rec_of[i] >= 0) return head(i, 4) == 0 ? none : recs[(size_t)rec_of[i]].blob;
        return i < g.count ? g.blobs[i] : none;
      };
      if (check_chal(new_count, g.enterpoint, g.maxlevel, g.threshold_level, [&](size_t i) { return (int)(int32_t)head(i, 0); },
                     [&](size_t i) { return (size_t)head(i, 4); }, blob_of, /*unlisted_ok=*/true))   // (a chunk of a diff: P7's exception)
        return fail(HS_ERR_CORRUPT, kCorruptText);
    }
    g.elements.resize(new_count * spe, 0);
    g.blobs.resize(new_count);
    for (Rec &rc : recs) {
      char *e = g.elements.data() + (size_t)rc.id * spe;
      memcpy(e, rc.head, rc.is_new ? 16 : 8);
      uint32_t total; memcpy(&total, e + 4, 4);
      g.blobs[rc.id] = (rc.blob.empty() || total == 0) ? std::vector<char>() : std::move(rc.blob);
      if (!rc.vec.empty()) memcpy(e + 24, rc.vec.data(), dim * 4);
      (rc.is_new ? added : changed).push_back(rc.id);
    }
    g.count = new_count;
    PackedIndex p;
    p.from_slim(g, false);
    return write_changed(ix, p, [&g](uint32_t i) { return g.vec(i); }, changed, added);
  });
}

// An index the host has already parsed: node i owns levels[i] + 1 consecutive neighbour lists (level 0 first),
// list t = list_ids[list_ptr[t] .. list_ptr[t+1]).  kind selects the searchKnn semantics (HS_KIND_HNSW / HS_KIND_SLIM).
hs_status hs_index_from_host_arrays(int kind, int metric, size_t n, size_t dim, const float *vectors, const uint64_t *labels,
                                    const uint8_t *deleted, const int32_t *levels, const uint64_t *list_ptr, const uint32_t *list_ids,
                                    uint32_t enterpoint, int32_t maxlevel, int32_t threshold_level, int device, hs_index **out) {
  if (!out || (n && (!vectors || !levels || !list_ptr || !list_ids))) return fail(HS_ERR_INVALID, "null argument");
  if (kind != HS_KIND_HNSW && kind != HS_KIND_SLIM) return fail(HS_ERR_INVALID, "bad index kind");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  if (dim == 0) return fail(HS_ERR_INVALID, "dim must be > 0");
  if (n && enterpoint >= n) return fail(HS_ERR_INVALID, "enter point out of range");
  return guarded([&] {
    PackedIndex p;
    {   // the preconditions of index_check.hpp on the caller's arrays, before anything is packed from them
      std::vector<size_t> first(n);
      size_t t = 0;
      for (size_t i = 0; i < n; i++) {
        if (levels[i] < 0 || levels[i] > maxlevel) return fail(HS_ERR_INVALID, "level out of range");
        first[i] = t;
        t += (size_t)levels[i] + 1;
      }
      auto level_of = [&](size_t i) { return (int)levels[i]; };
      const char *bad = check_entry(n, enterpoint, maxlevel, kind == HS_KIND_SLIM ? threshold_level : 0, true, level_of);
      if (!bad)
        bad = check_lists(n, level_of, [](size_t) { return true; }, [&](size_t i, int l, const uint32_t *&ids, size_t &cnt) {
          const uint64_t s0 = list_ptr[first[i] + l], e0 = list_ptr[first[i] + l + 1];
          if (e0 < s0) return false;
          ids = list_ids + s0;
          cnt = e0 - s0;
          return true;
        });
      if (bad) return fail(HS_ERR_INVALID, bad);
    }
    p.kind = kind; p.metric = (Metric)metric; p.n = n; p.dim = dim;
    p.maxlevel = maxlevel; p.threshold_level = kind == HS_KIND_SLIM ? threshold_level : 0; p.enterpoint = enterpoint;
    p.vec.assign(vectors, vectors + n * dim);
    p.labels.resize(n);
    p.deleted.assign(n, 0);
    size_t nd = 0;
    for (size_t i = 0; i < n; i++) {
      p.labels[i] = labels ? labels[i] : (uint64_t)i;
      if (deleted) { p.deleted[i] = deleted[i] ? 1 : 0; nd += p.deleted[i]; }
    }
    p.has_deleted = nd > 0;
    p.row_ptr0.assign(n + 1, 0);
    p.up_base.assign(n, PackedIndex::NONE);
    size_t t = 0;
    std::vector<size_t> first(n);
    for (size_t i = 0; i < n; i++) {   // level-0 lists first (CSR rows), then the upper levels appended to cols
      if (levels[i] < 0 || levels[i] > maxlevel) return fail(HS_ERR_INVALID, "level out of range");
      first[i] = t;
      const uint64_t s0 = list_ptr[t], e0 = list_ptr[t + 1];
      if (e0 < s0) return fail(HS_ERR_INVALID, "list_ptr not monotone");
      for (uint64_t j = s0; j < e0; j++) {
        if (list_ids[j] >= n) return fail(HS_ERR_INVALID, "neighbour id out of range");
        p.cols.push_back(list_ids[j]);
      }
      p.max_deg0 = std::max<size_t>(p.max_deg0, e0 - s0);
      p.row_ptr0[i + 1] = (uint32_t)p.cols.size();
      t += (size_t)levels[i] + 1;
    }
    for (size_t i = 0; i < n; i++) {
      if (levels[i] <= 0) continue;
      p.up_base[i] = (uint32_t)p.up_ptr.size();
      for (int l = 1; l <= levels[i]; l++) {
        p.up_ptr.push_back((uint32_t)p.cols.size());
        const uint64_t s0 = list_ptr[first[i] + l], e0 = list_ptr[first[i] + l + 1];
        if (e0 < s0) return fail(HS_ERR_INVALID, "list_ptr not monotone");
        for (uint64_t j = s0; j < e0; j++) {
          if (list_ids[j] >= n) return fail(HS_ERR_INVALID, "neighbour id out of range");
          p.cols.push_back(list_ids[j]);
        }
      }
      p.up_ptr.push_back((uint32_t)p.cols.size());
    }
    if (p.cols.size() >= PackedIndex::NONE) return fail(HS_ERR_INVALID, "adjacency too large for 32-bit CSR offsets");
    p.index_size = 16 * n + 4 * p.cols.size();
    return upload_new(p, device, out, [](hs_index &) {});
  });
}

hs_status hs_index_load(const char *path, int kind, int metric, size_t dim, size_t max_elements, int device,
                        hs_index **out) {
  if (!path || !out) return fail(HS_ERR_INVALID, "null argument");
  return guarded(kLoadNomem, [&] { return load_from(BinSource(path), kind, metric, dim, max_elements, device, out); });
}

hs_status hs_index_load_mem(const void *bytes, size_t len, int kind, int metric, size_t dim, size_t max_elements, int device,
                            hs_index **out) {
  if (!bytes || !out) return fail(HS_ERR_INVALID, "null argument");
  return guarded(kLoadNomem, [&] { return load_from(BinSource(bytes, len), kind, metric, dim, max_elements, device, out); });
}

void hs_index_free(hs_index *ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  delete ix;
}

hs_status hs_set_ef(hs_index *ix, size_t ef) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (ef != ix->ef) ix->grow_hash = ix->grow_cand = 0;   // what hs_search_check learned about the scratch shares held for the old ef
  ix->ef = ef;
  return HS_OK;
}
hs_status hs_set_capacity(hs_index *ix, uint32_t cand_cap, uint32_t hash_slots) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  ix->user_cand_cap = cand_cap;
  ix->user_hash_slots = hash_slots;
  return HS_OK;
}
hs_status hs_set_exact_order(hs_index *ix, int on) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  ix->exact_order = on != 0;
  return HS_OK;
}
const char *hs_last_kernel(const hs_index *ix) { return ix ? ix->last_kernel : ""; }
hs_status hs_index_info(const hs_index *ix, hs_info *out) {
  if (!ix || !out) return fail(HS_ERR_INVALID, "null argument");
  *out = ix->info;
  return HS_OK;
}

hs_status hs_index_set_row_format(hs_index *ix, int format) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (format != ROWS_F32 && format != ROWS_F16 && format != ROWS_U8) return fail(HS_ERR_INVALID, "bad row format");
  if (ix->info.kind == HS_KIND_SLIMQ) return fail(HS_ERR_UNSUPPORTED, "narrow rows: a SlimQ index has no flat-kernel rows");
  return guarded([&] {
    if (format != ROWS_F32 && (ix->info.dim & 15) != 0)
      return fail(HS_ERR_UNSUPPORTED, "narrow rows need dim % 16 == 0 (the flat kernel does not serve dim " + std::to_string(ix->info.dim) + ")");
    if (format == ix->row_fmt) return HS_OK;
    if (!ix->f32_resident)   // every other format is converted from the fp32 rows
      return fail(HS_ERR_INVALID, "the index holds no fp32 rows: restore the fp32 rows first (hs_index_set_f32_resident(ix, 1))");
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());   // no search may be in flight on this index while its rows change
    DevBuf<uint8_t> fresh;
    if (format != ROWS_F32) {
      hs_status s = build_narrow(ix, format, fresh);   // into a buffer of its own: a refusal leaves the index exactly as it was
      if (s != HS_OK) return s;
    }
    ix->narrow.release();
    std::swap(ix->narrow.p, fresh.p);
    std::swap(ix->narrow.n, fresh.n);
    ix->row_fmt = format;
    refresh_device_bytes(ix);
    return HS_OK;
  });
}
int hs_index_row_format(const hs_index *ix) { return ix ? ix->row_fmt : ROWS_F32; }

hs_status hs_index_set_f32_resident(hs_index *ix, int on) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (!on && ix->row_fmt == ROWS_F32) return fail(HS_ERR_INVALID, "the fp32 rows are the only rows of this index: hs_index_set_row_format first");
  if ((on != 0) == ix->f32_resident) return HS_OK;
  return guarded([&] {
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());   // no search may be in flight on this index while its rows change
    const size_t n = ix->info.n, dim = ix->info.dim;
    if (on) {
      HIP_TRY(ix->vec.alloc(std::max<size_t>(std::max<size_t>(ix->cap_rows, n) * dim, 1)));
      HIP_TRY(launch_narrow_widen(ix->narrow.p, ix->vec.p, ix->row_fmt, 0, (uint32_t)n, (uint32_t)dim, nullptr));
      HIP_TRY(hipDeviceSynchronize());
      ix->dev.vec = ix->vec.p;
    } else {
      ix->vec.release();
      ix->dev.vec = nullptr;
    }
    ix->f32_resident = on != 0;
    refresh_device_bytes(ix);
    return HS_OK;
  });
}
int hs_index_f32_resident(const hs_index *ix) { return ix ? (ix->f32_resident ? 1 : 0) : 1; }
hs_status hs_rows_representable(const float *rows, size_t n, size_t dim, int format, uint64_t *first_bad) {
  if (!first_bad || (n && dim && !rows)) return fail(HS_ERR_INVALID, "null argument");
  if (format != ROWS_F32 && format != ROWS_F16 && format != ROWS_U8) return fail(HS_ERR_INVALID, "bad row format");
  *first_bad = dim ? first_unfit(rows, n * dim, format) / dim : n;
  return HS_OK;
}

hs_status hs_rows_to_narrow(const float *rows, size_t n, size_t dim, int format, void *out, uint64_t *first_bad) {
  if (!first_bad || (n && dim && (!rows || !out))) return fail(HS_ERR_INVALID, "null argument");
  if (format != ROWS_F16 && format != ROWS_U8) return fail(HS_ERR_INVALID, "bad row format (HS_ROWS_U8 or HS_ROWS_F16)");
  if ((dim & 15) != 0) return fail(HS_ERR_UNSUPPORTED, "narrow rows need dim % 16 == 0");
  *first_bad = dim ? rows_to_narrow_host(rows, n, dim, format, out) : n;
  return HS_OK;
}

hs_status hs_index_load_narrow(const char *path, int kind, int metric, size_t dim, size_t max_elements, int device, int format,
                               hs_index **out) {
  if (!path || !out) return fail(HS_ERR_INVALID, "null argument");
  *out = nullptr;
  if (format != ROWS_F16 && format != ROWS_U8) return fail(HS_ERR_INVALID, "bad row format (HS_ROWS_U8 or HS_ROWS_F16)");
  if (kind == HS_KIND_SLIMQ) return fail(HS_ERR_UNSUPPORTED, "narrow rows: a SlimQ index has no flat-kernel rows");
  return guarded(kLoadNomem, [&] {
    if ((dim & 15) != 0) return fail(HS_ERR_UNSUPPORTED, "narrow rows need dim % 16 == 0 (the flat kernel does not serve dim " + std::to_string(dim) + ")");
    return load_from(BinSource(path), kind, metric, dim, max_elements, device, out, format);
  });
}

hs_status hs_labels(const hs_index *ix, uint64_t *out_labels) {
  if (!ix || !out_labels) return fail(HS_ERR_INVALID, "null argument");
  std::copy(ix->host_labels.begin(), ix->host_labels.end(), out_labels);
  return HS_OK;
}
