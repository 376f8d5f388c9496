// capi_filter.cpp -- the C ABI (include/hnsw_slim_amd.h): filter sets and the searches under them.
#include "capi_internal.hpp"

// ---- filter sets ---------------------------------------------------------------------------------------------------------
// nf bitmaps over the index's internal ids, resident on the index's device; a search names the set and one row per query, so
// queries under different filters share a launch and nothing is uploaded or rebuilt per call.  The rows hold the functor's
// answers only: the kernels test "marked deleted or bit clear" themselves (beam_search.hip), as the reference tests
// "!isMarkedDeleted(id) && (*isIdAllowed)(label)" (hnswalg.h:348-349, 442-444; hnswalg_slim.h:578-580).
size_t hs_filter_row_words(size_t n) { return ((n + 31) / 32 + 3) / 4 * 4; }

hs_status hs_filter_pack(const uint8_t *allowed, size_t n, size_t nf, uint32_t *out_words) {
  if ((!allowed && n * nf > 0) || !out_words) return fail(HS_ERR_INVALID, "null argument");
  const size_t rw = hs_filter_row_words(n);
  std::fill(out_words, out_words + nf * rw, 0u);
  for (size_t f = 0; f < nf; f++)
    for (size_t i = 0; i < n; i++)
      if (allowed[f * n + i]) out_words[f * rw + (i >> 5)] |= 1u << (i & 31);
  return HS_OK;
}

// The refusals of hs_search_batch_filtered, with its texts (the SlimQ one is search_dev_group's).
static hs_status filter_index_ok(const hs_index *ix) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (ix->info.kind == HS_KIND_SLIMQ) return fail(HS_ERR_INVALID, "SlimQ index: use hs_slimq_search_batch");
  if (ix->info.kind == HS_KIND_SLIM && ix->info.threshold_level != 0)
    return fail(HS_ERR_UNSUPPORTED, "filtered search on a Slim index with threshold_level > 0 is not supported");
  return HS_OK;
}

hs_status hs_filter_set_create(hs_index *ix, size_t nf, hs_filter_set **out) {
  if (!out) return fail(HS_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&] {
    hs_status s = filter_index_ok(ix);
    if (s != HS_OK) return s;
    if (nf == 0) return fail(HS_ERR_INVALID, "a filter set needs at least one filter");
    const size_t rw = hs_filter_row_words(ix->info.n);
    if (nf > 0xFFFFFFFFu || nf * rw > (size_t)1 << 40) return fail(HS_ERR_INVALID, "filter set too large");
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_ptr<hs_filter_set> fs(new hs_filter_set());
    fs->device = ix->device; fs->n = ix->info.n; fs->nf = nf; fs->row_words = rw;
    if (fs->bits.alloc(std::max<size_t>(nf * rw, 1)) != hipSuccess) return fail(HS_ERR_NOMEM, "Not enough memory: filter set of " + std::to_string(nf * rw * 4) + " bytes");
    HIP_TRY(hipMemset(fs->bits.p, 0, std::max<size_t>(nf * rw, 1) * 4));
    *out = fs.release();
    return HS_OK;
  });
}

void hs_filter_set_free(hs_filter_set *fs) {
  if (!fs) return;
  (void)hipSetDevice(fs->device);
  delete fs;
}

static hs_status filter_rows_ok(const hs_filter_set *fs, size_t first, size_t count, const void *src) {
  if (!fs || (!src && count > 0)) return fail(HS_ERR_INVALID, "null argument");
  if (first > fs->nf || count > fs->nf - first)
    return fail(HS_ERR_INVALID, "filter rows [" + std::to_string(first) + ", " + std::to_string(first + count) + ") outside a set of " + std::to_string(fs->nf));
  return HS_OK;
}

hs_status hs_filter_set_write_dev(hs_filter_set *fs, size_t first, size_t count, const uint8_t *d_allowed, void *stream) {
  return guarded([&] {
    hs_status s = filter_rows_ok(fs, first, count, d_allowed);
    if (s != HS_OK || count == 0) return s;
    HIP_TRY(hipSetDevice(fs->device));
    HIP_TRY(launch_filter_pack(d_allowed, fs->bits.p + first * fs->row_words, (uint32_t)fs->n, (uint32_t)count, (uint32_t)fs->row_words, (hipStream_t)stream));
    return HS_OK;
  });
}

// Host bytes go through a device buffer of at most kFilterStageBytes (one row, if a row is longer) and are packed there.
static constexpr size_t kFilterStageBytes = 8u << 20;
hs_status hs_filter_set_write(hs_filter_set *fs, size_t first, size_t count, const uint8_t *allowed) {
  return guarded([&] {
    hs_status s = filter_rows_ok(fs, first, count, allowed);
    if (s != HS_OK || count == 0) return s;
    HIP_TRY(hipSetDevice(fs->device));
    if (fs->n == 0) return HS_OK;
    const size_t per = std::max<size_t>(kFilterStageBytes / fs->n, 1);
    HIP_TRY(fs->stage.ensure(std::min(per, count) * fs->n));
    for (size_t r0 = 0; r0 < count; r0 += per) {
      const size_t m = std::min(per, count - r0);
      HIP_TRY(hipMemcpyAsync(fs->stage.p, allowed + r0 * fs->n, m * fs->n, hipMemcpyHostToDevice, nullptr));
      HIP_TRY(launch_filter_pack(fs->stage.p, fs->bits.p + (first + r0) * fs->row_words, (uint32_t)fs->n, (uint32_t)m, (uint32_t)fs->row_words, nullptr));
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    return HS_OK;
  });
}

hs_status hs_filter_set_write_bits(hs_filter_set *fs, size_t first, size_t count, const uint32_t *words) {
  return guarded([&] {
    hs_status s = filter_rows_ok(fs, first, count, words);
    if (s != HS_OK || count == 0) return s;
    HIP_TRY(hipSetDevice(fs->device));
    HIP_TRY(hipMemcpy(fs->bits.p + first * fs->row_words, words, count * fs->row_words * 4, hipMemcpyHostToDevice));
    return HS_OK;
  });
}

hs_status hs_filter_set_read(hs_filter_set *fs, size_t f, uint8_t *out_allowed) {
  if (!fs || !out_allowed) return fail(HS_ERR_INVALID, "null argument");
  return guarded([&] {
    if (f >= fs->nf) return fail(HS_ERR_INVALID, "filter " + std::to_string(f) + " outside a set of " + std::to_string(fs->nf));
    if (fs->n == 0) return HS_OK;
    HIP_TRY(hipSetDevice(fs->device));
    HIP_TRY(fs->unpacked.ensure(fs->n));
    HIP_TRY(launch_filter_unpack(fs->bits.p + f * fs->row_words, fs->unpacked.p, (uint32_t)fs->n, nullptr));
    HIP_TRY(hipMemcpy(out_allowed, fs->unpacked.p, fs->n, hipMemcpyDeviceToHost));
    return HS_OK;
  });
}

hs_status hs_filter_set_info(const hs_filter_set *fs, uint64_t *nf, uint64_t *n, uint64_t *row_words, uint64_t *device_bytes) {
  if (!fs) return fail(HS_ERR_INVALID, "null argument");
  if (nf) *nf = fs->nf;
  if (n) *n = fs->n;
  if (row_words) *row_words = fs->row_words;
  if (device_bytes) *device_bytes = (uint64_t)fs->nf * fs->row_words * 4;
  return HS_OK;
}

// Everything a search under `fs` is refused for on the host, before anything is launched.
static hs_status filter_use_ok(const hs_index *ix, const hs_filter_set *fs) {
  hs_status s = filter_index_ok(ix);
  if (s != HS_OK) return s;
  if (!fs) return fail(HS_ERR_INVALID, "null filter set");
  if (fs->device != ix->device)
    return fail(HS_ERR_INVALID, "the filter set lives on device " + std::to_string(fs->device) + ", the index on device " + std::to_string(ix->device));
  if (fs->n != ix->info.n)
    return fail(HS_ERR_INVALID, "the filter set was created for " + std::to_string(fs->n) + " elements, the index holds " + std::to_string(ix->info.n));
  return HS_OK;
}

hs_status hs_search_batch_filter_set_dev(hs_index *ix, const hs_filter_set *fs, const float *d_queries, size_t nq, size_t k,
                                         const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                         uint32_t *d_out_counts, uint32_t *d_stats, void *stream) {
  return guarded([&] {
    hs_status s = filter_use_ok(ix, fs);
    if (s != HS_OK) return s;
    if (!d_queries || !d_filter_of_query) return fail(HS_ERR_INVALID, "null argument");
    if (!d_out_labels64 || !d_out_dists || !d_out_counts) return fail(HS_ERR_INVALID, "out_labels64/out_dists/out_counts required");
    const FilterUse fu{fs, d_filter_of_query};
    return search_dev(ix, d_queries, nq, k, HS_MODE_PQ, nullptr, d_out_labels64, d_out_dists, d_out_counts, d_stats, nullptr, nullptr,
                      (hipStream_t)stream, &fu);
  });
}

hs_status hs_search_batch_filter_set(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, size_t k,
                                     const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts,
                                     uint32_t *stats) {
  return guarded([&] {
    hs_status s = filter_use_ok(ix, fs);
    if (s != HS_OK) return s;
    if (!queries || !filter_of_query) return fail(HS_ERR_INVALID, "null argument");
    if (!out_labels64 || !out_dists || !out_counts) return fail(HS_ERR_INVALID, "out_labels64/out_dists/out_counts required");
    for (size_t i = 0; i < nq; i++)
      if (filter_of_query[i] >= fs->nf)
        return fail(HS_ERR_INVALID, "query " + std::to_string(i) + " names filter " + std::to_string(filter_of_query[i]) + " of a set of " + std::to_string(fs->nf));
    if (nq == 0) return HS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    hs_index::StreamWs *w = ix->stream_ws(nullptr);
    HIP_TRY(w->afoq.ensure(nq));
    HIP_TRY(hipMemcpyAsync(w->afoq.p, filter_of_query, nq * 4, hipMemcpyHostToDevice, nullptr));
    const FilterUse fu{fs, w->afoq.p};
    s = search_async(ix, queries, nq, k, HS_MODE_PQ, nullptr, out_labels64, out_dists, out_counts, stats, nullptr, &fu);
    if (s != HS_OK) return s;
    return hs_search_check(ix, nullptr);
  });
}
