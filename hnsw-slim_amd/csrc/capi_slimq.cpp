// capi_slimq.cpp -- the C ABI (include/hnsw_slim_amd.h): HNSW-SlimQ -- loading, search, trace and preparation entries, and the
// host-side RaBitQ exports.
#include "capi_internal.hpp"

#include "rabitq_est.hpp"
#include "rabitq_host.hpp"
#include "slimq_tiles.hpp"

static uint32_t next_pow2(uint32_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// The packed graph of a SlimQ file image: CSR of the CHAL blobs, labels, the header's fields (no rows: they come with setDataset).
static void pack_slimq(PackedIndex &p, const SlimQGraph &q) {
  p.kind = HS_KIND_SLIMQ; p.metric = (Metric)q.metric; p.n = q.count; p.dim = q.dim;
  p.maxlevel = q.maxlevel; p.threshold_level = q.threshold_level; p.enterpoint = q.enterpoint;
  p.index_size = q.count * 20;   // HierarchicalNSWSlimQ::indexSize() (hnswalg_slimq.h:2047-2057): 20 B per element + blobs
  for (size_t i = 0; i < q.count; i++) p.index_size += 2 * (size_t)q.level[i] + 4 * (size_t)q.total(i);
  p.labels = q.label;
  p.deleted.assign(q.count, 0);
  p.pack_chal([&](size_t i) { return (int)q.level[i]; }, [&](size_t i) { return (size_t)q.total(i); },
              [&](size_t i) -> const std::vector<char> & { return q.blobs[i]; });
}

// HierarchicalNSWSlimQ::loadIndex (hnswalg_slimq.h:1218-1313): the file parse, then the one way to residency.  (This and
// slimq_make_resident throw what the loaders throw: the exported entries that reach them guard.)
hs_status load_slimq(const BinSource &src, int metric, size_t dim, int device, hs_index **out) {
  std::unique_ptr<SlimQGraph> q(new SlimQGraph());
  q->load(src, metric, dim);
  return slimq_make_resident(std::move(q), device, out);
}

// graph -> CSR/tiles (upload), element records -> 16-byte header {f_add, f_rescale, cluster id, f_error} + sign code, the fused
// level-0 and upper-level tiles (slimq_tiles.hip, layout in slimq_engine.hpp / slimq_tiles.hpp), rotated centroids and rotator flips
// as they are.  The record fields go up as they lie in the image and are freed once the kernels have read them.
hs_status slimq_make_resident(std::unique_ptr<SlimQGraph> qp, int device, hs_index **out) {
  if (!qp || !out) return fail(HS_ERR_INVALID, "null argument");
  const auto t0 = std::chrono::steady_clock::now();
  const SlimQGraph &q = *qp;
  PackedIndex p;
  if (q.rot.trunc < 64) return fail(HS_ERR_UNSUPPORTED, "SlimQ supports dim >= 64");
  if (q.check()) return fail(HS_ERR_CORRUPT, kCorruptText);   // index_check.hpp: the image may come from a conversion, not a file
  for (uint32_t c : q.cluster)   // g_add[cluster] in the kernel's estimate (slimq_search.hip)
    if (c >= q.num_cluster) return fail(HS_ERR_CORRUPT, kCorruptText);
  pack_slimq(p, q);
  if (q.count > 0xFFFFFFF0ull || p.up_ptr.size() > 0xFFFFFFF0ull) return fail(HS_ERR_UNSUPPORTED, "SlimQ index too large");
  // only now: a hostile image is refused as such on a machine without a device too (a negative device is no device either)
  if (device_ok(device < 0 ? std::numeric_limits<int>::max() : device, true) != HS_OK) return HS_ERR_DEVICE;
  std::unique_ptr<hs_index> ix(new hs_index());
  ix->device = device;
  hs_status s = upload(ix.get(), p);
  if (s != HS_OK) return s;
  const uint32_t n = (uint32_t)q.count, rw = slimq_rec_words(q.padded);
  // fused level-0 tiles (see slimq_engine.hpp): 288 GB of HBM buys one dependent access per expansion.
  // HS_SLIMQ_FUSED=0 (debug/test knob) keeps the CSR + record-array layout that wide graphs (degree > 64) fall back to.
  const bool fused = diag_from_env().slimq_fused != 0;   // (read at every load, not once per process)
  const uint32_t stride = fused ? ix->dev.tile_stride : 0;
  // fused upper-level tiles: slot up_base[i] + l - 1 holds level l of node i
  const uint32_t up_stride = fused ? slimq_up_stride(p.up_ptr) : 0;
  const size_t rec_words = (size_t)n * rw, ft_words = (size_t)n * stride * rw, ut_words = up_stride ? p.up_ptr.size() * (size_t)up_stride * (rw + 4) : 0;
  {
    DevBuf<float> d_fac;
    DevBuf<uint32_t> d_cl;
    DevBuf<uint64_t> d_code;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t e = d_fac.upload(q.factors);
    if (e == hipSuccess) e = d_cl.upload(q.cluster);
    if (e == hipSuccess) e = d_code.upload(q.code);
    if (e == hipSuccess) e = ix->q_rec.alloc(std::max<size_t>(rec_words, 1));
    if (e == hipSuccess && up_stride) e = ix->q_uptile.alloc(ut_words);
    if (e == hipSuccess && stride) e = ix->q_ftile.alloc(std::max<size_t>(ft_words, 1));
    if (e == hipSuccess) e = ix->q_cent.upload(q.centroids);
    if (e == hipSuccess) e = ix->q_flips.upload(q.rot.flip);
    if (e == hipSuccess) e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, nullptr);
    if (e == hipSuccess) e = launch_slimq_records(d_fac.p, d_cl.p, d_code.p, n, (uint32_t)q.padded, ix->q_rec.p, nullptr);
    if (e == hipSuccess && stride) e = launch_slimq_ftile(ix->q_rec.p, ix->tile0.p, n, stride, rw, ix->q_ftile.p, nullptr);
    if (e == hipSuccess && up_stride)
      e = launch_slimq_uptile(ix->q_rec.p, ix->up_ptr.p, (uint32_t)p.up_ptr.size(), ix->cols.p, ix->up_base.p, n, up_stride, rw, ix->q_uptile.p, nullptr);
    if (e == hipSuccess) e = hipEventRecord(ev1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);   // the staging arrays are freed below: the kernels must have read them
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (e != hipSuccess) return fail(HS_ERR_DEVICE, std::string("SlimQ upload: ") + hipGetErrorString(e));
    ix->tile_kernel_ms = ms;
  }
  DevSlimQ &d = ix->sq;
  d.rec = ix->q_rec.p; d.ftile = stride ? ix->q_ftile.p : nullptr; d.raw = nullptr;
  d.uptile = up_stride ? ix->q_uptile.p : nullptr; d.up_stride = up_stride;
  d.ep_base = ep_base_of(p); d.cent = ix->q_cent.p; d.flips = ix->q_flips.p;
  d.rec_words = rw; d.padded = (uint32_t)q.padded; d.trunc = (uint32_t)q.rot.trunc; d.ncl = (uint32_t)q.num_cluster;
  d.fht_scale = q.rot.fac;
  d.t_const = rq_default_tconst(q.padded, 1);
  ix->base_bytes += (rec_words + ft_words + ut_words) * 4 + q.centroids.size() * 4 + q.rot.flip.size();
  refresh_device_bytes(ix.get());
  ix->host_slimq = std::move(qp);
  ix->resident_ms = ms_since(t0);
  *out = ix.release();
  return HS_OK;
}

// ---- HNSW-SlimQ ------------------------------------------------------------------------------------------------
hs_status slimq_set_dataset_pitched(hs_index *ix, const void *rows, size_t pitch, size_t n, size_t dim) {
  if (!ix || !rows) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind != HS_KIND_SLIMQ) return fail(HS_ERR_INVALID, "not a SlimQ index");
  if (n != ix->info.n || dim != ix->info.dim) return fail(HS_ERR_INVALID, "dataset shape does not match the index");
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(ix->vec.alloc(std::max<size_t>(n * dim, 1)));
  if (pitch == dim * sizeof(float)) HIP_TRY(hipMemcpy(ix->vec.p, rows, n * dim * sizeof(float), hipMemcpyHostToDevice));
  else if (n) HIP_TRY(hipMemcpy2D(ix->vec.p, dim * sizeof(float), rows, pitch, dim * sizeof(float), n, hipMemcpyHostToDevice));
  ix->dev.vec = ix->vec.p;
  ix->sq.raw = ix->vec.p;
  ix->has_dataset = true;
  ix->base_bytes += n * dim * 4;
  refresh_device_bytes(ix);
  return HS_OK;
}
hs_status hs_slimq_set_dataset(hs_index *ix, const float *base, size_t n, size_t dim) {
  return guarded([&] { return slimq_set_dataset_pitched(ix, base, dim * sizeof(float), n, dim); });
}
hs_status hs_slimq_set_tconst(hs_index *ix, double t_const) {
  if (!ix || !(t_const > 0)) return fail(HS_ERR_INVALID, "bad argument");
  if (ix->info.kind != HS_KIND_SLIMQ) return fail(HS_ERR_INVALID, "not a SlimQ index");
  ix->sq.t_const = t_const;
  return HS_OK;
}
double hs_slimq_get_tconst(const hs_index *ix) { return ix && ix->info.kind == HS_KIND_SLIMQ ? ix->sq.t_const : 0.0; }

static constexpr uint32_t kSlimQMaxHash = 16384;  // largest expanded-node set in LDS (64 KiB)
static constexpr uint32_t kSlimQFbHash = 65536, kSlimQFbGrid = 64;  // second pass: the set in global memory, 256 KiB per workgroup

hs_status hs_slimq_search_batch_dev(hs_index *ix, const float *d_queries, size_t nq, size_t k, uint64_t *d_out_labels,
                                    float *d_out_dists, uint32_t *d_out_counts, uint32_t *d_stats, void *stream_) {
  if (!ix || !d_queries || !d_out_labels || !d_out_dists || !d_out_counts) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind != HS_KIND_SLIMQ) return fail(HS_ERR_INVALID, "not a SlimQ index");
  if (!ix->has_dataset) return fail(HS_ERR_INVALID, "hs_slimq_set_dataset() first (setDataset, hnswalg_slimq.h:303)");
  if (k == 0 || k > 1024) return fail(HS_ERR_INVALID, "k must be in 1..1024");
  if (!slimq_supported((uint32_t)ix->ef)) return fail(HS_ERR_UNSUPPORTED, "SlimQ supports 1 <= ef <= 1024");
  if (nq > 0x7FFFFFFFu) return fail(HS_ERR_INVALID, "nq too large");
  if (nq == 0) return HS_OK;
  return guarded([&] {
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(ix->device));
    hs_index::StreamWs *w = ix->stream_ws(stream);
    HIP_TRY(w->status.ensure(nq));
    if (w->counters.n < 48) {   // sticky until hs_search_check clears them (see search_dev_group); status: written for every query by the first pass
      HIP_TRY(w->counters.ensure(48));
      HIP_TRY(hipMemsetAsync(w->counters.p, 0, 48 * sizeof(uint32_t), stream));
    }
    w->last_nq += nq;
    SlimQArgs a{};
    a.queries = d_queries; a.nq = (uint32_t)nq; a.k = (uint32_t)k; a.pool_cap = (uint32_t)ix->ef;
    // expansions per query stay below ~ef on real graphs; 75 % fill of 4 ef slots leaves 3x headroom, and a query
    // that still outgrows it is redone with the 64 KiB set
    a.hash_slots = ix->user_hash_slots ? next_pow2(ix->user_hash_slots) : next_pow2(std::max<uint32_t>(256, 4 * (uint32_t)ix->ef));
    a.hash_slots = std::min(a.hash_slots, kSlimQMaxHash);
    a.out_labels = d_out_labels; a.out_dists = d_out_dists; a.out_counts = d_out_counts; a.stats = d_stats;
    a.status = w->status.p;
    a.trace = ix->trace_ptr; a.trace_cap = ix->trace_cap;
    const uint32_t pw = slimq_prep_words(ix->sq.ncl, ix->sq.padded);
    HIP_TRY(w->prep.ensure(nq * (size_t)pw));
    ix->last_kernel = "hs::slimq_kernel";
    HIP_TRY(launch_slimq_prep(ix->sq, (uint32_t)ix->info.dim, ix->info.metric, d_queries, (uint32_t)nq, w->prep.p, nullptr, stream));
    a.prep = w->prep.p;
    a.select_mask = 1u << ST_TODO; a.grid = (uint32_t)nq; a.counters = w->counters.p;
    if (!a.trace && split_launch(diag(), nq)) {
      // descent / order by the entry's estimated distance, farthest first / level-0 search (see search_dev_group)
      HIP_TRY(w->entry.ensure(nq * 4));
      HIP_TRY(w->order.ensure(nq));
      a.entry = reinterpret_cast<uint4 *>(w->entry.p); a.order = w->order.p;
      a.phase = 1;
      HIP_TRY(launch_slimq(ix->dev, ix->sq, a, stream));
      HIP_TRY(launch_order(a.entry, w->order.p, (uint32_t)nq, stream));
      a.phase = 2;
      HIP_TRY(launch_slimq(ix->dev, ix->sq, a, stream));
      a.phase = 0;
    } else {
      HIP_TRY(launch_slimq(ix->dev, ix->sq, a, stream));
    }
    {
      HIP_TRY(w->fb.ensure((size_t)kSlimQFbGrid * kSlimQFbHash));
      a.select_mask = 1u << ST_OVERFLOW; a.grid = (uint32_t)std::min<size_t>(nq, kSlimQFbGrid); a.hash_slots = kSlimQFbHash; a.fb_tab = w->fb.p;
      a.counters = w->counters.p + 8;
      HIP_TRY(launch_slimq(ix->dev, ix->sq, a, stream));
    }
    return HS_OK;
  });
}

// Parity/debug entry: the query preparation as the kernel computed it (rotation, split query, centroid table).
hs_status hs_slimq_prepare_debug(hs_index *ix, const float *queries, size_t nq, float *out) {
  if (!ix || !queries || !out) return fail(HS_ERR_INVALID, "null argument");
  if (ix->info.kind != HS_KIND_SLIMQ) return fail(HS_ERR_INVALID, "not a SlimQ index");
  return guarded([&] {
    if (nq == 0) return HS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    const size_t P = ix->sq.padded, ncl = ix->sq.ncl, npl = P / 8, row = P + 3 + ncl + npl;
    const uint32_t pw = slimq_prep_words(ix->sq.ncl, ix->sq.padded);
    DevBuf<float> dq, dy;
    DevBuf<uint32_t> dp;
    HIP_TRY(dq.alloc(nq * ix->info.dim)); HIP_TRY(dy.alloc(nq * P)); HIP_TRY(dp.alloc(nq * (size_t)pw));
    HIP_TRY(hipMemcpy(dq.p, queries, nq * ix->info.dim * 4, hipMemcpyHostToDevice));
    HIP_TRY(launch_slimq_prep(ix->sq, (uint32_t)ix->info.dim, ix->info.metric, dq.p, (uint32_t)nq, dp.p, dy.p, nullptr));
    std::vector<float> y(nq * P);
    std::vector<uint32_t> pr(nq * (size_t)pw);
    HIP_TRY(hipMemcpy(y.data(), dy.p, y.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pr.data(), dp.p, pr.size() * 4, hipMemcpyDeviceToHost));
    const size_t poff = (4 + ncl + 1) & ~size_t(1);
    for (size_t i = 0; i < nq; i++) {
      float *o = out + i * row;
      const uint32_t *r = &pr[i * pw];
      memcpy(o, &y[i * P], P * 4);
      memcpy(o + P, r, 12);
      memcpy(o + P + 3, r + 4, ncl * 4);
      memcpy(o + P + 3 + ncl, r + poff, npl * 4);
    }
    return HS_OK;
  });
}

// Parity/debug entry: the sequence of SearchBuffer pops of each query (node id, bit 31 = already expanded).
hs_status hs_slimq_trace(hs_index *ix, const float *queries, size_t nq, size_t k, uint32_t *out_trace, size_t trace_cap,
                         uint32_t *stats) {
  if (!ix || !queries || !out_trace || trace_cap == 0) return fail(HS_ERR_INVALID, "null argument");
  return guarded([&] {
    if (nq == 0) return HS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    DevBuf<float> dq, dd;
    DevBuf<uint64_t> dl;
    DevBuf<uint32_t> dc, ds, dt;
    HIP_TRY(dq.alloc(nq * ix->info.dim)); HIP_TRY(dl.alloc(nq * k)); HIP_TRY(dd.alloc(nq * k)); HIP_TRY(dc.alloc(nq));
    HIP_TRY(ds.alloc(nq * 4)); HIP_TRY(dt.alloc(nq * trace_cap));
    HIP_TRY(hipMemcpy(dq.p, queries, nq * ix->info.dim * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dt.p, 0xFF, nq * trace_cap * 4));
    ix->trace_ptr = dt.p; ix->trace_cap = (uint32_t)trace_cap;
    hs_status s = hs_slimq_search_batch_dev(ix, dq.p, nq, k, dl.p, dd.p, dc.p, ds.p, nullptr);
    ix->trace_ptr = nullptr; ix->trace_cap = 0;
    if (s != HS_OK) return s;
    s = hs_search_check(ix, nullptr);
    if (s != HS_OK) return s;
    HIP_TRY(hipMemcpy(out_trace, dt.p, nq * trace_cap * 4, hipMemcpyDeviceToHost));
    if (stats) HIP_TRY(hipMemcpy(stats, ds.p, nq * 16, hipMemcpyDeviceToHost));
    return HS_OK;
  });
}

hs_status hs_slimq_search_batch(hs_index *ix, const float *queries, size_t nq, size_t k, uint64_t *out_labels,
                                float *out_dists, uint32_t *out_counts, uint32_t *stats) {
  if (!ix || !queries || !out_labels) return fail(HS_ERR_INVALID, "null argument");
  return guarded([&] {
    if (nq == 0) return HS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    const size_t dim = ix->info.dim;
    HIP_TRY(ix->wq.ensure(nq * dim));
    HIP_TRY(ix->wl64.ensure(nq * k));
    HIP_TRY(ix->wdist.ensure(nq * k));
    HIP_TRY(ix->wcnt.ensure(nq));
    HIP_TRY(ix->wstats.ensure(nq * 4));
    hipStream_t st = nullptr;
    HIP_TRY(hipMemcpyAsync(ix->wq.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, st));
    hs_status s = hs_slimq_search_batch_dev(ix, ix->wq.p, nq, k, ix->wl64.p, ix->wdist.p, ix->wcnt.p, ix->wstats.p, st);
    if (s != HS_OK) return s;
    s = hs_search_check(ix, st);
    if (s != HS_OK) return s;
    HIP_TRY(hipMemcpy(out_labels, ix->wl64.p, nq * k * 8, hipMemcpyDeviceToHost));
    if (out_dists) HIP_TRY(hipMemcpy(out_dists, ix->wdist.p, nq * k * 4, hipMemcpyDeviceToHost));
    if (out_counts) HIP_TRY(hipMemcpy(out_counts, ix->wcnt.p, nq * 4, hipMemcpyDeviceToHost));
    if (stats) HIP_TRY(hipMemcpy(stats, ix->wstats.p, nq * 16, hipMemcpyDeviceToHost));
    return HS_OK;
  });
}

double hs_rabitq_default_tconst(size_t padded_dim, uint64_t seed) {
  if (padded_dim == 0 || padded_dim % 64) return 0.0;
  double t = 0.0;   // (its answer to a bad argument, also when the sample vector cannot be allocated)
  (void)guarded([&] {
    t = rq_default_tconst(padded_dim, seed);
    return HS_OK;
  });
  return t;
}

hs_status hs_rabitq_rotate(size_t dim, const uint8_t *flips, const float *in, size_t n, float *out) {
  if (!flips || !in || !out || dim == 0) return fail(HS_ERR_INVALID, "bad argument");
  return guarded([&] {
    Rotator r;
    r.init(dim);
    if (r.trunc < 64 || r.trunc > 2048) return fail(HS_ERR_UNSUPPORTED, "rotator supports 64 <= dim < 4096");
    std::copy(flips, flips + r.flip.size(), r.flip.begin());
    for (size_t i = 0; i < n; i++) r.rotate(in + i * dim, out + i * r.padded);
    return HS_OK;
  });
}
hs_status hs_rabitq_quantize_data(size_t padded, int metric, const float *rotated, size_t n, const float *centroid,
                                  uint64_t *codes, float *factors) {
  if (!rotated || !centroid || !codes || !factors || padded % 64) return fail(HS_ERR_INVALID, "bad argument");
  return guarded([&] {
    for (size_t i = 0; i < n; i++) rq_quantize_data(rotated + i * padded, centroid, padded, metric, codes + i * padded / 64, factors + i * 3);
    return HS_OK;
  });
}
hs_status hs_rabitq_prepare_query(size_t padded, double t_const, const float *rotated_q, size_t n, float *out3,
                                  uint64_t *bins) {
  if (!rotated_q || !out3 || !bins || padded % 64) return fail(HS_ERR_INVALID, "bad argument");
  return guarded([&] {
    RqQuery q;
    for (size_t i = 0; i < n; i++) {
      rq_prepare_query(rotated_q + i * padded, padded, t_const, q);
      out3[i * 3] = q.delta; out3[i * 3 + 1] = q.vl; out3[i * 3 + 2] = q.k1xsumq;
      std::copy(q.bins.begin(), q.bins.end(), bins + i * padded / 64 * 4);
    }
    return HS_OK;
  });
}
hs_status hs_rabitq_estimate(size_t padded, const uint64_t *codes, const float *factors, size_t nd, const float *q3,
                             const uint64_t *bins, const float *g_add, const float *g_error, size_t nq, float *out) {
  if (!codes || !factors || !q3 || !bins || !g_add || !g_error || !out) return fail(HS_ERR_INVALID, "bad argument");
  const uint32_t nblk = (uint32_t)(padded / 64);
  for (size_t i = 0; i < nq; i++)
    for (size_t j = 0; j < nd; j++) {
      const float ip = rq_ip_x0_qr(codes + j * nblk, bins + i * nblk * 4, nblk, q3[i * 3], q3[i * 3 + 1]);
      const float est = rq_est_dist(factors[j * 3], g_add[i], factors[j * 3 + 1], ip, q3[i * 3 + 2]);
      float *o = out + (i * nd + j) * 3;
      o[0] = ip; o[1] = est; o[2] = est - factors[j * 3 + 2] * g_error[i];
    }
  return HS_OK;
}
