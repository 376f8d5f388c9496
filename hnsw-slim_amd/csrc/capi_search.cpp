// capi_search.cpp -- the C ABI (include/hnsw_slim_amd.h): the graph search of a batch -- planned by search_plan.cpp, its arguments
// filled in here, each kernel launched through launch_search (engine.hpp) by the family and row format the plan names -- and the
// device, staged, zero-copy and raw entry points over it.
#include "capi_internal.hpp"

#include <cstdio>

// One launch group serves at most kMaxLaunchQueries queries: the per-query scratch in global memory (96 KiB each) is
// sized for that many, larger batches run as consecutive groups on the same stream (counters accumulate).
static constexpr size_t kMaxLaunchQueries = 32768;

// What the launch plan of a search on `ix` depends on (search_plan.hpp), knobs included.
static PlanInput plan_input(const hs_index *ix, size_t k, size_t nq, int mode, bool has_filter, bool want_raw) {
  PlanInput in{};
  const DevIndex &d = ix->dev;
  in.n = ix->info.n; in.dim = ix->info.dim;
  in.has_tile0 = d.tile0 != nullptr; in.has_uptile = d.uptile != nullptr;
  in.maxlevel = d.maxlevel; in.threshold_level = d.threshold_level; in.has_deleted = d.has_deleted; in.kind = d.kind;
  in.ef = ix->ef; in.k = k; in.nq = nq; in.mode = mode;
  in.user_cand_cap = ix->user_cand_cap; in.user_hash_slots = ix->user_hash_slots; in.grow_cand = ix->grow_cand; in.grow_hash = ix->grow_hash;
  in.exact_order = ix->exact_order; in.want_raw = want_raw; in.has_filter = has_filter;
  in.row_fmt = ix->row_fmt; in.f32_resident = ix->f32_resident; in.has_dup0 = ix->has_dup0;
  in.diag = diag();
  return in;
}

// An index without elements (cur_element_count == 0: hnswalg.h:1382, hnswalg_slim.h:2031-2032 return an empty result): no kernel
// is launched -- there is no row 0 and no tile 0 to read -- and every output the caller asked for is filled, in stream order, with
// what a query that found nothing gets: count 0, labels ~0, distances +inf, counters 0, an empty raw heap.
static hs_status empty_index_outputs(hs_index *ix, size_t nq, size_t k, uint32_t *l32, uint64_t *l64, float *dd, uint32_t *cnt,
                                     uint32_t *stats, uint32_t *rawsz, hipStream_t stream) {
  HIP_TRY(hipSetDevice(ix->device));
  if (l32) HIP_TRY(hipMemsetAsync(l32, 0xFF, nq * k * sizeof(uint32_t), stream));
  if (l64) HIP_TRY(hipMemsetAsync(l64, 0xFF, nq * k * sizeof(uint64_t), stream));
  if (dd) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)dd, 0x7F800000, nq * k, stream));   // +inf
  if (cnt) HIP_TRY(hipMemsetAsync(cnt, 0, nq * sizeof(uint32_t), stream));
  if (stats) HIP_TRY(hipMemsetAsync(stats, 0, nq * 4 * sizeof(uint32_t), stream));
  if (rawsz) HIP_TRY(hipMemsetAsync(rawsz, 0, nq * sizeof(uint32_t), stream));
  ix->last_kernel = "";
  return HS_OK;
}

static hs_status search_dev_group(hs_index *ix, const float *d_q, size_t nq, size_t k, int mode, uint32_t *l32,
                                  uint64_t *l64, float *dd, uint32_t *cnt, uint32_t *stats, Pair *raw, uint32_t *rawsz,
                                  hipStream_t stream, bool first_group, size_t nq_total, const FilterUse *fu = nullptr) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (k == 0) return fail(HS_ERR_INVALID, "k must be > 0");
  if (mode != HS_MODE_SLIM_IDS && mode != HS_MODE_PQ) return fail(HS_ERR_INVALID, "bad mode");
  if (ix->info.kind == HS_KIND_SLIMQ) return fail(HS_ERR_INVALID, "SlimQ index: use hs_slimq_search_batch");
  if (mode == HS_MODE_SLIM_IDS && ix->info.kind != HS_KIND_SLIM)
    return fail(HS_ERR_INVALID, "HS_MODE_SLIM_IDS needs a Slim index (searchKnn(q,k,tableint*) exists on HierarchicalNSWSlim only)");
  if (nq > 0x7FFFFFFFu) return fail(HS_ERR_INVALID, "nq too large");
  if (nq == 0) return HS_OK;
  if (ix->info.n == 0) return empty_index_outputs(ix, nq, k, l32, l64, dd, cnt, stats, rawsz, stream);
  SearchPlan p;
  const char *why = "";
  hs_status ps = plan_search(plan_input(ix, k, nq, mode, fu != nullptr, raw != nullptr), p, &why);
  if (ps != HS_OK) return fail(ps, why);
  HIP_TRY(hipSetDevice(ix->device));
  hs_index::StreamWs *w = ix->stream_ws(stream);
  HIP_TRY(w->status.ensure(nq));
  HIP_TRY(w->spill.ensure(nq * (size_t)p.spill_stride));
  // (status needs no clearing: pass 0 takes every query and writes each one's final status)
  // counters[0..12): per-pass overflow / hazard counts.  They are STICKY: they accumulate over the launch groups of a call and
  // over every call issued on this stream until hs_search_check reads and clears them, so a capacity failure in any batch of
  // a pipelined sequence is reported by the check that follows it.
  if (w->counters.n < 48) {
    HIP_TRY(w->counters.ensure(48));
    HIP_TRY(hipMemsetAsync(w->counters.p, 0, 48 * sizeof(uint32_t), stream));
  }
  if (first_group) w->last_nq += nq_total;   // queries since the last hs_search_check on this stream
  if (p.split) {
    HIP_TRY(w->entry.ensure(nq * 4));
    HIP_TRY(w->order.ensure(nq));
  }
  HIP_TRY(w->fb.ensure((size_t)kFbGrid * ((size_t)kFbCand * 2 + kFbSpill)));
  ix->last_kernel = p.name;

  SearchArgs a{};
  FilterArgs fa{};
  if (fu) fa = FilterArgs{fu->fs->bits.p, fu->d_of_query, w->counters.p + 12, (uint32_t)fu->fs->row_words, (uint32_t)fu->fs->nf};
  const FilterArgs *fap = fu ? &fa : nullptr;
  a.queries = d_q; a.nq = (uint32_t)nq; a.k = (uint32_t)k; a.ef = p.ef;
  a.mode = mode; a.mark_ep = (int32_t)p.mark_ep;
  a.out_labels32 = l32; a.out_labels64 = l64; a.out_dists = dd; a.out_counts = cnt; a.stats = stats;
  a.raw_top = raw; a.raw_size = rawsz; a.raw_stride = p.ef;
  a.status = w->status.p;
  a.spill = w->spill.p; a.spill_slots = kSpillSlots; a.spill_stride = p.spill_stride; a.cand2_cap = kCand2Cap;
  a.log_cap = p.log_cap; a.hop_cap = p.hop_cap;
  a.flat = p.flat;
  // pass 0: every query, one wavefront each, by the kernel the plan names (over the narrow copy of the rows where it says so)
  a.cand_cap = p.cand_cap; a.hash_slots = p.hash_slots; a.vis_bits = p.vis_bits; a.hash_fill_shift = p.hash_fill_shift;
  if (p.family == HS_PLAN_FLAT) { a.fl_nb = p.fl_nb; a.fl_mul = p.fl_mul; a.fl_sh = p.fl_sh; }
  a.counters = w->counters.p; a.pass_id = 0;
  a.select_mask = 1u << ST_TODO; a.grid = (uint32_t)nq;
  if (p.split) {   // descent / order / level-0 search (why: search_plan.cpp)
    a.entry = reinterpret_cast<uint4 *>(w->entry.p); a.order = w->order.p;
    a.phase = 1;
    HIP_TRY(launch_search(p.family, p.rows, ix->dev, a, ix->narrow.p, stream, fap));
    if (p.skip_order) a.order = nullptr;
    else HIP_TRY(launch_order(a.entry, w->order.p, (uint32_t)nq, stream));
    a.phase = 2;
    HIP_TRY(launch_search(p.family, p.rows, ix->dev, a, ix->narrow.p, stream, fap));
    a.phase = 0;
  } else {
    HIP_TRY(launch_search(p.family, p.rows, ix->dev, a, ix->narrow.p, stream, fap));
  }
  // Re-run pass (normally empty: a launch that scans the statuses and exits): the strict kernel, a few workgroups, candidate heap
  // and a large tier-2 visited set per workgroup in global memory (kFbGrid)
  a.select_mask = p.rerun_select_mask; a.grid = (uint32_t)std::min<size_t>(nq, kFbGrid);
  a.cand_cap = p.rerun_cand_cap; a.hash_slots = p.rerun_hash_slots; a.vis_bits = 0; a.hash_fill_shift = 0;
  a.fb_cand = w->fb.p; a.fb_spill = w->fb.p + (size_t)kFbGrid * kFbCand * 2; a.spill_slots = kFbSpill;
  a.counters = w->counters.p + 8; a.pass_id = 2;
  HIP_TRY(launch_search(HS_PLAN_STRICT, p.rerun_rows, ix->dev, a, ix->narrow.p, stream, fap));
  return HS_OK;
}

hs_status search_dev(hs_index *ix, const float *d_q, size_t nq, size_t k, int mode, uint32_t *l32, uint64_t *l64, float *dd,
                     uint32_t *cnt, uint32_t *stats, Pair *raw, uint32_t *rawsz, hipStream_t stream, const FilterUse *fu) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  if (nq > 0x7FFFFFFFu) return fail(HS_ERR_INVALID, "nq too large");
  const size_t dim = ix->info.dim, ef = std::max(ix->ef, k);
  for (size_t off = 0; off < nq || off == 0; off += kMaxLaunchQueries) {
    const size_t m = std::min(kMaxLaunchQueries, nq - off);
    // (a group's kernels index every per-query array from the group's first query: so the filter indices too)
    const FilterUse g{fu ? fu->fs : nullptr, fu ? fu->d_of_query + off : nullptr};
    hs_status s = search_dev_group(ix, d_q + off * dim, m, k, mode, l32 ? l32 + off * k : nullptr, l64 ? l64 + off * k : nullptr,
                                   dd ? dd + off * k : nullptr, cnt ? cnt + off : nullptr, stats ? stats + off * 4 : nullptr,
                                   raw ? raw + off * ef : nullptr, rawsz ? rawsz + off : nullptr, stream, off == 0, nq, fu ? &g : nullptr);
    if (s != HS_OK || nq == 0) return s;
  }
  return HS_OK;
}

hs_status hs_search_check(hs_index *ix, void *stream) {
  if (!ix) return fail(HS_ERR_INVALID, "null index");
  return guarded([&] {
    uint32_t c[13];   // [12]: queries of filter-set searches whose filter index was outside the set
    HIP_TRY(hipSetDevice(ix->device));
    hs_index::StreamWs *w = ix->stream_ws((hipStream_t)stream);
    if (!w->counters.p) {   // no kernel was launched on this stream; the padding outputs of an empty index may still be on their way
      HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      return HS_OK;
    }
    HIP_TRY(hipMemcpyAsync(c, w->counters.p, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(w->counters.p, 0, sizeof(c), (hipStream_t)stream));   // read and cleared: see search_dev_group
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    // learn the scratch sizes from the data: if more than 1% of a batch overflowed in the first passes,
    // later batches start with twice the visited-set slots / candidate capacity.
    const size_t nq = std::max<size_t>(w->last_nq, 1);
    w->last_nq = 0;
    if (diag().verbose) fprintf(stderr, "[hs check] nq %zu: visited overflow %u, candidate overflow %u, tie replays %u, visited-set spills %u | pass 2: %u %u | grow_hash %u grow_cand %u\n",
                         nq, c[0], c[1], c[2], c[3], c[8], c[9], ix->grow_hash, ix->grow_cand);
    if ((size_t)c[3] * 10 > nq && ix->grow_hash < 8 && !ix->user_hash_slots) ix->grow_hash++;
    if ((size_t)(c[1] + c[5]) * 100 > nq && ix->grow_cand < 4 && !ix->user_cand_cap) ix->grow_cand++;
    if (c[12] > 0)
      return fail(HS_ERR_INVALID, std::to_string(c[12]) + " queries named a filter index outside the filter set (count 0 returned for them)");
    if (ix->info.kind == HS_KIND_SLIMQ) {
      if (c[8] > 0) return fail(HS_ERR_CAPACITY, std::to_string(c[8]) + " queries expanded more nodes than the 64 KiB on-chip set holds");
      return HS_OK;
    }
    if (c[8] + c[9] > 0)
      return fail(HS_ERR_CAPACITY, std::to_string(c[8] + c[9]) + " queries exhausted even a whole CU's on-chip scratch");
    return HS_OK;
  });
}

// Parity/debug: the launch plan as a function of its inputs alone (no device), and those inputs for a live index
hs_status hs_debug_search_plan(const hs_plan_in *in, hs_plan_out *out) {
  if (!in || !out) return fail(HS_ERR_INVALID, "null argument");
  const char *why = "";
  hs_status s = plan_search(*in, *out, &why);
  return s == HS_OK ? s : fail(s, why);
}
hs_status hs_debug_plan_input(const hs_index *ix, size_t k, size_t nq, int has_filter, int want_raw, hs_plan_in *in) {
  if (!ix || !in) return fail(HS_ERR_INVALID, "null argument");
  *in = plan_input(ix, k, nq, HS_MODE_PQ, has_filter != 0, want_raw != 0);
  return HS_OK;
}

hs_status hs_debug_fast_shape(int metric, uint64_t dim, uint64_t ef, uint64_t k, int bare, hs_fast_shape *out) {
  if (!out) return fail(HS_ERR_INVALID, "null argument");
  if (metric_ok(metric) != HS_OK) return HS_ERR_INVALID;
  const uint64_t run_ef = std::max(ef, k);   // the search runs with max(ef, k)
  if (dim == 0 || dim > UINT32_MAX || run_ef == 0 || run_ef > 512) return fail(HS_ERR_INVALID, "no fast-kernel shape: dim = 0 or max(ef, k) outside 1..512");
  const FastShape s = fast_shape(metric, (uint32_t)dim, (uint32_t)run_ef, (uint32_t)k, bare != 0);
  out->d16 = s.d16; out->slots = s.slots; out->wb = s.wb;
  return HS_OK;
}

hs_status hs_debug_heap_ops(const uint32_t *ops, size_t n_ops, int wave_pop, uint32_t lds_slots, uint32_t *out_heap, uint32_t *out_pops,
                            uint32_t *out_n) {
  if (!ops || !out_heap || !out_pops || !out_n) return fail(HS_ERR_INVALID, "null argument");
  if (lds_slots < 2 || lds_slots > 8192 || (lds_slots & 1)) return fail(HS_ERR_INVALID, "lds_slots: even, 2..8192");
  return guarded([&] {
    DevBuf<uint32_t> d_ops, d_n;
    DevBuf<uint2> d_spill, d_heap, d_pops;
    HIP_TRY(d_ops.alloc(std::max<size_t>(3 * n_ops, 1)));
    HIP_TRY(d_n.alloc(2));
    HIP_TRY(d_spill.alloc(n_ops + 2));
    HIP_TRY(d_heap.alloc(n_ops + 2));
    HIP_TRY(d_pops.alloc(n_ops + 2));
    HIP_TRY(hipMemcpy(d_ops.p, ops, 3 * n_ops * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(flat_heap_ops(d_ops.p, (uint32_t)n_ops, d_spill.p, d_heap.p, d_pops.p, d_n.p, wave_pop, lds_slots, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_n, d_n.p, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_heap, d_heap.p, (size_t)out_n[0] * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_pops, d_pops.p, (size_t)out_n[1] * 8, hipMemcpyDeviceToHost));
    return HS_OK;
  });
}

hs_status hs_search_batch_dev(hs_index *ix, const float *d_queries, size_t nq, size_t k, int mode,
                              uint32_t *d_out_labels32, uint64_t *d_out_labels64, float *d_out_dists,
                              uint32_t *d_out_counts, uint32_t *d_stats, void *stream) {
  if (mode == HS_MODE_SLIM_IDS && !d_out_labels32) return fail(HS_ERR_INVALID, "out_labels32 required");
  if (mode == HS_MODE_PQ && (!d_out_labels64 || !d_out_dists || !d_out_counts)) return fail(HS_ERR_INVALID, "out_labels64/out_dists/out_counts required");
  return guarded([&] {
    return search_dev(ix, d_queries, nq, k, mode, d_out_labels32, d_out_labels64, d_out_dists, d_out_counts, d_stats, nullptr, nullptr, (hipStream_t)stream);
  });
}

// H2D of the queries, the search, D2H of the requested outputs: all enqueued on `stream`, no host synchronisation.  The
// staging buffers belong to (index, stream): a second call on the same stream reuses them in stream order.
// The device's address of a host buffer that is page-locked AND mapped into the device's address space (hipHostMalloc /
// hs_host_alloc, hipHostRegister with the mapped flag), or null: such a buffer needs no staging copy -- the kernels read the
// queries from it and write the results into it directly.
static void *mapped_device_pointer(const void *host) {
  if (!host) return nullptr;
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }   // pageable memory
  if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
  return at.devicePointer;
}
// A batch from page-locked host buffers, stream-ordered.  A SMALL batch (<= kZeroCopyQueryBytes of queries) is served in place:
// every wavefront stages its query once straight from the mapped host buffer and writes its few dozen result bytes straight
// into the caller's -- a small batch's copy-engine round trips (two per batch, each a cross-engine dependency in the stream)
// cost more than they move: 1250-query batches, 16 in flight, PCIe-inclusive 5.22 -> 5.65 M q/s.  Larger batches go through
// the staging copies (10k-query batches: 13.9 vs 13.6 M q/s in favour of staging).
static constexpr size_t kZeroCopyQueryBytes = 2u << 20;
hs_status search_async(hs_index *ix, const float *queries, size_t nq, size_t k, int mode, uint32_t *l32, uint64_t *l64, float *dd,
                       uint32_t *cnt, uint32_t *stats, hipStream_t st, const FilterUse *fu) {
  if (!ix || !queries) return fail(HS_ERR_INVALID, "null argument");
  if (k == 0) return fail(HS_ERR_INVALID, "k must be > 0");
  if (nq == 0) return HS_OK;
  HIP_TRY(hipSetDevice(ix->device));
  const size_t dim = ix->info.dim;
  hs_index::StreamWs *w = ix->stream_ws(st);
  const bool zero_copy_off = diag().zero_copy == HS_PLAN_ZERO_COPY_OFF;        // diagnostic A/B knobs
  const bool zero_copy_in_only = diag().zero_copy == HS_PLAN_ZERO_COPY_IN;   // (outputs staged)
  const bool ids = mode == HS_MODE_SLIM_IDS;
  const float *dq = nullptr;
  if (!zero_copy_off && nq * dim * sizeof(float) <= kZeroCopyQueryBytes) dq = static_cast<const float *>(mapped_device_pointer(queries));
  if (!dq) {
    HIP_TRY(w->aq.ensure(nq * dim));
    HIP_TRY(hipMemcpyAsync(w->aq.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, st));
    dq = w->aq.p;
  }
  // each output: the caller's buffer itself when the device can write it (small batches, as for the queries: with 10k-query
  // batches the staged path measured 2 % faster), else a device buffer + a copy back
  const bool small = nq * dim * sizeof(float) <= kZeroCopyQueryBytes;
  auto direct = [&](void *host) -> void * { return (zero_copy_off || zero_copy_in_only || !small) ? nullptr : mapped_device_pointer(host); };
  uint32_t *o32 = static_cast<uint32_t *>(direct(l32));
  uint64_t *o64 = static_cast<uint64_t *>(direct(l64));
  float *odd = static_cast<float *>(direct(dd));
  uint32_t *ocnt = static_cast<uint32_t *>(direct(cnt));
  uint32_t *ost = static_cast<uint32_t *>(direct(stats));
  const bool c32 = !o32 && (l32 || ids), c64 = !o64 && (l64 || !ids), cdd = !odd && (dd || !ids), ccnt = !ocnt, cst = !ost && stats;
  if (c32) { HIP_TRY(w->al32.ensure(nq * k)); o32 = w->al32.p; }
  if (c64) { HIP_TRY(w->al64.ensure(nq * k)); o64 = w->al64.p; }
  if (cdd) { HIP_TRY(w->adist.ensure(nq * k)); odd = w->adist.p; }
  if (ccnt) { HIP_TRY(w->acnt.ensure(nq)); ocnt = w->acnt.p; }
  if (cst) { HIP_TRY(w->astats.ensure(nq * 4)); ost = w->astats.p; }
  hs_status s = search_dev(ix, dq, nq, k, mode, o32, o64, odd, ocnt, ost, nullptr, nullptr, st, fu);
  if (s != HS_OK) return s;
  if (c32 && l32) HIP_TRY(hipMemcpyAsync(l32, w->al32.p, nq * k * 4, hipMemcpyDeviceToHost, st));
  if (c64 && l64) HIP_TRY(hipMemcpyAsync(l64, w->al64.p, nq * k * 8, hipMemcpyDeviceToHost, st));
  if (cdd && dd) HIP_TRY(hipMemcpyAsync(dd, w->adist.p, nq * k * 4, hipMemcpyDeviceToHost, st));
  if (ccnt && cnt) HIP_TRY(hipMemcpyAsync(cnt, w->acnt.p, nq * 4, hipMemcpyDeviceToHost, st));
  if (cst && stats) HIP_TRY(hipMemcpyAsync(stats, w->astats.p, nq * 16, hipMemcpyDeviceToHost, st));
  return HS_OK;
}

static hs_status search_host(hs_index *ix, const float *queries, size_t nq, size_t k, int mode, uint32_t *l32,
                             uint64_t *l64, float *dd, uint32_t *cnt, uint32_t *stats, float *raw_d, uint32_t *raw_i,
                             uint32_t *raw_sz) {
  if (!ix || !queries) return fail(HS_ERR_INVALID, "null argument");
  if (nq == 0) return HS_OK;
  const bool want_raw = raw_d || raw_i || raw_sz;
  if (!want_raw) {   // one stream-ordered sequence of copies and launches, one synchronisation
    hs_status s = search_async(ix, queries, nq, k, mode, l32, l64, dd, cnt, stats, nullptr);
    if (s != HS_OK) return s;
    return hs_search_check(ix, nullptr);
  }
  HIP_TRY(hipSetDevice(ix->device));
  const size_t dim = ix->info.dim;
  const size_t ef = std::max(ix->ef, k);
  HIP_TRY(ix->wq.ensure(nq * dim));
  HIP_TRY(ix->wstats.ensure(nq * 4));
  HIP_TRY(ix->wraw.ensure(nq * ef));
  HIP_TRY(ix->wrawsz.ensure(nq));
  hipStream_t st = nullptr;
  HIP_TRY(hipMemcpyAsync(ix->wq.p, queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_TRY(ix->wl32.ensure(nq * k));
  HIP_TRY(ix->wl64.ensure(nq * k));
  HIP_TRY(ix->wdist.ensure(nq * k));
  HIP_TRY(ix->wcnt.ensure(nq));
  hs_status s = search_dev(ix, ix->wq.p, nq, k, mode, ix->wl32.p, ix->wl64.p, ix->wdist.p, ix->wcnt.p, ix->wstats.p,
                           ix->wraw.p, ix->wrawsz.p, st);
  if (s != HS_OK) return s;
  s = hs_search_check(ix, st);
  if (s != HS_OK) return s;
  if (stats) HIP_TRY(hipMemcpy(stats, ix->wstats.p, nq * 16, hipMemcpyDeviceToHost));
  std::vector<Pair> raw(nq * ef);
  std::vector<uint32_t> sz(nq);
  HIP_TRY(hipMemcpy(raw.data(), ix->wraw.p, nq * ef * sizeof(Pair), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sz.data(), ix->wrawsz.p, nq * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < nq; i++) {
    if (raw_sz) raw_sz[i] = sz[i];
    for (size_t j = 0; j < ef; j++) {
      const bool v = j < sz[i];
      if (raw_d) raw_d[i * ef + j] = v ? raw[i * ef + j].d : 0.f;
      if (raw_i) raw_i[i * ef + j] = v ? raw[i * ef + j].id : 0u;
    }
  }
  return HS_OK;
}

hs_status hs_search_batch_async(hs_index *ix, const float *queries, size_t nq, size_t k, int mode, uint32_t *out_labels32,
                                uint64_t *out_labels64, float *out_dists, uint32_t *out_counts, uint32_t *stats, void *stream) {
  if (mode == HS_MODE_SLIM_IDS && !out_labels32) return fail(HS_ERR_INVALID, "out_labels32 required");
  if (mode == HS_MODE_PQ && (!out_labels64 || !out_dists || !out_counts)) return fail(HS_ERR_INVALID, "out_labels64/out_dists/out_counts required");
  if (mode != HS_MODE_SLIM_IDS && mode != HS_MODE_PQ) return fail(HS_ERR_INVALID, "bad mode");
  return guarded([&] { return search_async(ix, queries, nq, k, mode, out_labels32, out_labels64, out_dists, out_counts, stats, (hipStream_t)stream); });
}
void *hs_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}
void hs_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}
void *hs_host_device_pointer(const void *host) { return mapped_device_pointer(host); }

hs_status hs_search_batch(hs_index *ix, const float *queries, size_t nq, size_t k, int mode, uint32_t *out_labels32,
                          uint64_t *out_labels64, float *out_dists, uint32_t *out_counts, uint32_t *stats) {
  if (mode == HS_MODE_SLIM_IDS && !out_labels32) return fail(HS_ERR_INVALID, "out_labels32 required");
  if (mode == HS_MODE_PQ && (!out_labels64 || !out_dists || !out_counts)) return fail(HS_ERR_INVALID, "out_labels64/out_dists/out_counts required");
  return guarded([&] { return search_host(ix, queries, nq, k, mode, out_labels32, out_labels64, out_dists, out_counts, stats, nullptr, nullptr, nullptr); });
}

// The reference tests "!isMarkedDeleted(id) && (*isIdAllowed)(label)" together wherever a filter is consulted
// (hnswalg.h:348-349, 442-444; hnswalg_slim.h:578-580), and a filter forces the !bare_bone branch
// (hnswalg.h:1421, hnswalg_slim.h:1884).  So a filtered search is the ordinary search over an index whose
// delete-mark array is (deleted | !allowed) and whose has_deleted flag is set.
hs_status hs_search_batch_filtered(hs_index *ix, const float *queries, size_t nq, size_t k, const uint8_t *allowed,
                                   uint64_t *out_labels64, float *out_dists, uint32_t *out_counts, uint32_t *stats) {
  if (!ix || !allowed) return fail(HS_ERR_INVALID, "null argument");
  if (!out_labels64 || !out_dists || !out_counts) return fail(HS_ERR_INVALID, "out_labels64/out_dists/out_counts required");
  if (ix->info.kind == HS_KIND_SLIM && ix->info.threshold_level != 0)
    return fail(HS_ERR_UNSUPPORTED, "filtered search on a Slim index with threshold_level > 0 is not supported");
  return guarded([&] {
    HIP_TRY(hipSetDevice(ix->device));
    const size_t n = ix->info.n;
    std::vector<uint8_t> excl(std::max<size_t>(n, 1));
    for (size_t i = 0; i < n; i++) excl[i] = (ix->host_deleted[i] || !allowed[i]) ? 1 : 0;
    HIP_TRY(ix->wexcl.ensure(excl.size()));
    HIP_TRY(hipMemcpy(ix->wexcl.p, excl.data(), excl.size(), hipMemcpyHostToDevice));
    const Restore put_back([ix, saved = ix->dev] { ix->dev = saved; });
    ix->dev.deleted = ix->wexcl.p;
    ix->dev.has_deleted = 1;
    return search_host(ix, queries, nq, k, HS_MODE_PQ, nullptr, out_labels64, out_dists, out_counts, stats, nullptr, nullptr, nullptr);
  });
}

hs_status hs_search_batch_raw(hs_index *ix, const float *queries, size_t nq, size_t k, int mode, float *raw_dists,
                              uint32_t *raw_ids, uint32_t *raw_sizes, uint32_t *stats) {
  if (!raw_dists || !raw_ids || !raw_sizes) return fail(HS_ERR_INVALID, "raw outputs required");
  return guarded([&] { return search_host(ix, queries, nq, k, mode, nullptr, nullptr, nullptr, nullptr, stats, raw_dists, raw_ids, raw_sizes); });
}
