// capi_queue.cpp -- the C ABI (include/hnsw_slim_amd.h): the search queue.  Small submissions from any thread are coalesced into
// one ordinary search launch group per flush: one gather kernel, search_dev as every other entry calls it (same plan, same
// kernels, same bits), one scatter kernel (segment_copy.hip).  The bookkeeping is search_queue.hpp's; this file is its HIP backend.
//
// A slot is what a launch in flight owns on the device: a stream, the launch's arrays (queries in, results out) and the event
// that marks its end.  A slab is what a launch owns in page-locked host memory from its first submission on: the rows of its
// host submissions, their results on the way back, and the segment table the copy kernels read.  The kernels address the slab
// through its device mapping, so a launch is gather + search + scatter on one stream and no copy-engine transfer at all.
#include "capi_internal.hpp"
#include "segment_copy.hpp"

#include <cstdlib>

namespace {

// Searches planned and checked through a queue read and write the index's learnt scratch sizes (hs_index::grow_*): one at a time,
// for every queue of the process.
std::mutex g_plan_mu;

struct Pinned {   // page-locked, device-mapped host memory
  void *h = nullptr, *d = nullptr;
  hipError_t alloc(size_t bytes) {
    hipError_t e = hipHostMalloc(&h, std::max<size_t>(bytes, 16), hipHostMallocDefault);
    if (e != hipSuccess) { h = nullptr; return e; }
    return hipHostGetDevicePointer(&d, h, 0);
  }
  void release() {
    if (h) (void)hipHostFree(h);
    h = d = nullptr;
  }
  template <typename T> T *host() const { return static_cast<T *>(h); }
  template <typename T> T *dev() const { return static_cast<T *>(d); }
};

struct Slot {
  hipStream_t st = nullptr;
  hipEvent_t done = nullptr;
  DevBuf<float> q, dd;
  DevBuf<uint32_t> foq, l32, cnt, stats;
  DevBuf<uint64_t> l64;
};
struct Slab {
  Pinned q, foq, l32, l64, dd, cnt, stats, first_row, entries;
};

struct HipBackend {
  hs_index *ix = nullptr;
  const hs_filter_set *fs = nullptr;
  size_t k = 0, dim = 0, max_q = 0;
  int mode = 0;
  // A host submission whose rows lie in page-locked, device-mapped memory is gathered where it lies (the rows cross the host link
  // once, inside the gather; the caller keeps them unchanged until the ticket's wait returns); any other is staged into the slab.
  // Measured on the bench workload: in place 12.9 vs staged 12.0 M q/s at 1250-query submissions, 13.0 vs 12.0 at 10 000 (DESIGN.md
  // section 5a-10).  HS_QUEUE_IN_PLACE=0 (diagnostic, read when the queue is created) stages everything, for that A/B.
  bool in_place = true;
  std::vector<Slot> slots;
  std::vector<Slab> slabs;

  static int err(std::string *msg, hipError_t e, const char *what) {
    if (msg) *msg = std::string(what) + ": " + hipGetErrorString(e);
    return HS_ERR_DEVICE;
  }
#define Q_TRY(expr)                                       \
  do {                                                    \
    const hipError_t _e = (expr);                         \
    if (_e != hipSuccess) return err(msg, _e, #expr);     \
  } while (0)

  void table(int slab, uint32_t **first_row, SegEntry **entries) {
    *first_row = slabs[slab].first_row.host<uint32_t>();
    *entries = slabs[slab].entries.host<SegEntry>();
  }

  int stage(int slab, size_t first_row, Segment &s, std::string *msg) {
    Q_TRY(hipSetDevice(ix->device));
    SegEntry &e = s.e;
    if (s.device) {
      hipEvent_t ev = nullptr;
      Q_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      const hipError_t r = hipEventRecord(ev, (hipStream_t)s.stream);
      if (r != hipSuccess) { (void)hipEventDestroy(ev); return err(msg, r, "hipEventRecord"); }
      s.event = ev;
      e.src = s.queries; e.foq_src = s.foq;
      e.l32 = s.l32; e.l64 = s.l64; e.dd = s.dd; e.cnt = s.cnt; e.stats = s.stats;
      return HS_OK;
    }
    Slab &b = slabs[slab];
    e.src = in_place ? static_cast<const float *>(hs_host_device_pointer(s.queries)) : nullptr;
    if (!e.src) {
      memcpy(b.q.host<float>() + first_row * dim, s.queries, s.nq * dim * sizeof(float));
      e.src = b.q.dev<float>() + first_row * dim;
    }
    if (fs) {
      memcpy(b.foq.host<uint32_t>() + first_row, s.foq, s.nq * sizeof(uint32_t));
      e.foq_src = b.foq.dev<uint32_t>() + first_row;
    }
    e.l32 = s.l32 ? b.l32.dev<uint32_t>() + first_row * k : nullptr;
    e.l64 = s.l64 ? b.l64.dev<uint64_t>() + first_row * k : nullptr;
    e.dd = s.dd ? b.dd.dev<float>() + first_row * k : nullptr;
    e.cnt = s.cnt ? b.cnt.dev<uint32_t>() + first_row : nullptr;
    e.stats = s.stats ? b.stats.dev<uint32_t>() + first_row * 4 : nullptr;
    return HS_OK;
  }

  int enqueue(int slot, int slab, const std::vector<Segment> &segs, size_t total, std::string *msg) {
    Slot &sl = slots[slot];
    Slab &b = slabs[slab];
    hipError_t first_bad = hipSetDevice(ix->device);
    bool any_dd = false, any_stats = false;
    for (const Segment &s : segs) {   // (every event is consumed, whatever fails)
      any_dd |= s.dd != nullptr;
      any_stats |= s.stats != nullptr;
      if (!s.event) continue;
      const hipError_t r = hipStreamWaitEvent(sl.st, (hipEvent_t)s.event, 0);
      if (first_bad == hipSuccess) first_bad = r;
      (void)hipEventDestroy((hipEvent_t)s.event);
    }
    if (first_bad != hipSuccess) return err(msg, first_bad, "hipStreamWaitEvent");
    if (fs && (fs->n != ix->info.n || fs->device != ix->device)) {
      if (msg) *msg = "the filter set was created for " + std::to_string(fs->n) + " elements, the index holds " + std::to_string(ix->info.n);
      return HS_ERR_INVALID;
    }
    const bool ids = mode == HS_MODE_SLIM_IDS;
    LaunchArrays a{};
    a.q = sl.q.p; a.foq = fs ? sl.foq.p : nullptr;
    a.l32 = ids ? sl.l32.p : nullptr; a.l64 = ids ? nullptr : sl.l64.p;
    a.dd = (!ids || any_dd) ? sl.dd.p : nullptr;
    a.cnt = sl.cnt.p;
    a.stats = any_stats ? sl.stats.p : nullptr;
    // Once the gather is enqueued the slot's stream reads the slab's table and the submissions' sources.  A failure after that
    // point -- a plan error, a scratch allocation -- makes the core free slot and slab at once and hands the error to callers who may
    // free their buffers: so the stream is drained first (error path only; the gather may sit behind device submitters' events).
    const uint32_t n_seg = (uint32_t)segs.size();
    Q_TRY(launch_gather_rows(b.first_row.dev<uint32_t>(), b.entries.dev<SegEntry>(), n_seg, (uint32_t)total, (uint32_t)dim, a.q, a.foq, sl.st));
    const int st = after_gather(sl, b, a, n_seg, total, msg);
    if (st != HS_OK) (void)hipStreamSynchronize(sl.st);
    return st;
  }
  int after_gather(Slot &sl, Slab &b, const LaunchArrays &a, uint32_t n_seg, size_t total, std::string *msg) {
    {
      std::lock_guard<std::mutex> g(g_plan_mu);
      const FilterUse fu{fs, a.foq};
      const hs_status s = search_dev(ix, a.q, total, k, mode, a.l32, a.l64, a.dd, a.cnt, a.stats, nullptr, nullptr, sl.st, fs ? &fu : nullptr);
      if (s != HS_OK) {
        if (msg) *msg = hs_last_error();
        return s;
      }
    }
    Q_TRY(launch_scatter_results(b.first_row.dev<uint32_t>(), b.entries.dev<SegEntry>(), n_seg, (uint32_t)total, (uint32_t)k, a, sl.st));
    Q_TRY(hipEventRecord(sl.done, sl.st));
    return HS_OK;
  }

  int complete(int slot, int slab, const std::vector<Segment> &segs, size_t total, std::string *msg) {
    (void)total;
    Slot &sl = slots[slot];
    Slab &b = slabs[slab];
    Q_TRY(hipSetDevice(ix->device));
    Q_TRY(hipEventSynchronize(sl.done));   // the long wait: outside every lock
    hs_status st;
    {
      std::lock_guard<std::mutex> g(g_plan_mu);
      st = hs_search_check(ix, sl.st);   // capacity / filter-index report of this slot's stream
      if (st != HS_OK && msg) *msg = hs_last_error();
    }
    for (const Segment &s : segs) {   // host submissions: results out of the slab (a reported query still has its padding outputs)
      if (s.device) continue;
      const size_t r = s.first_row;
      if (s.l32) memcpy(s.l32, b.l32.host<uint32_t>() + r * k, s.nq * k * 4);
      if (s.l64) memcpy(s.l64, b.l64.host<uint64_t>() + r * k, s.nq * k * 8);
      if (s.dd) memcpy(s.dd, b.dd.host<float>() + r * k, s.nq * k * 4);
      if (s.cnt) memcpy(s.cnt, b.cnt.host<uint32_t>() + r, s.nq * 4);
      if (s.stats) memcpy(s.stats, b.stats.host<uint32_t>() + r * 4, s.nq * 16);
    }
    return st;
  }

  int join(int slot, void *stream, std::string *msg) {
    Q_TRY(hipSetDevice(ix->device));
    Q_TRY(hipStreamWaitEvent((hipStream_t)stream, slots[slot].done, 0));
    return HS_OK;
  }
#undef Q_TRY
};

}  // namespace

struct hs_queue {
  HipBackend be;
  std::unique_ptr<SearchQueueCore<HipBackend>> core;
  uint64_t device_bytes = 0;
  ~hs_queue() {
    if (!be.ix) return;
    (void)hipSetDevice(be.ix->device);
    for (Slot &s : be.slots) {
      if (s.st) {
        (void)hipStreamSynchronize(s.st);
        std::lock_guard<std::mutex> g(be.ix->ws_mu);
        be.ix->ws.erase(s.st);   // the index's per-stream scratch of a stream that ends here
      }
      if (s.done) (void)hipEventDestroy(s.done);
      if (s.st) (void)hipStreamDestroy(s.st);
    }
    for (Slab &b : be.slabs)
      for (Pinned *p : {&b.q, &b.foq, &b.l32, &b.l64, &b.dd, &b.cnt, &b.stats, &b.first_row, &b.entries}) p->release();
  }
};

static hs_status relay(int st, const std::string &msg) { return st == HS_OK ? HS_OK : fail((hs_status)st, msg); }

hs_status hs_queue_create(hs_index *ix, size_t k, int mode, size_t max_queries, int slots, const hs_filter_set *fs, hs_queue **out) {
  if (!out) return fail(HS_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&] {
    if (!ix) return fail(HS_ERR_INVALID, "null index");
    if (k == 0) return fail(HS_ERR_INVALID, "k must be > 0");
    if (mode != HS_MODE_SLIM_IDS && mode != HS_MODE_PQ) return fail(HS_ERR_INVALID, "bad mode");
    if (ix->info.kind == HS_KIND_SLIMQ) return fail(HS_ERR_INVALID, "SlimQ index: a search queue serves HNSW and Slim indexes");
    if (mode == HS_MODE_SLIM_IDS && ix->info.kind != HS_KIND_SLIM)
      return fail(HS_ERR_INVALID, "HS_MODE_SLIM_IDS needs a Slim index (searchKnn(q,k,tableint*) exists on HierarchicalNSWSlim only)");
    if (max_queries == 0 || max_queries > kQueueMaxQueries) return fail(HS_ERR_INVALID, "max_queries: 1.." + std::to_string(kQueueMaxQueries));
    if (slots < 1 || slots > kQueueMaxSlots) return fail(HS_ERR_INVALID, "slots: 1.." + std::to_string(kQueueMaxSlots));
    if (k > 0xFFFFFFFFu / 8 / max_queries) return fail(HS_ERR_INVALID, "k too large");
    if (fs) {
      if (mode != HS_MODE_PQ) return fail(HS_ERR_INVALID, "a queue under a filter set answers in HS_MODE_PQ (as hs_search_batch_filter_set)");
      if (ix->info.kind == HS_KIND_SLIM && ix->info.threshold_level != 0)
        return fail(HS_ERR_UNSUPPORTED, "filtered search on a Slim index with threshold_level > 0 is not supported");
      if (fs->device != ix->device)
        return fail(HS_ERR_INVALID, "the filter set lives on device " + std::to_string(fs->device) + ", the index on device " + std::to_string(ix->device));
      if (fs->n != ix->info.n)
        return fail(HS_ERR_INVALID, "the filter set was created for " + std::to_string(fs->n) + " elements, the index holds " + std::to_string(ix->info.n));
    }
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_ptr<hs_queue> q(new hs_queue());
    HipBackend &be = q->be;
    be.ix = ix; be.fs = fs; be.k = k; be.dim = ix->info.dim; be.max_q = max_queries; be.mode = mode;
    const char *knob = getenv("HS_QUEUE_IN_PLACE");
    be.in_place = !(knob && knob[0] == '0');
    const bool ids = mode == HS_MODE_SLIM_IDS;
    const size_t m = max_queries, dim = be.dim;
    be.slots.resize(slots);
    be.slabs.resize(slots + 1);
    for (Slot &s : be.slots) {
      HIP_TRY(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
      HIP_TRY(s.q.alloc(m * dim));
      if (fs) HIP_TRY(s.foq.alloc(m));
      if (ids) HIP_TRY(s.l32.alloc(m * k));
      else HIP_TRY(s.l64.alloc(m * k));
      HIP_TRY(s.dd.alloc(m * k));
      HIP_TRY(s.cnt.alloc(m));
      HIP_TRY(s.stats.alloc(m * 4));
      q->device_bytes += (s.q.n + s.dd.n + s.foq.n + s.l32.n + s.cnt.n + s.stats.n) * 4 + s.l64.n * 8;
    }
    for (Slab &b : be.slabs) {
      HIP_TRY(b.q.alloc(m * dim * 4));
      if (fs) HIP_TRY(b.foq.alloc(m * 4));
      if (ids) HIP_TRY(b.l32.alloc(m * k * 4));
      else HIP_TRY(b.l64.alloc(m * k * 8));
      HIP_TRY(b.dd.alloc(m * k * 4));
      HIP_TRY(b.cnt.alloc(m * 4));
      HIP_TRY(b.stats.alloc(m * 16));
      HIP_TRY(b.first_row.alloc((m + 1) * 4));
      HIP_TRY(b.entries.alloc(m * sizeof(SegEntry)));
    }
    q->core.reset(new SearchQueueCore<HipBackend>(be, max_queries, slots));
    *out = q.release();
    return HS_OK;
  });
}

void hs_queue_free(hs_queue *q) {
  if (!q) return;
  (void)guarded([&] {   // (what the last launches report has nobody left to read it)
    std::string msg;
    (void)q->core->drain(&msg);
    return HS_OK;
  });
  delete q;
}

static hs_status queue_submit(hs_queue *q, bool device, const float *queries, size_t nq, const uint32_t *filter_of_query,
                              uint32_t *l32, uint64_t *l64, float *dd, uint32_t *cnt, uint32_t *stats, void *stream, uint64_t *ticket) {
  if (!q || !ticket) return fail(HS_ERR_INVALID, "null argument");
  if (nq > 0) {
    if (!queries) return fail(HS_ERR_INVALID, "null queries");
    if (q->be.mode == HS_MODE_SLIM_IDS && !l32) return fail(HS_ERR_INVALID, "out_labels32 required");
    if (q->be.mode == HS_MODE_PQ && (!l64 || !dd || !cnt)) return fail(HS_ERR_INVALID, "out_labels64/out_dists/out_counts required");
    if (q->be.fs && !filter_of_query) return fail(HS_ERR_INVALID, "filter_of_query required on a queue under a filter set");
  }
  Segment s;
  s.queries = queries; s.nq = nq; s.foq = q->be.fs ? filter_of_query : nullptr;
  // (only the outputs of the queue's mode travel: the other label array is not the search's to write)
  s.l32 = q->be.mode == HS_MODE_SLIM_IDS ? l32 : nullptr;
  s.l64 = q->be.mode == HS_MODE_PQ ? l64 : nullptr;
  s.dd = dd; s.cnt = cnt; s.stats = stats;
  s.device = device; s.stream = stream;
  std::string msg;
  return relay(q->core->submit(s, ticket, &msg), msg);
}

hs_status hs_queue_submit(hs_queue *q, const float *queries, size_t nq, const uint32_t *filter_of_query, uint32_t *out_labels32,
                          uint64_t *out_labels64, float *out_dists, uint32_t *out_counts, uint32_t *stats, uint64_t *ticket) {
  return guarded([&] { return queue_submit(q, false, queries, nq, filter_of_query, out_labels32, out_labels64, out_dists, out_counts, stats, nullptr, ticket); });
}

hs_status hs_queue_submit_dev(hs_queue *q, const float *d_queries, size_t nq, const uint32_t *d_filter_of_query, uint32_t *d_out_labels32,
                              uint64_t *d_out_labels64, float *d_out_dists, uint32_t *d_out_counts, uint32_t *d_stats, void *stream,
                              uint64_t *ticket) {
  return guarded([&] {
    return queue_submit(q, true, d_queries, nq, d_filter_of_query, d_out_labels32, d_out_labels64, d_out_dists, d_out_counts, d_stats, stream, ticket);
  });
}

// flush / wait / join_stream / drain: one call into the core, its status and text relayed
template <class Call>
static hs_status core_call(hs_queue *q, Call &&call) {
  if (!q) return fail(HS_ERR_INVALID, "null argument");
  return guarded([&] {
    std::string msg;
    const int st = call(*q->core, &msg);
    return relay(st, msg);
  });
}
hs_status hs_queue_flush(hs_queue *q) {
  return core_call(q, [](SearchQueueCore<HipBackend> &c, std::string *msg) { return c.flush(msg); });
}
hs_status hs_queue_wait(hs_queue *q, uint64_t ticket) {
  return core_call(q, [=](SearchQueueCore<HipBackend> &c, std::string *msg) { return c.wait(ticket, msg); });
}
hs_status hs_queue_join_stream(hs_queue *q, uint64_t ticket, void *stream) {
  return core_call(q, [=](SearchQueueCore<HipBackend> &c, std::string *msg) { return c.join_stream(ticket, stream, msg); });
}
hs_status hs_queue_drain(hs_queue *q) {
  return core_call(q, [](SearchQueueCore<HipBackend> &c, std::string *msg) { return c.drain(msg); });
}

hs_status hs_queue_info(const hs_queue *q, struct hs_queue_info *out) {
  if (!q || !out) return fail(HS_ERR_INVALID, "null argument");
  const QueueInfo i = q->core->info();
  out->submitted = i.submitted; out->launches = i.launches; out->pending = i.pending; out->in_flight = i.in_flight;
  out->largest_launch = i.largest_launch; out->device_bytes = q->device_bytes;
  return HS_OK;
}
