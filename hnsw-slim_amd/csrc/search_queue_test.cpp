// search_queue_test.cpp -- host-only test of csrc/search_queue.hpp, the bookkeeping of the search queue (capi_queue.cpp), against a
// fake CPU backend: "gather" reads the segment table the core wrote, the fake "search" writes a function of each query's first
// float into that query's outputs, "scatter" follows the table back -- in complete(), outside the core's lock, as the real backend's copy-out.  Built twice (make search_queue_test): under AddressSanitizer
// / UBSan, and under ThreadSanitizer, where the threaded case is the point.  Stand-alone binaries, never loaded into Python.
// Build: g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined search_queue_test.cpp -o search_queue_test
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>

#include "search_queue.hpp"

using namespace hs;

static constexpr size_t kDim = 3, kK = 2;
static constexpr int kStCapacity = 7;   // HS_ERR_CAPACITY

// what the fake search answers for a query whose first float is x (x may be negative: through int32)
static uint32_t label_of(float x) { return (uint32_t)(int32_t)(2 * x + 1); }

struct FakeBackend {
  size_t max_q;
  struct Slab { std::vector<float> q; std::vector<uint32_t> first_row; std::vector<SegEntry> entries; };
  struct Slot { std::vector<float> q; std::vector<uint32_t> l32; std::vector<float> dd; std::vector<uint32_t> cnt, stats; std::atomic<int> busy{0}; int status = 0; };
  std::vector<Slab> slabs;
  std::vector<std::unique_ptr<Slot>> slots;
  std::atomic<int> fail_next{0}, joins{0}, completes{0}, bad{0};
  std::vector<size_t> launch_sizes, launch_segs;   // written under the core's lock

  FakeBackend(size_t max_queries, int n_slots) : max_q(max_queries), slabs(n_slots + 1) {
    for (Slab &b : slabs) { b.q.resize(max_q * kDim); b.first_row.resize(max_q + 1); b.entries.resize(max_q); }
    for (int i = 0; i < n_slots; i++) {
      slots.emplace_back(new Slot());
      Slot &s = *slots.back();
      s.q.resize(max_q * kDim); s.l32.resize(max_q * kK); s.dd.resize(max_q * kK); s.cnt.resize(max_q); s.stats.resize(max_q * 4);
    }
  }
  void table(int slab, uint32_t **first_row, SegEntry **entries) { *first_row = slabs[slab].first_row.data(); *entries = slabs[slab].entries.data(); }
  int stage(int slab, size_t first_row, Segment &s, std::string *) {
    if (first_row + s.nq > max_q) bad++;
    memcpy(&slabs[slab].q[first_row * kDim], s.queries, s.nq * kDim * sizeof(float));
    s.e.src = &slabs[slab].q[first_row * kDim];
    s.e.l32 = s.l32; s.e.dd = s.dd; s.e.cnt = s.cnt; s.e.stats = s.stats;
    return kStOk;
  }
  int enqueue(int slot, int slab, const std::vector<Segment> &segs, size_t total, std::string *msg) {
    launch_sizes.push_back(total);
    launch_segs.push_back(segs.size());
    if (fail_next.exchange(0)) { *msg = "fake enqueue failure"; return kStCapacity; }
    Slot &sl = *slots[slot];
    if (sl.busy.exchange(1)) bad++;   // a slot is never handed out twice
    const Slab &b = slabs[slab];
    const uint32_t n_seg = (uint32_t)segs.size();
    if (b.first_row[0] != 0 || b.first_row[n_seg] != total || total > max_q) bad++;
    sl.status = kStOk;
    for (uint32_t row = 0; row < total; row++) {   // gather
      const uint32_t s = segment_of_row(b.first_row.data(), n_seg, row);
      if (!(b.first_row[s] <= row && row < b.first_row[s + 1])) bad++;
      memcpy(&sl.q[row * kDim], b.entries[s].src + (row - b.first_row[s]) * kDim, kDim * sizeof(float));
    }
    for (uint32_t row = 0; row < total; row++) {   // "search"
      const float x = sl.q[row * kDim];
      if (x < 0) sl.status = kStCapacity;          // a query that the capacity check of this launch reports
      for (size_t j = 0; j < kK; j++) { sl.l32[row * kK + j] = label_of(x) + (uint32_t)j; sl.dd[row * kK + j] = x + 0.5f + j; }
      sl.cnt[row] = (uint32_t)kK;
      for (size_t j = 0; j < 4; j++) sl.stats[row * 4 + j] = label_of(x) * 4 + (uint32_t)j;
    }
    return kStOk;
  }
  // as the HIP backend: the callers' buffers are written here, outside the core's lock
  int complete(int slot, int slab, const std::vector<Segment> &segs, size_t total, std::string *msg) {
    Slot &sl = *slots[slot];
    const Slab &b = slabs[slab];
    const uint32_t n_seg = (uint32_t)segs.size();
    completes++;
    std::this_thread::yield();
    for (uint32_t row = 0; row < total; row++) {   // scatter
      const uint32_t s = segment_of_row(b.first_row.data(), n_seg, row);
      const size_t local = row - b.first_row[s];
      const SegEntry &e = b.entries[s];
      for (size_t j = 0; j < kK; j++) {
        if (e.l32) e.l32[local * kK + j] = sl.l32[row * kK + j];
        if (e.dd) e.dd[local * kK + j] = sl.dd[row * kK + j];
      }
      if (e.cnt) e.cnt[local] = sl.cnt[row];
      for (size_t j = 0; j < 4; j++)
        if (e.stats) e.stats[local * 4 + j] = sl.stats[row * 4 + j];
    }
    const int st = sl.status;
    if (st != kStOk) *msg = "fake capacity report";
    if (!sl.busy.exchange(0)) bad++;
    return st;
  }
  int join(int, void *, std::string *) { joins++; return kStOk; }
};

// One caller's batch and the buffers its answers land in.
struct Batch {
  std::vector<float> q;
  std::vector<uint32_t> l32, cnt, stats;
  std::vector<float> dd;
  uint64_t ticket = 0;
  Batch(size_t nq, float first, bool want_dd = true, bool want_stats = true)
      : q(nq * kDim), l32(nq * kK, 77u), cnt(nq, 77u), stats(want_stats ? nq * 4 : 0, 77u), dd(want_dd ? nq * kK : 0, -1.f) {
    for (size_t i = 0; i < nq; i++) q[i * kDim] = first + (float)i;
  }
  size_t nq() const { return cnt.size(); }
  Segment seg() {
    Segment s;
    s.queries = q.data(); s.nq = nq(); s.l32 = l32.data(); s.cnt = cnt.data();
    s.dd = dd.empty() ? nullptr : dd.data(); s.stats = stats.empty() ? nullptr : stats.data();
    return s;
  }
  bool answered() const {
    for (size_t i = 0; i < nq(); i++) {
      const float x = q[i * kDim];
      for (size_t j = 0; j < kK; j++) {
        if (l32[i * kK + j] != label_of(x) + j) return false;
        if (!dd.empty() && dd[i * kK + j] != x + 0.5f + j) return false;
      }
      if (cnt[i] != kK) return false;
      for (size_t j = 0; j < 4; j++)
        if (!stats.empty() && stats[i * 4 + j] != label_of(x) * 4 + j) return false;
    }
    return true;
  }
  bool untouched() const {
    for (uint32_t v : l32) if (v != 77u) return false;
    return true;
  }
};

static int cases = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using Core = SearchQueueCore<FakeBackend>;

// n_seg segments of rows_each rows in one launch: every ticket answered, one launch, the table's prefix right
static int segments_case(size_t n_seg, size_t rows_each) {
  FakeBackend be(1024, 2);
  Core q(be, 1024, 2);
  std::vector<std::unique_ptr<Batch>> bs;
  std::string msg;
  for (size_t i = 0; i < n_seg; i++) {
    bs.emplace_back(new Batch(rows_each + (rows_each > 1 ? i % 3 : 0), (float)(i * 10), i % 2 == 0, i % 3 != 0));
    CHECK(q.submit(bs.back()->seg(), &bs.back()->ticket, &msg) == kStOk);
  }
  CHECK(be.launch_sizes.empty() && q.info().pending == q.info().submitted);
  CHECK(q.wait(bs[n_seg / 2]->ticket, &msg) == kStOk);   // any ticket's wait flushes all
  CHECK(be.launch_sizes.size() == 1 && be.launch_segs[0] == n_seg && be.launch_sizes[0] == q.info().submitted);
  CHECK(q.info().launches == 1 && q.info().largest_launch == q.info().submitted && q.info().pending == 0 && q.info().in_flight == 0);
  for (size_t i = 0; i < n_seg; i++) {
    CHECK(bs[i]->answered());
    if (i != n_seg / 2) CHECK(q.wait(bs[i]->ticket, &msg) == kStOk);
  }
  CHECK(be.completes == 1 && be.bad == 0);
  cases++;
  return 0;
}

static int auto_flush_case() {
  std::string msg;
  for (size_t last : {(size_t)15, (size_t)16, (size_t)17}) {   // one below, exactly at, one above max_queries = 64 after 48 pending
    FakeBackend be(64, 2);
    Core q(be, 64, 2);
    Batch a(48, 0), b(last, 100);
    CHECK(q.submit(a.seg(), &a.ticket, &msg) == kStOk && q.submit(b.seg(), &b.ticket, &msg) == kStOk);
    if (last <= 16) {
      CHECK(be.launch_sizes.empty() && q.info().pending == 48 + last);
    } else {
      CHECK(be.launch_sizes == std::vector<size_t>{48} && q.info().pending == last && q.info().in_flight == 1);
    }
    Batch c(1, 200);   // one more: past the limit in the "exactly at" case only
    CHECK(q.submit(c.seg(), &c.ticket, &msg) == kStOk);
    if (last == 16) CHECK(be.launch_sizes == std::vector<size_t>{64} && q.info().pending == 1);
    CHECK(q.drain(&msg) == kStOk && a.answered() && b.answered() && c.answered() && be.bad == 0);
    CHECK(q.info().pending == 0 && q.info().in_flight == 0 && q.info().submitted == 49 + last);
    cases++;
  }
  return 0;
}

static int refusals_case() {
  std::string msg;
  FakeBackend be(64, 2);
  Core q(be, 64, 2);
  Batch a(5, 0), big(65, 0), none(0, 0);
  CHECK(q.submit(a.seg(), &a.ticket, &msg) == kStOk);
  // oversize: refused, state unchanged
  uint64_t t = 999;
  CHECK(q.submit(big.seg(), &t, &msg) == kStInvalid && t == 999 && !msg.empty());
  CHECK(q.info().pending == 5 && q.info().submitted == 5 && q.info().launches == 0 && be.launch_sizes.empty());
  // nq == 0: a ticket that is already complete; its wait launches nothing
  CHECK(q.submit(none.seg(), &none.ticket, &msg) == kStOk && none.ticket != 0 && none.ticket != a.ticket);
  CHECK(q.wait(none.ticket, &msg) == kStOk && q.info().launches == 0 && q.info().pending == 5);
  CHECK(q.wait(none.ticket, &msg) == kStInvalid);
  // join_stream keeps the ticket, wait releases it; double wait and unknown ticket
  CHECK(q.join_stream(a.ticket, nullptr, &msg) == kStOk && be.joins == 1 && q.info().launches == 1 && q.info().in_flight == 1);
  CHECK(q.wait(a.ticket, &msg) == kStOk && a.answered());
  CHECK(q.join_stream(a.ticket, nullptr, &msg) == kStInvalid);
  CHECK(q.wait(a.ticket, &msg) == kStInvalid && q.wait(12345, &msg) == kStInvalid && q.wait(0, &msg) == kStInvalid);
  CHECK(q.flush(&msg) == kStOk && q.info().launches == 1);   // nothing pending: no launch
  CHECK(be.bad == 0);
  cases++;
  return 0;
}

static int slots_case() {
  std::string msg;
  // slots exhausted: the third flush completes the oldest launch to get its slot; completion order is launch order
  FakeBackend be(64, 2);
  Core q(be, 64, 2);
  Batch a(3, 0), b(4, 10), c(5, 20), d(6, 30);
  CHECK(q.submit(a.seg(), &a.ticket, &msg) == kStOk && q.flush(&msg) == kStOk);
  CHECK(q.submit(b.seg(), &b.ticket, &msg) == kStOk && q.flush(&msg) == kStOk);
  CHECK(q.info().in_flight == 2 && be.completes == 0);
  CHECK(q.submit(c.seg(), &c.ticket, &msg) == kStOk);   // submit itself never waits for a slot
  CHECK(be.completes == 0 && q.info().in_flight == 2 && q.info().pending == 5);
  CHECK(q.flush(&msg) == kStOk && be.completes == 1 && q.info().in_flight == 2);
  CHECK(q.wait(c.ticket, &msg) == kStOk && c.answered() && be.completes == 2);   // out of order: c before b
  CHECK(q.wait(a.ticket, &msg) == kStOk && a.answered() && be.completes == 2);   // completed by the flush, status kept
  CHECK(q.wait(b.ticket, &msg) == kStOk && b.answered() && be.completes == 3);
  // one slot: three flushes complete in order
  FakeBackend be1(64, 1);
  Core q1(be1, 64, 1);
  Batch x(1, 0), y(2, 10), z(3, 20);
  CHECK(q1.submit(x.seg(), &x.ticket, &msg) == kStOk && q1.flush(&msg) == kStOk);
  CHECK(q1.submit(y.seg(), &y.ticket, &msg) == kStOk && q1.flush(&msg) == kStOk && be1.completes == 1);
  CHECK(q1.submit(z.seg(), &z.ticket, &msg) == kStOk && q1.flush(&msg) == kStOk && be1.completes == 2);
  CHECK(q1.wait(z.ticket, &msg) == kStOk && q1.wait(y.ticket, &msg) == kStOk && q1.wait(x.ticket, &msg) == kStOk);
  CHECK(x.answered() && y.answered() && z.answered() && be1.launch_sizes == (std::vector<size_t>{1, 2, 3}));
  CHECK(be.bad == 0 && be1.bad == 0);
  cases++;
  return 0;
}

static int errors_case() {
  std::string msg;
  FakeBackend be(64, 2);
  Core q(be, 64, 2);
  // a launch that cannot be enqueued: all its tickets carry the error, nothing was written, later launches are unaffected
  Batch a(2, 0), b(3, 10), c(4, 20);
  CHECK(q.submit(a.seg(), &a.ticket, &msg) == kStOk && q.submit(b.seg(), &b.ticket, &msg) == kStOk);
  be.fail_next = 1;
  CHECK(q.flush(&msg) == kStOk && q.info().in_flight == 0);
  CHECK(q.submit(c.seg(), &c.ticket, &msg) == kStOk);
  msg.clear();
  CHECK(q.wait(a.ticket, &msg) == kStCapacity && msg == "fake enqueue failure" && a.untouched());
  CHECK(q.wait(c.ticket, &msg) == kStOk && c.answered());
  msg.clear();
  CHECK(q.wait(b.ticket, &msg) == kStCapacity && msg == "fake enqueue failure" && b.untouched());
  // a launch whose check reports: every ticket of it, and only of it
  Batch d(2, 0), e(1, -5), f(2, 30);
  CHECK(q.submit(d.seg(), &d.ticket, &msg) == kStOk && q.submit(e.seg(), &e.ticket, &msg) == kStOk && q.flush(&msg) == kStOk);
  CHECK(q.submit(f.seg(), &f.ticket, &msg) == kStOk);
  CHECK(q.wait(d.ticket, &msg) == kStCapacity && msg == "fake capacity report" && d.answered());
  CHECK(q.wait(f.ticket, &msg) == kStOk && f.answered());
  CHECK(q.wait(e.ticket, &msg) == kStCapacity);
  // drain with unwaited tickets: everything completes, every ticket is released, the first error is reported
  Batch g(2, 0), h(1, -1), i(3, 40);
  CHECK(q.submit(g.seg(), &g.ticket, &msg) == kStOk && q.flush(&msg) == kStOk);
  CHECK(q.submit(h.seg(), &h.ticket, &msg) == kStOk && q.flush(&msg) == kStOk);
  CHECK(q.submit(i.seg(), &i.ticket, &msg) == kStOk);
  CHECK(q.drain(&msg) == kStCapacity && g.answered() && i.answered());
  CHECK(q.info().pending == 0 && q.info().in_flight == 0);
  CHECK(q.wait(g.ticket, &msg) == kStInvalid && q.wait(h.ticket, &msg) == kStInvalid && q.wait(i.ticket, &msg) == kStInvalid);
  CHECK(q.drain(&msg) == kStOk && be.bad == 0);
  cases++;
  return 0;
}

// 8 threads x 200 submit + wait of one to three rows against two slots
static int threads_case() {
  FakeBackend be(16, 2);
  Core q(be, 16, 2);
  std::atomic<int> wrong{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < 8; t++)
    ts.emplace_back([&, t] {
      std::string msg;
      for (int i = 0; i < 200; i++) {
        Batch b(1 + (size_t)(i + t) % 3, (float)(t * 1000 + i));
        if (q.submit(b.seg(), &b.ticket, &msg) != kStOk) { wrong++; continue; }
        if (i % 7 == 0 && q.flush(&msg) != kStOk) wrong++;
        if (q.wait(b.ticket, &msg) != kStOk || !b.answered()) wrong++;
        if (q.wait(b.ticket, &msg) != kStInvalid) wrong++;
      }
    });
  for (auto &t : ts) t.join();
  std::string msg;
  CHECK(wrong == 0 && be.bad == 0 && q.drain(&msg) == kStOk);
  const QueueInfo i = q.info();
  size_t sum = 0;
  for (size_t s : be.launch_sizes) { CHECK(s >= 1 && s <= 16); sum += s; }
  CHECK(i.pending == 0 && i.in_flight == 0 && i.launches == be.launch_sizes.size() && i.launches <= 1600 && sum == i.submitted);
  cases++;
  return 0;
}

// 12 threads of submit + wait while one thread drains over and over: a ticket may be released by the drain, but only once its
// launch is done -- whichever status the wait returns, the answers are in place when it returns, and nothing is written after
// (the batches die right after their wait: a late write is a use after free)
static int drain_against_wait_case() {
  FakeBackend be(16, 2);
  Core q(be, 16, 2);
  std::atomic<int> wrong{0}, live{12}, lost{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < 12; t++)
    ts.emplace_back([&, t] {
      std::string msg;
      for (int i = 0; i < 150; i++) {
        Batch b(1 + (size_t)(i + t) % 3, (float)(t * 1000 + i));
        if (q.submit(b.seg(), &b.ticket, &msg) != kStOk) { wrong++; continue; }
        const int st = q.wait(b.ticket, &msg);
        if (st == kStInvalid) lost++;
        if ((st != kStOk && st != kStInvalid) || !b.answered()) wrong++;
      }
      live--;
    });
  std::thread drainer([&] {
    std::string msg;
    while (live.load() > 0)
      if (q.drain(&msg) != kStOk) wrong++;
  });
  for (auto &t : ts) t.join();
  drainer.join();
  std::string msg;
  CHECK(wrong == 0 && be.bad == 0 && q.drain(&msg) == kStOk);
  CHECK(q.info().pending == 0 && q.info().in_flight == 0 && q.info().submitted > 0);
  printf("drain against wait: %d of 1800 tickets released by the drain first\n", lost.load());
  cases++;
  return 0;
}

int main() {
  for (size_t n_seg : {1, 2, 64, 65, 300})
    if (segments_case(n_seg, 2)) return 1;
  if (segments_case(300, 1)) return 1;   // segments of one row
  if (auto_flush_case() || refusals_case() || slots_case() || errors_case() || threads_case() || drain_against_wait_case()) return 1;
  printf("search_queue ok: %d cases\n", cases);
  return 0;
}
