// search_queue.hpp -- the bookkeeping of a search queue (hs_queue_*, capi_queue.cpp), host only and without HIP: small submissions
// from any thread are gathered into one launch per flush, and every query's results go back to its own caller's buffers.
//
// What lives here: the segment table (one entry per submission of a launch: where its rows come from, where its results go, its
// first row in the launch), when a submission triggers a flush, ticket -> launch -> status, the rotation of slots and slabs, and
// who completes a launch.  What does not: anything that touches a device.  The core is parameterised on a backend:
//   void  table(int slab, uint32_t **first_row, SegEntry **entries)   the slab's segment table (room for max_queries + 1 / max_queries)
//   int   stage(int slab, size_t first_row, Segment &s, std::string *msg)
//         a submission joins the launch that fills `slab`: host queries are copied into the slab (the caller's buffer is free when
//         submit returns), a device submission records its stream; fills s.e -- the submission's entry of the table
//   int   enqueue(int slot, int slab, const std::vector<Segment> &segs, size_t total, std::string *msg)
//         gather, one search launch group over `total` rows, scatter -- enqueued on the slot's stream, never blocking on it
//   int   complete(int slot, int slab, const std::vector<Segment> &segs, size_t total, std::string *msg)
//         block until the slot's launch is done, run its capacity check, hand host submissions their results
//   int   join(int slot, void *stream, std::string *msg)              `stream` waits for the slot's launch, the host does not
// Statuses are the C ABI's (0 = HS_OK, 4 = HS_ERR_INVALID); the core passes a backend's status and text through to every ticket of
// the launch they belong to.
//
// Rules (the header comment of hs_queue_* states them for callers):
//   - a submission that would take the pending total past max_queries flushes what is pending first and joins the next launch;
//     nq > max_queries is refused and changes nothing; nq == 0 gets a ticket that is already complete
//   - `slots` launches may be in flight, each on its own slot (stream + result staging); a flush that finds every slot busy
//     completes the oldest launch first.  Queries are staged into slabs, of which there is one more than slots: a launch holds its
//     slab from its first submission until it is complete, so the launch being filled always has one and submit never waits
//   - whoever first needs a launch done (a wait on one of its tickets, a flush that needs its slot, drain) completes it, outside
//     the lock; others that need it meanwhile sleep on the condition variable.  A launch that could not be enqueued is complete at
//     once, with the error, and holds no slot: nothing ever waits forever
//   - a ticket is released by its wait, or by drain once its launch is done (a wait that loses that race gets HS_ERR_INVALID with
//     its results already in place); a second wait or an unknown ticket is HS_ERR_INVALID
#pragma once
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "hd.hpp"

namespace hs {

// One entry of the segment table, as the copy kernels (segment_copy.hip) read it: device-visible addresses; a null output is one
// the submission did not ask for.  64 bytes.
struct SegEntry {
  const float *src;         // the submission's rows, nq x dim
  const uint32_t *foq_src;  // its filter indices (null without a filter set)
  uint32_t *l32;
  uint64_t *l64;
  float *dd;
  uint32_t *cnt, *stats;
  uint64_t pad;
};
static_assert(sizeof(SegEntry) == 64, "SegEntry is read by the device as 64-byte records");

// The segment of a row: the last s in [0, n_seg) with first_row[s] <= row (first_row[0] == 0, strictly increasing; first_row[n_seg]
// = total rows).  The same search on the host (the core's test) and in both kernels, over LDS or global memory.
HS_HD uint32_t segment_of_row(const uint32_t *first_row, uint32_t n_seg, uint32_t row) {
  uint32_t lo = 0, hi = n_seg;   // invariant: first_row[lo] <= row < first_row[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (first_row[mid] <= row) lo = mid;
    else hi = mid;
  }
  return lo;
}

constexpr int kStOk = 0, kStInvalid = 4;   // HS_OK, HS_ERR_INVALID
constexpr size_t kQueueMaxQueries = 32768; // one launch group of the search (capi_search.cpp)
constexpr int kQueueMaxSlots = 16;

// One submission.  The caller's pointers as given; `e` is what the table carries (filled by Backend::stage).
struct Segment {
  const float *queries = nullptr;
  size_t nq = 0;
  const uint32_t *foq = nullptr;
  uint32_t *l32 = nullptr;
  uint64_t *l64 = nullptr;
  float *dd = nullptr;
  uint32_t *cnt = nullptr, *stats = nullptr;
  bool device = false;
  void *stream = nullptr;   // device submissions: the caller's stream
  void *event = nullptr;    // ... and the event recorded on it at submit (the backend's)
  uint64_t ticket = 0;
  size_t first_row = 0;
  SegEntry e{};
};

struct QueueInfo {
  uint64_t submitted = 0, launches = 0, pending = 0, in_flight = 0, largest_launch = 0;
};

template <class Backend>
class SearchQueueCore {
 public:
  SearchQueueCore(Backend &b, size_t max_queries, int slots) : be_(b), max_(max_queries), slots_(slots) {
    for (int i = slots - 1; i >= 0; i--) free_slots_.push_back(i);
    for (int i = slots; i >= 1; i--) free_slabs_.push_back(i);
    fill_slab_ = 0;
  }

  int submit(Segment s, uint64_t *ticket, std::string *msg) {
    std::unique_lock<std::mutex> g(mu_);
    if (s.nq > max_) return say(msg, kStInvalid, "a submission of " + std::to_string(s.nq) + " queries on a queue of max_queries " + std::to_string(max_));
    if (s.nq == 0) {   // nothing to search: a ticket that is already complete
      const uint64_t t = next_ticket_++;
      tickets_[t] = nullptr;
      if (ticket) *ticket = t;
      return kStOk;
    }
    while (pending_total_ + s.nq > max_) flush_locked(g);   // (a flush may wait for a slot unlocked: look again)
    s.ticket = next_ticket_;
    s.first_row = pending_total_;
    const int st = be_.stage(fill_slab_, s.first_row, s, msg);
    if (st != kStOk) return st;   // nothing joined, no ticket
    next_ticket_++;
    if (!fill_) fill_ = std::make_shared<Launch>();
    tickets_[s.ticket] = fill_;
    pending_total_ += s.nq;
    info_.submitted += s.nq;
    if (ticket) *ticket = s.ticket;
    pending_.push_back(std::move(s));
    return kStOk;
  }

  int flush(std::string *msg) {
    std::unique_lock<std::mutex> g(mu_);
    (void)msg;
    flush_locked(g);
    return kStOk;   // a launch's errors belong to its tickets
  }

  int wait(uint64_t ticket, std::string *msg) {
    std::unique_lock<std::mutex> g(mu_);
    auto it = tickets_.find(ticket);
    if (it == tickets_.end()) return say(msg, kStInvalid, "unknown ticket " + std::to_string(ticket) + " (a ticket is waited once)");
    std::shared_ptr<Launch> L = it->second;
    tickets_.erase(it);   // released here: a second wait, from any thread, finds nothing
    if (!L) return kStOk;
    while (L->state == kFilling) flush_locked(g);
    finish(L, g);
    return say(msg, L->status, L->msg);
  }

  int join_stream(uint64_t ticket, void *stream, std::string *msg) {
    std::unique_lock<std::mutex> g(mu_);
    auto it = tickets_.find(ticket);
    if (it == tickets_.end()) return say(msg, kStInvalid, "unknown ticket " + std::to_string(ticket));
    std::shared_ptr<Launch> L = it->second;   // (the ticket stays: its wait, or drain, still reports the launch's status)
    if (!L) return kStOk;
    while (L->state == kFilling) flush_locked(g);
    if (L->state == kDone) return say(msg, L->status, L->msg);
    return be_.join(L->slot, stream, msg);   // in flight or being completed: its slot is still its own
  }

  int drain(std::string *msg) {
    std::unique_lock<std::mutex> g(mu_);
    int first = kStOk;
    std::string first_msg;
    while (fill_) flush_locked(g);
    // every ticket outstanding at this moment: complete its launch, THEN release it.  A ticket stays findable until its launch is
    // done, so a wait that races this drain either takes the ticket itself (and sleeps until the launch is done) or finds it gone
    // after its results are in the caller's buffers -- never while the launch may still write them.
    std::vector<uint64_t> ids;
    for (auto &t : tickets_) ids.push_back(t.first);
    for (uint64_t id : ids) {
      auto it = tickets_.find(id);
      if (it == tickets_.end()) continue;   // waited meanwhile
      std::shared_ptr<Launch> L = it->second;
      if (L) {
        while (L->state == kFilling) flush_locked(g);   // (a submission that joined while the lock was released)
        finish(L, g);                                   // may release the lock: `it` is not used again
        if (L->status != kStOk && first == kStOk) { first = L->status; first_msg = L->msg; }
      }
      tickets_.erase(id);
    }
    while (!in_flight_.empty()) {   // launches whose tickets were all waited cannot exist; launches being completed elsewhere can
      std::shared_ptr<Launch> L = in_flight_.begin()->second;
      finish(L, g);
    }
    return say(msg, first, first_msg);
  }

  QueueInfo info() {
    std::lock_guard<std::mutex> g(mu_);
    QueueInfo i = info_;
    i.pending = pending_total_;
    i.in_flight = in_flight_.size();
    return i;
  }

 private:
  enum State { kFilling, kInFlight, kCompleting, kDone };
  struct Launch {
    uint64_t id = 0;
    State state = kFilling;
    int slot = -1, slab = -1;
    std::vector<Segment> segs;
    size_t total = 0;
    int status = kStOk;
    std::string msg;
  };

  static int say(std::string *msg, int st, const std::string &text) {
    if (msg && st != kStOk) *msg = text;
    return st;
  }

  // L is in flight, being completed by another thread, or done: return once it is done.
  void finish(const std::shared_ptr<Launch> &L, std::unique_lock<std::mutex> &g) {
    if (L->state == kInFlight) {
      L->state = kCompleting;
      g.unlock();
      std::string m;
      const int st = be_.complete(L->slot, L->slab, L->segs, L->total, &m);   // blocks: outside the lock
      g.lock();
      L->status = st;
      L->msg = m;
      L->state = kDone;
      free_slots_.push_back(L->slot);
      free_slabs_.push_back(L->slab);
      in_flight_.erase(L->id);
      cv_.notify_all();
      return;
    }
    cv_.wait(g, [&] { return L->state == kDone; });
  }

  // Turn what is pending into a launch.  One flusher at a time: it may release the lock while it frees a slot.
  void flush_locked(std::unique_lock<std::mutex> &g) {
    if (flushing_) {   // someone else is at it; the caller re-examines its reason afterwards
      cv_.wait(g, [&] { return !flushing_; });
      return;
    }
    if (!fill_) return;
    flushing_ = true;
    while (free_slots_.empty()) {   // every slot busy: the oldest launch first
      std::shared_ptr<Launch> oldest = in_flight_.begin()->second;
      finish(oldest, g);
    }
    std::shared_ptr<Launch> L = fill_;   // (submissions that joined while the lock was released are part of it)
    fill_.reset();
    L->id = ++launch_seq_;
    L->segs.swap(pending_);
    L->total = pending_total_;
    pending_total_ = 0;
    L->slab = fill_slab_;
    L->slot = free_slots_.back();
    free_slots_.pop_back();
    uint32_t *first_row = nullptr;
    SegEntry *entries = nullptr;
    be_.table(L->slab, &first_row, &entries);
    for (size_t i = 0; i < L->segs.size(); i++) {
      first_row[i] = (uint32_t)L->segs[i].first_row;
      entries[i] = L->segs[i].e;
    }
    first_row[L->segs.size()] = (uint32_t)L->total;
    info_.launches++;
    if (L->total > info_.largest_launch) info_.largest_launch = L->total;
    std::string m;
    const int st = be_.enqueue(L->slot, L->slab, L->segs, L->total, &m);
    if (st == kStOk) {
      L->state = kInFlight;
      in_flight_[L->id] = L;
    } else {   // complete at once, with the error; slot and slab are free
      L->status = st;
      L->msg = m;
      L->state = kDone;
      free_slots_.push_back(L->slot);
      free_slabs_.push_back(L->slab);
    }
    // one slab more than slots, and every launch that holds a slab holds a slot: one is free
    fill_slab_ = free_slabs_.back();
    free_slabs_.pop_back();
    flushing_ = false;
    cv_.notify_all();
  }

  Backend &be_;
  const size_t max_;
  const int slots_;
  std::mutex mu_;
  std::condition_variable cv_;
  bool flushing_ = false;
  uint64_t next_ticket_ = 1, launch_seq_ = 0;
  std::vector<Segment> pending_;
  size_t pending_total_ = 0;
  std::shared_ptr<Launch> fill_;                              // the launch being filled (null when nothing is pending)
  int fill_slab_ = 0;
  std::vector<int> free_slots_, free_slabs_;
  std::map<uint64_t, std::shared_ptr<Launch>> in_flight_;     // by launch id: begin() is the oldest
  std::map<uint64_t, std::shared_ptr<Launch>> tickets_;       // outstanding tickets (null: complete at birth)
  QueueInfo info_;
};

}  // namespace hs
