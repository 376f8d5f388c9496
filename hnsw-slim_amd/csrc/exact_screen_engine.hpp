// exact_screen_engine.hpp -- launch interface of the screened exact search (exact_screen.hip): a matrix-core screen with a proven
// margin, a re-rank in the reference's arithmetic, and per query the scan of exact_search.hip where the screen cannot decide.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exact_engine.hpp"

namespace hs {

static constexpr uint32_t kXsTile = 64;       // queries per workgroup tile
static constexpr uint32_t kXsSlack = 16;      // a candidate list holds k + kXsSlack entries
static constexpr uint32_t kXsStateWords = 8;  // state[0]: flagged queries of the launch group, [1]: of the call, [2..3]: re-ranked rows (u64)

static constexpr uint32_t kXsNoSlot = 0xFFFFFFFFu;

// What the screens (exact_screen.hip, exact_screen_q8.hip) hand to the re-rank: per (query, row chunk, unit parity) a list of rows
// whose distance interval [lo, hi] the chunk's bound has not ruled out.
struct XsCand { float hi, lo; uint32_t row; };   // 12 bytes
__host__ __device__ inline uint32_t xs_cap(uint32_t k) { return k + kXsSlack; }
// candidate workspace: nq x nruns lists of cap entries, then nq x nruns sizes
__host__ __device__ inline size_t xs_hdr_offset(uint32_t nq, uint32_t nruns, uint32_t cap) { return (size_t)nq * nruns * cap * sizeof(XsCand); }

// One survivor into a list sorted by hi (lane 0 only).  A full list first drops what its bound has ruled out since; an insertion into
// a full list of live entries flags the query.
__device__ __forceinline__ void xs_insert(XsCand *L, uint32_t *sz, float *U, uint32_t *flag, uint32_t k, uint32_t cap, float hi, float lo, uint32_t row) {
  if (*flag || !(lo <= *U)) return;
  uint32_t n = *sz;
  if (n == cap) {
    const float u = *U;
    uint32_t w = 0;
    for (uint32_t i = 0; i < n; i++)
      if (L[i].lo <= u) L[w++] = L[i];
    n = w;
    if (n == cap) { *flag = 1; return; }
  }
  uint32_t pos = n;
  while (pos > 0 && hi < L[pos - 1].hi) { L[pos] = L[pos - 1]; pos--; }
  L[pos] = XsCand{hi, lo, row};
  n++;
  *sz = n;
  *U = n >= k ? L[k - 1].hi : INFINITY;
}

// One launch group.  x: the exact scan's arguments -- queries, outputs, `order` (the screen's tile slots, nullable), and the
// fallback's workspace and geometry (partial, grid_x, rows_per_block as bf_partial_bytes plans them).
struct ScreenArgs {
  ExactArgs x;
  float *xnorm2, *qnorm2;   // ix.n words, written by launch_exact_screen_norms once per call; x.nq words, written per group
  void *cand;               // xs_plan() bytes: the candidate lists of every (query, row chunk, unit parity)
  uint32_t grid_x, rows_per_block;
  uint32_t *state;          // kXsStateWords
  bool first_group;         // of the call: its totals, state[1..3], start at zero
  uint32_t *qflag;          // x.nq words: the query falls back
  uint32_t *fb_order;       // x.nq words: the flagged queries first, 0xFFFFFFFF behind them
};

// Positions of the query tile staged in LDS at a time: dim where the whole tile fits the on-chip memory, else slices of 128.
uint32_t xs_slice(uint32_t dim, uint32_t k);
// Dynamic LDS of the screen kernel: the tile (or a slice of it) in operand layout, its norms and slots, two candidate lists per query.
size_t xs_screen_lds_bytes(uint32_t dim, uint32_t k);
// dim % 16 == 0, dim <= 4096, 1 <= k <= 64; anything else is the existing entry's.
bool xs_supported(uint32_t dim, uint32_t k);
// Geometry of the screen (row chunks, a multiple of 64 rows each) and the bytes of `cand`.
size_t xs_plan(uint32_t n, uint32_t nq, uint32_t k, uint32_t *grid_x, uint32_t *rows_per_block);
// |x|^2 of every row the index holds, once per call, ahead of its launch groups.
hipError_t launch_exact_screen_norms(const DevIndex &ix, const void *rows, int fmt, float *xnorm2, hipStream_t stream);
// |q|^2 of nq fp32 queries by the same kernel.
hipError_t launch_exact_screen_qnorms(const float *queries, uint32_t nq, uint32_t dim, float *qnorm2, hipStream_t stream);
// Query norms, screen, re-rank, fallback of one group: all enqueued, nothing read back.  rows / fmt as launch_exact_search.
hipError_t launch_exact_screen(const DevIndex &ix, const void *rows, int fmt, const ScreenArgs &a, const FilterArgs *f, hipStream_t stream);
const char *xs_kernel_name(int fmt);
// The two ends of a group that every screen shares: the clearing of state, flags and fallback order ahead of it; behind it the re-rank
// of the lists in `a.cand` over a.x.queries and the scan of the flagged queries.
hipError_t launch_exact_screen_init(const ScreenArgs &a, hipStream_t stream);
hipError_t launch_exact_screen_finish(const DevIndex &ix, const void *rows, int fmt, const ScreenArgs &a, const FilterArgs *f, hipStream_t stream);

}  // namespace hs
