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
// Query norms, screen, re-rank, fallback of one group: all enqueued, nothing read back.  rows / fmt as launch_exact_search.
hipError_t launch_exact_screen(const DevIndex &ix, const void *rows, int fmt, const ScreenArgs &a, const FilterArgs *f, hipStream_t stream);
const char *xs_kernel_name(int fmt);

}  // namespace hs
