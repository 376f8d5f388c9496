// search_finish.hpp -- what every search kernel does behind its hop loop, once: the reference's k-selection on its raw result
// heap, the replay that rebuilds that heap from the insertion log when equal keys straddle a boundary, and the stats block.
// The strict kernel owns a result heap and ends in select_and_write; the fast, lean and flat kernels keep keys in registers
// and call replay_boundary for the queries whose k-subset depends on the heap's layout.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "heap_emul.hpp"
#include "wave_util.hpp"

namespace hs {

// k-selection on the reference's result heap top[0 .. ts) (libstdc++ mechanics, heap_emul.hpp): std::nth_element(top, top + k,
// top + size) (hnswalg_slim.h:2126-2130) for mode 0, while (size > k) pop_heap (hnswalg_slim.h:2019-2022, hnswalg.h:1430-1432)
// otherwise; then result slot i = top[i] for the `valid` = min(ts, k) first slots, padding behind them.  (The count is an argument:
// every caller holds it already, and derived here from the size the replay's loop carries it costs the flat kernels 4 to 8 bytes
// of scratch per lane.)  FULL: the caller has shown ts >= k, so every slot is valid -- no guard, no padding (the fast kernel, whose
// any-dim bodies sit at the inliner's threshold: with the guard one of them is no longer inlined into its kernel).
template <bool FULL = false>
__device__ __forceinline__ void select_and_write(const DevIndex &ix, const SearchArgs &a, uint32_t qi, Pair *top, uint32_t ts, uint32_t valid, int lane) {
  const uint32_t k = a.k;
  if (lane == 0) {
    if (a.mode == 0) {
      if (FULL || ts >= k) nth_element(top, (long)k, (long)ts, LessD());
    } else {
      for (uint32_t t = ts; t > k; t--) pop_heap(top, (long)t, LessD());
    }
  }
  wave_sync();
  for (uint32_t i = lane; i < k; i += 64) {
    const bool v = FULL || i < valid;
    const Pair p = v ? top[i] : Pair{__builtin_inff(), 0};
    const uint64_t label = v ? ix.labels[p.id] : ~0ull;
    if (a.out_labels32) a.out_labels32[(size_t)qi * k + i] = v ? (uint32_t)label : 0xFFFFFFFFu;  // size_t -> tableint truncation (:2129)
    if (a.out_labels64) a.out_labels64[(size_t)qi * k + i] = label;
    if (a.out_dists) a.out_dists[(size_t)qi * k + i] = p.d;
  }
}

// The reference's result heap rebuilt exactly: the n_log logged insertions (distance bits, id) replayed through libstdc++'s
// push_heap / pop_heap (hnswalg_slim.h:419-448) into top[0 .. ef], then select_and_write.  The caller has made the log visible
// to the wave (it was written by this wave: __threadfence_block) and checked that it holds every insertion; valid = min(n_log, ef, k).
template <bool FULL = false>
__device__ __forceinline__ void replay_boundary(const DevIndex &ix, const SearchArgs &a, uint32_t qi, Pair *top, const uint2 *tlog,
                                                uint32_t n_log, uint32_t valid, int lane) {
  const uint32_t ef = a.ef;
  uint32_t ts = 0;
  for (uint32_t base = 0; base < n_log; base += 64) {
    const uint32_t m = min(64u, n_log - base);
    uint2 e = make_uint2(0, 0);
    if ((uint32_t)lane < m) e = tlog[base + lane];
    for (uint32_t j = 0; j < m; j++) {
      const float d = __uint_as_float(__builtin_amdgcn_readlane(e.x, j));
      const uint32_t nb = __builtin_amdgcn_readlane(e.y, j);
      if (lane == 0) {
        top[ts].d = d;  // :419-423
        top[ts].id = nb;
        push_heap(top, (long)ts + 1, LessD());
        if (ts + 1 > ef) pop_heap(top, (long)ts + 1, LessD());  // :434-448
      }
      ts = min(ts + 1, ef);
    }
  }
  select_and_write<FULL>(ix, a, qi, top, ts, valid, lane);
}

// The four-word stats block of a finished query and its status (one lane).  `mark`: the pass that answered the query, or 1 for
// "answered by the boundary replay".
__device__ __forceinline__ void write_stats(const SearchArgs &a, uint32_t qi, uint32_t n_dist, uint32_t n_hops, uint32_t n_nbr, uint32_t mark) {
  if (a.stats) {
    a.stats[qi * 4 + 0] = n_dist;
    a.stats[qi * 4 + 1] = n_hops;
    a.stats[qi * 4 + 2] = n_nbr;
    a.stats[qi * 4 + 3] = mark;
  }
  a.status[qi] = ST_DONE;
}

}  // namespace hs
