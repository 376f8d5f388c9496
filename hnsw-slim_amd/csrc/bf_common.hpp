// bf_common.hpp -- what the exhaustive scans share (brute_force.hip over a bare fp32 array, exact_search.hip over the rows of a
// resident index): the workgroup geometry, the entry of a sorted k-list and the insertion of one pass's candidates into it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wave_util.hpp"

namespace hs {

static constexpr int kQT = 8;       // queries per workgroup tile
static constexpr int kWaves = 4;    // waves per workgroup

struct BfEntry { float d; uint32_t row; uint64_t label; };   // 16 bytes

__device__ __forceinline__ bool bf_less(float d, uint64_t l, const BfEntry &e) { return d < e.d || (d == e.d && l < e.label); }

// Candidates of one pass (mask m, value d in the owning lane, row = rb + (lane >> SHIFT)) against one query's sorted k-list.
template <int SHIFT>
__device__ __forceinline__ void bf_offer(unsigned long long m, float d, uint32_t rb, const uint64_t *labels, BfEntry *L, uint32_t *sz,
                                         uint32_t k, int lane) {
  while (m) {
    const int l = __ffsll((long long)m) - 1;
    m &= m - 1;
    const float dj = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(d), l));
    const uint32_t rj = rb + (uint32_t)(l >> SHIFT);
    if (lane == 0) {
      const uint64_t lab = labels ? labels[rj] : (uint64_t)rj;
      uint32_t cur = *sz;
      if (cur < k || bf_less(dj, lab, L[k - 1])) {
        uint32_t pos = cur < k ? cur : k - 1;
        while (pos > 0 && bf_less(dj, lab, L[pos - 1])) { L[pos] = L[pos - 1]; pos--; }
        L[pos] = BfEntry{dj, rj, lab};
        if (cur < k) *sz = cur + 1;
      }
    }
    wave_sync();
  }
}

}  // namespace hs
