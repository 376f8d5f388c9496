// exact_screen_rows.hpp -- what the fp32 MFMA screens (exact_screen.hip, exact_range_screen.hip) share on the device: how a row of
// any of the six formats reaches the matrix operand in stored order, how the query tile is staged to match, and the recipe distance
// of one (query, row) pair with the scan's own loads and accumulation order.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "bf_common.hpp"
#include "exact_screen_engine.hpp"
#include "narrow_load.hpp"
#include "narrow_rows.hpp"

namespace hs {

typedef float xs_f16v __attribute__((ext_vector_type(16)));

// the dim index stored at position p of a row: identity for fp32 rows, the inverse of narrow_slot for the narrow copy
template <typename ROW>
__device__ __forceinline__ uint32_t xs_dim_at(uint32_t p, uint32_t dim) {
  if constexpr (!RowKind<ROW>::narrow) return p;
  const uint32_t per = dim >> 3, s = p / per, rem = p - s * per;
  return 16u * (rem >> 1) + 2u * s + (rem & 1u);
}

// four stored values of a row at position 8 cc + 4 h, as loaded and widened
template <typename ROW> struct XsChunk;
template <> struct XsChunk<float> {
  float4 w;
  __device__ __forceinline__ void load(const float *row, uint32_t h, uint32_t cc) { w = reinterpret_cast<const float4 *>(row)[2 * cc + h]; }
  __device__ __forceinline__ float4 wide() const { return w; }
};
template <> struct XsChunk<uint8_t> {
  uint32_t w;
  __device__ __forceinline__ void load(const uint8_t *row, uint32_t h, uint32_t cc) { w = reinterpret_cast<const uint32_t *>(row)[2 * cc + h]; }
  __device__ __forceinline__ float4 wide() const {
    const hs_f2 a = narrow_pair((const uint8_t *)nullptr, &w, 0), b = narrow_pair((const uint8_t *)nullptr, &w, 1);
    return make_float4(a.x, a.y, b.x, b.y);
  }
};
template <> struct XsChunk<int8_t> {
  uint32_t w;
  __device__ __forceinline__ void load(const int8_t *row, uint32_t h, uint32_t cc) { w = reinterpret_cast<const uint32_t *>(row)[2 * cc + h]; }
  __device__ __forceinline__ float4 wide() const {
    const hs_f2 a = narrow_pair((const int8_t *)nullptr, &w, 0), b = narrow_pair((const int8_t *)nullptr, &w, 1);
    return make_float4(a.x, a.y, b.x, b.y);
  }
};
template <> struct XsChunk<hs_f8> {
  uint32_t w;
  __device__ __forceinline__ void load(const hs_f8 *row, uint32_t h, uint32_t cc) { w = reinterpret_cast<const uint32_t *>(row)[2 * cc + h]; }
  __device__ __forceinline__ float4 wide() const {
    const hs_f2 a = f8_pair(w, false), b = f8_pair(w, true);
    return make_float4(a.x, a.y, b.x, b.y);
  }
};
template <> struct XsChunk<_Float16> {
  uint32_t w[2];
  __device__ __forceinline__ void load(const _Float16 *row, uint32_t h, uint32_t cc) {
    const uint2 v = reinterpret_cast<const uint2 *>(row)[2 * cc + h];
    w[0] = v.x; w[1] = v.y;
  }
  __device__ __forceinline__ float4 wide() const {
    const hs_f2 a = narrow_pair((const _Float16 *)nullptr, w, 0), b = narrow_pair((const _Float16 *)nullptr, w, 1);
    return make_float4(a.x, a.y, b.x, b.y);
  }
};
template <> struct XsChunk<hs_bf16> {
  uint32_t w[2];
  __device__ __forceinline__ void load(const hs_bf16 *row, uint32_t h, uint32_t cc) {
    const uint2 v = reinterpret_cast<const uint2 *>(row)[2 * cc + h];
    w[0] = v.x; w[1] = v.y;
  }
  __device__ __forceinline__ float4 wide() const {
    const hs_f2 a = bf16_pair(w[0]), b = bf16_pair(w[1]);
    return make_float4(a.x, a.y, b.x, b.y);
  }
};

// Positions [p0, p0 + len) of the tile's queries into LDS in operand layout: [len / 8][2][64 queries][4].
template <typename ROW>
__device__ __forceinline__ void xs_stage(float *qL, const uint32_t *slot_q, const float *queries, uint32_t dim, uint32_t p0, uint32_t len, int tid) {
  for (uint32_t i = tid; i < kXsTile * len; i += 256) {
    const uint32_t t = i / len, pos = i - t * len, qi = slot_q[t];
    const float v = qi != kXsNoSlot ? queries[(size_t)qi * dim + xs_dim_at<ROW>(p0 + pos, dim)] : 0.f;
    qL[(((pos >> 3) * 2 + ((pos >> 2) & 1u)) * kXsTile + t) * 4 + (pos & 3u)] = v;
  }
}

// The recipe's distance of the query in LDS to row `at / dim`, four lanes per row: the loads and the accumulation order of
// exact_search.hip's exact_scan_body for one query, so the bits are its bits.
template <int METRIC, typename ROW>
__device__ __forceinline__ float xs_recipe_dist(const float *q, const void *rows, size_t at, uint32_t dim, int sub, bool &owner) {
  const uint32_t steps = dim >> 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (RowKind<ROW>::narrow) {
    const ROW *ca = static_cast<const ROW *>(rows) + at + (uint32_t)sub * (dim >> 2), *cb = ca + 2 * steps;
    const bool aligned4 = sizeof(ROW) == 2 || !(steps & 1u);
    for (uint32_t s0 = 0; s0 < steps; s0 += 8) {
      const uint32_t nb = min(8u, steps - s0);
      const uint32_t nw = aligned4 ? (nb & ~3u) : 0u;
      NarrowRound<ROW> ra, rc;
      ra.load(ca + 2 * s0, nb, nw);
      rc.load(cb + 2 * s0, nb, nw);
#pragma unroll
      for (uint32_t i = 0; i < 8; i++)
        if (i < nb) {
          const hs_f2 xa = ra.pair(i, nw), xb = rc.pair(i, nw);
          const float4 xv = make_float4(xa.x, xa.y, xb.x, xb.y);
          const float4 qv = *reinterpret_cast<const float4 *>(q + (s0 + i) * 16 + sub * 4);
          step4<METRIC>(acc, qv, xv);
        }
    }
  } else {
    const float4 *x = reinterpret_cast<const float4 *>(static_cast<const float *>(rows) + at) + sub;
    for (uint32_t st = 0; st < steps; st++) {
      const float4 xv = x[st * 4];
      const float4 qv = *reinterpret_cast<const float4 *>(q + st * 16 + sub * 4);
      step4<METRIC>(acc, qv, xv);
    }
  }
  return lane4_reduce<METRIC>(acc, sub, owner);
}

}  // namespace hs
