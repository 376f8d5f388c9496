// narrow_load.hpp -- device-side reads of an index's narrow (u8 / fp16) row copy: which rows a kernel instantiation reads, and
// the exact widening of stored element pairs.  Shared by flat_search.hip (8 lanes per row) and beam_search.hip (4 lanes per row).
// Layout and conversion: narrow_rows.hpp / narrow_rows.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine.hpp"
#include "wave_util.hpp"

namespace hs {

template <typename ROW> struct RowKind { static constexpr bool narrow = true; };
template <> struct RowKind<float> { static constexpr bool narrow = false; };
typedef uint32_t hs_u4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t hs_u2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef _Float16 hs_h2 __attribute__((ext_vector_type(2)));

// The rows a strict / fast kernel instantiation reads.  ROW = float: the resident fp32 rows, taken from the DevIndex (the struct is
// empty, so the fp32 kernels carry no extra argument and compile to what they were).  ROW = uint8_t / _Float16: the base of the
// narrow copy, a kernel argument of its own (DevIndex keeps its layout).
template <typename ROW> struct RowSrc { const ROW *p; };
template <> struct RowSrc<float> {};

// element pair i of a lane's chunk, widened: a u8 pair is half a dword (v_cvt_f32_ubyteN), an f16 pair one dword (v_cvt_f32_f16)
__device__ __forceinline__ hs_f2 narrow_pair(const uint8_t *, const uint32_t *dw, int i) {
  const uint32_t w = dw[i >> 1] >> ((i & 1) * 16);
  return hs_f2{(float)(w & 0xFFu), (float)((w >> 8) & 0xFFu)};
}
__device__ __forceinline__ hs_f2 narrow_pair(const _Float16 *, const uint32_t *dw, int i) {
  const hs_h2 h = __builtin_bit_cast(hs_h2, dw[i]);
  return hs_f2{(float)h.x, (float)h.y};
}
__device__ __forceinline__ hs_f2 narrow_pair_at(const uint8_t *chunk, uint32_t i) {
  const uint32_t w = *reinterpret_cast<const unsigned short *>(chunk + 2 * i);
  return hs_f2{(float)(w & 0xFFu), (float)(w >> 8)};
}
__device__ __forceinline__ hs_f2 narrow_pair_at(const _Float16 *chunk, uint32_t i) {
  const hs_h2 h = *reinterpret_cast<const hs_h2 *>(chunk + 2 * i);
  return hs_f2{(float)h.x, (float)h.y};
}

// One round of a lane's chunk at a runtime dim: up to eight consecutive element pairs, held as they were loaded and widened on use.
// load(c, nb, nw): pairs [0, nw) -- nw = 0, 4 or 8, at most nb, and only where c is dword aligned -- arrive in one 16-byte load
// (u8: eight pairs; fp16: four, so two loads for eight) or one 8-byte load (u8: four pairs); pairs [nw, nb) in one load each
// (2 / 4 bytes).  Nothing beyond pair nb is touched.  pair(i, nw) widens pair i < nb, with the nw that load() was given.
template <typename ROW> struct NarrowRound;
template <> struct NarrowRound<uint8_t> {
  uint32_t w[4], p[8];
  __device__ __forceinline__ void load(const uint8_t *c, uint32_t nb, uint32_t nw) {
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = 0;
    if (nw == 8) {
      const hs_u4_a4 v = *reinterpret_cast<const hs_u4_a4 *>(c);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if (nw == 4) {
      const hs_u2_a4 v = *reinterpret_cast<const hs_u2_a4 *>(c);
      w[0] = v.x; w[1] = v.y;
    }
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
      p[i] = 0;
      if (i >= nw && i < nb) p[i] = *reinterpret_cast<const unsigned short *>(c + 2 * i);
    }
  }
  __device__ __forceinline__ hs_f2 pair(uint32_t i, uint32_t nw) const {
    const uint32_t h = i < nw ? w[i >> 1] >> ((i & 1u) * 16u) : p[i];
    return hs_f2{(float)(h & 0xFFu), (float)((h >> 8) & 0xFFu)};
  }
};
template <> struct NarrowRound<_Float16> {
  uint32_t w[8];   // pair i is dword i, whichever load brought it
  __device__ __forceinline__ void load(const _Float16 *c, uint32_t nb, uint32_t nw) {
    const uint32_t *cp = reinterpret_cast<const uint32_t *>(c);
    if (nw >= 4) {
      const hs_u4_a4 v = *reinterpret_cast<const hs_u4_a4 *>(cp);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    if (nw == 8) {
      const hs_u4_a4 v = *reinterpret_cast<const hs_u4_a4 *>(cp + 4);
      w[4] = v.x; w[5] = v.y; w[6] = v.z; w[7] = v.w;
    }
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
      if (i >= nw) w[i] = 0;
      if (i >= nw && i < nb) w[i] = cp[i];
    }
  }
  __device__ __forceinline__ hs_f2 pair(uint32_t i, uint32_t) const {
    const hs_h2 h = __builtin_bit_cast(hs_h2, w[i]);
    return hs_f2{(float)h.x, (float)h.y};
  }
};

}  // namespace hs
