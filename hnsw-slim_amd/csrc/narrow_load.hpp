// narrow_load.hpp -- device-side reads of an index's narrow (u8 / i8 / fp16 / bf16 / fp8) row copy: which rows a kernel instantiation reads, and
// the exact widening of stored element pairs.  Shared by flat_search.hip (8 lanes per row) and beam_search.hip (4 lanes per row).
// Layout and conversion: narrow_rows.hpp / narrow_rows.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine.hpp"
#include "narrow_rows.hpp"
#include "wave_util.hpp"

namespace hs {

template <typename ROW> struct RowKind { static constexpr bool narrow = true; };
template <> struct RowKind<float> { static constexpr bool narrow = false; };
typedef uint32_t hs_u4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t hs_u2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef _Float16 hs_h2 __attribute__((ext_vector_type(2)));

// The rows a strict / fast kernel instantiation reads.  ROW = float: the resident fp32 rows, taken from the DevIndex (the struct is
// empty, so the fp32 kernels carry no extra argument and compile to what they were).  ROW = uint8_t / int8_t / _Float16 / hs_bf16 / hs_f8: the base of the
// narrow copy, a kernel argument of its own (DevIndex keeps its layout).
template <typename ROW> struct RowSrc { const ROW *p; };
template <> struct RowSrc<float> {};

// element pair i of a lane's chunk, widened: a u8 or i8 pair is half a dword (v_cvt_f32_ubyteN; i8 below), an f16 pair one dword
// (v_cvt_f32_f16)
__device__ __forceinline__ hs_f2 narrow_pair(const uint8_t *, const uint32_t *dw, int i) {
  const uint32_t w = dw[i >> 1] >> ((i & 1) * 16);
  return hs_f2{(float)(w & 0xFFu), (float)((w >> 8) & 0xFFu)};
}
__device__ __forceinline__ hs_f2 narrow_pair(const _Float16 *, const uint32_t *dw, int i) {
  const hs_h2 h = __builtin_bit_cast(hs_h2, dw[i]);
  return hs_f2{(float)h.x, (float)h.y};
}
// A signed byte (two's complement, narrow_rows.hpp) has no v_cvt_f32_ubyteN.  Neither a v_bfe_i32 in front of the conversion nor a
// biased byte with a subtract behind it is needed on gfx950: the conversion's sub-dword operand select extends the sign itself,
//   v_cvt_f32_i32_sdwa v, sext(w) src0_sel:BYTE_n
// which is what the compiler makes of (float)(int8_t)(w >> 8 n): one instruction per element, as for u8.  Exact: the operand is
// the integer the byte stands for, |v| <= 128 < 2^24, and every such integer is an fp32 value.
__device__ __forceinline__ hs_f2 i8_pair(uint32_t h) { return hs_f2{(float)(int)(int8_t)h, (float)(int)(int8_t)(h >> 8)}; }   // bytes 0 and 1 of h
__device__ __forceinline__ hs_f2 narrow_pair(const int8_t *, const uint32_t *dw, int i) {
  const uint32_t w = dw[i >> 1];
  return (i & 1) ? hs_f2{(float)(int)(int8_t)(w >> 16), (float)((int)w >> 24)} : i8_pair(w);
}
// A bf16 pair is one dword w, the low element in its low half word: the fp32 values are w << 16 and w & 0xFFFF0000, reinterpreted --
// one VALU instruction per element (v_lshlrev_b32, v_and_b32) and no v_cvt.  Exact by construction: a bf16 element IS the upper half of
// an fp32 value whose lower half is zero (narrow_rows.hpp), so the register holds the very bit pattern the fp32 row holds.  No
// conversion runs, hence no rounding and no denormal mode: a subnormal (below 2^-126) and -0 arrive as the fp32 kernel reads them, and
// what the recipe then does with them is the fp32 kernel's own arithmetic.
__device__ __forceinline__ hs_f2 bf16_pair(uint32_t w) { return hs_f2{__uint_as_float(w << 16), __uint_as_float(w & 0xFFFF0000u)}; }
__device__ __forceinline__ hs_f2 narrow_pair(const hs_bf16 *, const uint32_t *dw, int i) { return bf16_pair(dw[i]); }
// An fp8 (E4M3) pair is half a dword, as a u8 pair: v_cvt_pk_f32_fp8 widens both elements of the selected half word in ONE instruction
// (the u8 / i8 kernels spend one conversion per element).  Exact: every E4M3 value, subnormals included, is a normal fp32 value, so no
// denormal mode enters; 0x80 gives -0.0f.  (hs_f8's own operator float is the decode on the bits the host uses; the two agree on all
// 256 bytes -- tests/test_gpu_f8_rows.py.)
// HS_F8_SINGLE (set by an object before this header): one v_cvt_f32_fp8 per element instead, for the kernels in which the aligned
// register pair of the packed form costs scratch (flat_search_f8.hip); the same values.
__device__ __forceinline__ hs_f2 f8_pair(uint32_t w, bool hi) {
#ifdef HS_F8_SINGLE
  return hi ? hs_f2{__builtin_amdgcn_cvt_f32_fp8((int)w, 2), __builtin_amdgcn_cvt_f32_fp8((int)w, 3)}
            : hs_f2{__builtin_amdgcn_cvt_f32_fp8((int)w, 0), __builtin_amdgcn_cvt_f32_fp8((int)w, 1)};
#else
  return hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
#endif
}
__device__ __forceinline__ hs_f2 narrow_pair(const hs_f8 *, const uint32_t *dw, int i) { return f8_pair(dw[i >> 1], i & 1); }
__device__ __forceinline__ hs_f2 narrow_pair_at(const uint8_t *chunk, uint32_t i) {
  const uint32_t w = *reinterpret_cast<const unsigned short *>(chunk + 2 * i);
  return hs_f2{(float)(w & 0xFFu), (float)(w >> 8)};
}
__device__ __forceinline__ hs_f2 narrow_pair_at(const int8_t *chunk, uint32_t i) {
  return i8_pair(*reinterpret_cast<const unsigned short *>(chunk + 2 * i));
}
__device__ __forceinline__ hs_f2 narrow_pair_at(const _Float16 *chunk, uint32_t i) {
  const hs_h2 h = *reinterpret_cast<const hs_h2 *>(chunk + 2 * i);
  return hs_f2{(float)h.x, (float)h.y};
}
__device__ __forceinline__ hs_f2 narrow_pair_at(const hs_f8 *chunk, uint32_t i) {
  return f8_pair(*reinterpret_cast<const unsigned short *>(chunk + 2 * i), false);
}
__device__ __forceinline__ hs_f2 narrow_pair_at(const hs_bf16 *chunk, uint32_t i) {
  return bf16_pair(*reinterpret_cast<const uint32_t *>(chunk + 2 * i));
}

// One round of a lane's chunk at a runtime dim: up to eight consecutive element pairs, held as they were loaded and widened on use.
// load(c, nb, nw): pairs [0, nw) -- nw = 0, 4 or 8, at most nb, and only where c is dword aligned -- arrive in one 16-byte load
// (u8 / i8: eight pairs; fp16 / bf16: four, so two loads for eight) or one 8-byte load (u8 / i8: four pairs); pairs [nw, nb) in one load each
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
// i8: the bytes arrive as the u8 round's do (the same 16-, 8- and 2-byte loads); only the widening differs
template <> struct NarrowRound<int8_t> : NarrowRound<uint8_t> {
  __device__ __forceinline__ void load(const int8_t *c, uint32_t nb, uint32_t nw) {
    NarrowRound<uint8_t>::load(reinterpret_cast<const uint8_t *>(c), nb, nw);
  }
  __device__ __forceinline__ hs_f2 pair(uint32_t i, uint32_t nw) const {
    return i8_pair(i < nw ? w[i >> 1] >> ((i & 1u) * 16u) : p[i]);
  }
};
// fp8: the bytes arrive as the u8 round's do; a pair is widened by one v_cvt_pk_f32_fp8
template <> struct NarrowRound<hs_f8> : NarrowRound<uint8_t> {
  __device__ __forceinline__ void load(const hs_f8 *c, uint32_t nb, uint32_t nw) {
    NarrowRound<uint8_t>::load(reinterpret_cast<const uint8_t *>(c), nb, nw);
  }
  __device__ __forceinline__ hs_f2 pair(uint32_t i, uint32_t nw) const {
    return f8_pair(i < nw ? w[i >> 1] >> ((i & 1u) * 16u) : p[i], false);   // (the half word first, as the u8 round: one conversion, not one per source)
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
// bf16: the half words arrive as the fp16 round's do (the same 16- and 4-byte loads); only the widening differs
template <> struct NarrowRound<hs_bf16> : NarrowRound<_Float16> {
  __device__ __forceinline__ void load(const hs_bf16 *c, uint32_t nb, uint32_t nw) {
    NarrowRound<_Float16>::load(reinterpret_cast<const _Float16 *>(c), nb, nw);
  }
  __device__ __forceinline__ hs_f2 pair(uint32_t i, uint32_t) const { return bf16_pair(w[i]); }
};

}  // namespace hs
