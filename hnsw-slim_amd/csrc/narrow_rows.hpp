// narrow_rows.hpp -- what "representable" means for a narrow row format, and where an element sits in a narrow row; shared by
// the conversion kernel (narrow_rows.hip) and the host side (capi_index.cpp: hs_rows_representable, hs_index_patch).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace hs {

enum : int { ROWS_F32 = 0, ROWS_F16 = 1, ROWS_U8 = 2, ROWS_I8 = 3, ROWS_BF16 = 4, ROWS_F8 = 5 };   // hs_row_format
constexpr int kRowFormats = 6;
inline bool is_narrow_format(int fmt) { return fmt == ROWS_F16 || fmt == ROWS_U8 || fmt == ROWS_I8 || fmt == ROWS_BF16 || fmt == ROWS_F8; }
inline size_t narrow_width(int fmt) { return fmt == ROWS_U8 || fmt == ROWS_I8 || fmt == ROWS_F8 ? 1 : fmt == ROWS_F16 || fmt == ROWS_BF16 ? 2 : 0; }
// The stored form of every format is the value itself in the format's own encoding: u8 the unsigned byte, i8 the two's complement
// byte (no bias: what a caller's int8 array holds is what the copy holds), f16 the IEEE half, bf16 the upper half word of the fp32
// value (hs_bf16 below: sign, the 8 exponent bits, the top 7 fraction bits -- what a caller's bfloat16 array holds), f8 the OCP E4M3
// "fn" byte (hs_f8 below).  Every place that writes or reads a
// narrow row -- the pack kernel, the record kernel of the live updates, hs_index_patch, hs_rows_to_narrow, hs_index_get_row,
// hs_index_load_narrow -- goes through narrow_cast and a plain widening conversion of T.

// A bf16 element.  No arithmetic type: the only operations are the two below, both on bits, so the host and the device agree by
// construction and no conversion instruction, rounding mode or denormal mode is involved.
struct hs_bf16 {
  uint16_t w;
  __host__ __device__ explicit operator float() const { return __builtin_bit_cast(float, (uint32_t)w << 16); }   // exact, subnormals included
};
static_assert(sizeof(hs_bf16) == 2, "a bf16 row is dim half words");

// An fp8 element in the OCP E4M3 "fn" encoding: sign, 4 exponent bits of bias 7, 3 fraction bits; no infinities, 0x7F and 0xFF are NaN,
// exponent field 0 holds the subnormals k 2^-9 (k = 1 .. 7) and the two zeros, the largest finite value is 0x7E = 448.  Bits only, as
// hs_bf16: the widening below builds the fp32 bit pattern, so host and device agree by construction.  (The search kernels widen pairs
// with v_cvt_pk_f32_fp8, narrow_load.hpp; tests/test_gpu_f8_rows.py pins that instruction to this decode on all 256 bytes.)
struct hs_f8 {
  uint8_t w;
  __host__ __device__ explicit operator float() const {
    const uint32_t s = (uint32_t)(w & 0x80u) << 24, e = (w >> 3) & 15u, m = w & 7u;
    uint32_t b;
    if ((w & 0x7Fu) == 0x7Fu) b = 0x7FC00000u;                                        // NaN
    else if (e != 0u) b = ((e + 120u) << 23) | (m << 20);                             // 1.m 2^(e - 7)
    else if (m >= 4u) b = (120u << 23) | ((m & 3u) << 21);                            // k 2^-9, normalised: 4 .. 7 -> 1.xx 2^-7
    else if (m >= 2u) b = (119u << 23) | ((m & 1u) << 22);                            //                      2, 3  -> 1.x 2^-8
    else b = m ? (118u << 23) : 0u;                                                   //                      1     -> 2^-9; 0
    return __builtin_bit_cast(float, s | b);
  }
};
static_assert(sizeof(hs_f8) == 1, "an fp8 row is dim bytes");

// slot of element j of a row in its narrow row (lane-major: see narrow_rows.hip)
__host__ __device__ inline uint32_t narrow_slot(uint32_t j, uint32_t dim) {
  const uint32_t i = j >> 4, s = (j >> 1) & 7u, e = j & 1u;
  return s * (dim >> 3) + 2u * i + e;
}
// the element a narrow row holds in slot p: the inverse of narrow_slot (dim % 16 == 0)
__host__ __device__ inline uint32_t narrow_elem(uint32_t p, uint32_t dim) {
  const uint32_t per = dim >> 3, s = p / per, rem = p - s * per;
  return 16u * (rem >> 1) + 2u * s + (rem & 1u);
}

template <typename T> __host__ __device__ inline T narrow_cast(float x);
// (an out-of-range or NaN value must not reach the float -> integer conversion, which is undefined for it)
template <> __host__ __device__ inline uint8_t narrow_cast<uint8_t>(float x) { return (x >= 0.0f && x <= 255.0f) ? (uint8_t)x : (uint8_t)0; }
template <> __host__ __device__ inline int8_t narrow_cast<int8_t>(float x) { return (x >= -128.0f && x <= 127.0f) ? (int8_t)(int)x : (int8_t)0; }
template <> __host__ __device__ inline _Float16 narrow_cast<_Float16>(float x) { return (_Float16)x; }   // round to nearest even, overflow -> inf
// (the upper half word: the value itself where it fits -- nothing rounds; what does not fit is refused by narrow_fits)
template <> __host__ __device__ inline hs_bf16 narrow_cast<hs_bf16>(float x) { return hs_bf16{(uint16_t)(__builtin_bit_cast(uint32_t, x) >> 16)}; }
// (the E4M3 byte of a value on the grid, from the fp32 fields: exponents 2^-6 .. 2^8 are the normal bytes, 2^-9 .. 2^-7 the subnormals
//  k = 1, 2 + f, 4 + ff; fraction bits that do not fit are dropped and anything else gives 0 -- narrow_fits refuses all of those)
template <> __host__ __device__ inline hs_f8 narrow_cast<hs_f8>(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x), s = (u >> 24) & 0x80u, ex = (u >> 23) & 255u, fr = u & 0x7FFFFFu;
  uint32_t b = 0u;
  if (ex == 0u && fr == 0u) b = s;                                    // +-0 keeps its sign
  else if (ex >= 121u && ex <= 135u) b = s | ((ex - 120u) << 3) | (fr >> 20);
  else if (ex == 120u) b = s | (4u + (fr >> 21));
  else if (ex == 119u) b = s | (2u + (fr >> 22));
  else if (ex == 118u) b = s | 1u;
  return hs_f8{(uint8_t)b};
}

// Representable: x == (float)(T)x, NaN and +-inf never -- u8: the integers 0 .. 255; i8: the integers -128 .. 127; f16: every
// finite fp16 value, subnormals included.  -0.0f passes in all (-0.0f == 0.0f; u8 and i8 store 0 and read back +0.0f, f16 keeps
// the sign), and reading +0 for -0 cannot change a distance: in the L2 recipe t = q - x gives t * t = +0 for every sign
// combination of zero operands and the same t for q != 0; in the IP recipe the product q * x is +-0 either way and a +-0 added to
// an accumulator that started at +0 (fma(q, x, acc): +0 + -0 = +0 in round-to-nearest) leaves it bit-identical.
// With i8 other elements of the row may be negative, so the IP accumulator may be negative or may pass through zero; the argument
// does not lean on its sign.  The swap changes only the term of the zero element, from one signed zero to the other.  Adding a
// zero of either sign to acc != 0 returns acc.  An accumulator that is zero is +0: it starts at +0, a sum of a zero term and +0 is
// +0, an exact cancellation of non-zero operands rounds to +0 in round-to-nearest, and nothing underflows to a zero (q, acc and so
// q * x + acc for an integer x are multiples of 2^-149); -0 arises only from -0 + -0, which needs an accumulator that already is
// -0.  So acc stays bit-identical at the swapped step and hence at every later one.
// bf16: the fp32 values whose low 16 bits are zero and whose exponent is not all ones -- every finite bf16 value, subnormals (below
// 2^-126: the fp32 subnormals k 2^-133, k = 1 .. 127) and -0 included; like f16 it keeps the sign of -0, so nothing is swapped at all.
// f8: the 254 finite E4M3 values -- +-k 2^-9 (k = 0 .. 7) and +-1.m 2^e (e = -6 .. 8) up to 448; like f16 and bf16 it keeps the sign of
// -0 (0x80), so nothing is swapped and the f16 case of the argument above carries over.  A value between two grid points, above 448
// (480 would be the NaN byte), below 2^-9, NaN and +-inf do not fit.
template <typename T> __host__ __device__ inline bool narrow_fits(float x);
template <> __host__ __device__ inline bool narrow_fits<uint8_t>(float x) { return x >= 0.0f && x <= 255.0f && (float)(uint8_t)x == x; }
template <> __host__ __device__ inline bool narrow_fits<int8_t>(float x) { return x >= -128.0f && x <= 127.0f && (float)(int8_t)(int)x == x; }
template <> __host__ __device__ inline bool narrow_fits<_Float16>(float x) {
  const float y = (float)(_Float16)x;
  return y == x && y - y == 0.0f;   // (y - y is NaN for +-inf)
}
template <> __host__ __device__ inline bool narrow_fits<hs_bf16>(float x) {
  const uint32_t b = __builtin_bit_cast(uint32_t, x);
  return (b & 0xFFFFu) == 0u && (b & 0x7F800000u) != 0x7F800000u;   // (on the bits: a subnormal is not flushed on the way, NaN and +-inf have the exponent all ones)
}
template <> __host__ __device__ inline bool narrow_fits<hs_f8>(float x) {
  const hs_f8 b = narrow_cast<hs_f8>(x);   // (on the bits: the byte widens back to the very pattern of x, and is not a NaN byte)
  return (b.w & 0x7Fu) != 0x7Fu && __builtin_bit_cast(uint32_t, (float)b) == __builtin_bit_cast(uint32_t, x);
}

}  // namespace hs
