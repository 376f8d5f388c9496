// narrow_rows.hpp -- what "representable" means for a narrow row format, and where an element sits in a narrow row; shared by
// the conversion kernel (narrow_rows.hip) and the host side (capi_index.cpp: hs_rows_representable, hs_index_patch).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace hs {

enum : int { ROWS_F32 = 0, ROWS_F16 = 1, ROWS_U8 = 2, ROWS_I8 = 3, ROWS_BF16 = 4 };   // hs_row_format
constexpr int kRowFormats = 5;
inline bool is_narrow_format(int fmt) { return fmt == ROWS_F16 || fmt == ROWS_U8 || fmt == ROWS_I8 || fmt == ROWS_BF16; }
inline size_t narrow_width(int fmt) { return fmt == ROWS_U8 || fmt == ROWS_I8 ? 1 : fmt == ROWS_F16 || fmt == ROWS_BF16 ? 2 : 0; }
// The stored form of every format is the value itself in the format's own encoding: u8 the unsigned byte, i8 the two's complement
// byte (no bias: what a caller's int8 array holds is what the copy holds), f16 the IEEE half, bf16 the upper half word of the fp32
// value (hs_bf16 below: sign, the 8 exponent bits, the top 7 fraction bits -- what a caller's bfloat16 array holds).  Every place that writes or reads a
// narrow row -- the pack kernel, the record kernel of the live updates, hs_index_patch, hs_rows_to_narrow, hs_index_get_row,
// hs_index_load_narrow -- goes through narrow_cast and a plain widening conversion of T.

// A bf16 element.  No arithmetic type: the only operations are the two below, both on bits, so the host and the device agree by
// construction and no conversion instruction, rounding mode or denormal mode is involved.
struct hs_bf16 {
  uint16_t w;
  __host__ __device__ explicit operator float() const { return __builtin_bit_cast(float, (uint32_t)w << 16); }   // exact, subnormals included
};
static_assert(sizeof(hs_bf16) == 2, "a bf16 row is dim half words");

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

}  // namespace hs
