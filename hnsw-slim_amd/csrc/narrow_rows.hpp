// narrow_rows.hpp -- what "representable" means for a narrow row format, and where an element sits in a narrow row; shared by
// the conversion kernel (narrow_rows.hip) and the host side (capi_index.cpp: hs_rows_representable, hs_index_patch).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace hs {

enum : int { ROWS_F32 = 0, ROWS_F16 = 1, ROWS_U8 = 2 };   // hs_row_format
inline size_t narrow_width(int fmt) { return fmt == ROWS_U8 ? 1 : fmt == ROWS_F16 ? 2 : 0; }

// slot of element j of a row in its narrow row (lane-major: see narrow_rows.hip)
__host__ __device__ inline uint32_t narrow_slot(uint32_t j, uint32_t dim) {
  const uint32_t i = j >> 4, s = (j >> 1) & 7u, e = j & 1u;
  return s * (dim >> 3) + 2u * i + e;
}

template <typename T> __host__ __device__ inline T narrow_cast(float x);
// (an out-of-range or NaN value must not reach the float -> integer conversion, which is undefined for it)
template <> __host__ __device__ inline uint8_t narrow_cast<uint8_t>(float x) { return (x >= 0.0f && x <= 255.0f) ? (uint8_t)x : (uint8_t)0; }
template <> __host__ __device__ inline _Float16 narrow_cast<_Float16>(float x) { return (_Float16)x; }   // round to nearest even, overflow -> inf

// Representable: x == (float)(T)x, NaN and +-inf never -- u8: the integers 0 .. 255; f16: every finite fp16 value, subnormals
// included.  -0.0f passes in both (-0.0f == 0.0f; u8 stores 0 and reads back +0.0f, f16 keeps the sign), and reading +0 for -0
// cannot change a distance: in the L2 recipe t = q - x gives t * t = +0 for every sign combination of zero operands and the
// same t for q != 0; in the IP recipe the product q * x is +-0 either way and a +-0 added to an accumulator that started at +0
// (fma(q, x, acc): +0 + -0 = +0 in round-to-nearest) leaves it bit-identical.
template <typename T> __host__ __device__ inline bool narrow_fits(float x);
template <> __host__ __device__ inline bool narrow_fits<uint8_t>(float x) { return x >= 0.0f && x <= 255.0f && (float)(uint8_t)x == x; }
template <> __host__ __device__ inline bool narrow_fits<_Float16>(float x) {
  const float y = (float)(_Float16)x;
  return y == x && y - y == 0.0f;   // (y - y is NaN for +-inf)
}

}  // namespace hs
