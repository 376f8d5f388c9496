// build_rows.hpp -- how the batched build's kernels (build_gpu.hip) read a row array of any element type: fp32, or u8 / fp16 in
// NATURAL (row-major) order, as hs_build_hnsw_batched_rows takes them.  u8 -> fp32 and fp16 -> fp32 are exact, and
// everything behind the read is the fp32 text on the widened values, so a build over narrow rows writes the bytes of the fp32 build
// of the widened rows.  (The lane-major layout of narrow_rows.hip is an index's private copy and is not read here.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hs {

// One element, widened (the copy of a row into LDS, the general recipes).  u8 has no -0.0; fp16's -0.0 widens to -0.0f, which is
// what the fp32 build of the widened rows reads: nothing to treat specially.
__device__ __forceinline__ float row_widen(float v) { return v; }
__device__ __forceinline__ float row_widen(uint8_t v) { return (float)v; }     // v_cvt_f32_ubyte0
__device__ __forceinline__ float row_widen(_Float16 v) { return (float)v; }    // v_cvt_f32_f16

// The row as dist_recipe.hpp's general recipes take it (one lane per row, any dim): element i widened on the read, one element per
// load -- a row of odd dim starts at an odd byte (u8) or an odd 2-byte word (fp16), and an element load is aligned at every row.
template <class ROW>
struct RowRead {
  const ROW *p;
  __device__ __forceinline__ float operator[](uint32_t i) const { return row_widen(p[i]); }
  __device__ __forceinline__ RowRead operator+(uint32_t k) const { return RowRead{p + k}; }
};
__device__ __forceinline__ const float *row_read(const float *p) { return p; }   // (fp32: the pointer itself, as it always was)
__device__ __forceinline__ RowRead<uint8_t> row_read(const uint8_t *p) { return RowRead<uint8_t>{p}; }
__device__ __forceinline__ RowRead<_Float16> row_read(const _Float16 *p) { return RowRead<_Float16>{p}; }

// A lane's four consecutive elements of one 16-element step (dim % 16 == 0: every row starts at a multiple of 16 elements, so the
// address is aligned to the load), held as loaded and widened on use, so that a round of eight loads is in flight before any
// arithmetic: fp32 one dwordx4, fp16 one dwordx2, u8 one dword.  The four lanes of a row cover 64 / 32 / 16 contiguous bytes.
// (No wider load for the narrow types: sixteen u8 of one load are all sixteen accumulators of a step, i.e. the other three lanes'
//  elements too -- handing them over costs more DPP moves than the load saves, and the bytes fetched are the same sectors.)
template <class ROW> struct RowQuad;
template <> struct RowQuad<float> {
  float4 v;
  __device__ __forceinline__ void load(const float *p) { v = *reinterpret_cast<const float4 *>(p); }
  __device__ __forceinline__ float4 widen() const { return v; }
};
template <> struct RowQuad<uint8_t> {
  uint32_t w;
  __device__ __forceinline__ void load(const uint8_t *p) { w = *reinterpret_cast<const uint32_t *>(p); }
  __device__ __forceinline__ float4 widen() const {   // v_cvt_f32_ubyte0 .. 3
    return float4{(float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24)};
  }
};
template <> struct RowQuad<_Float16> {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  uint2 w;
  __device__ __forceinline__ void load(const _Float16 *p) { w = *reinterpret_cast<const uint2 *>(p); }
  __device__ __forceinline__ float4 widen() const {   // v_cvt_f32_f16 on each half; never packed fp16 arithmetic
    const h2 a = __builtin_bit_cast(h2, w.x), b = __builtin_bit_cast(h2, w.y);
    return float4{(float)a.x, (float)a.y, (float)b.x, (float)b.y};
  }
};

}  // namespace hs
