// narrow_rows.hip -- the narrow copy of an index's rows (hs_index_set_row_format): layout, device conversion with the
// representability check, and its inverse (widening, exact).  The kernels that search over the copy are the narrow objects of
// flat_search.hip and beam_search.hip (flat_search_u8.hip, beam_search_f16.hip, ...), reached through launch_search (engine.hpp).
//
// Layout (narrow_rows.hpp narrow_slot): row r occupies dim elements at r * dim, lane-major for the flat kernel's 8 lanes per row,
//   narrow[r * dim + s * (dim / 8) + 2 i + e] = x[r][16 i + 2 s + e]      s = 0..7, i = 0..dim/16 - 1, e = 0..1
// so the elements lane s multiplies (flat_search.hip flat_dist8) are one contiguous chunk.  dim % 16 == 0, so a u8 row is a
// multiple of 16 bytes and every row starts 16-byte aligned.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "narrow_rows.hpp"

namespace hs {

// One thread per element of rows [row0, row0 + nrows): writes the narrow value at its lane-major slot and, where the fp32 value
// does not survive the round trip, lowers *first_bad to its row (an ordinary vector atomic min).
template <typename T>
__global__ void __launch_bounds__(256) narrow_convert_kernel(const float *vec, T *out, uint32_t row0, uint32_t nrows, uint32_t dim, uint32_t *first_bad) {
  const uint64_t total = (uint64_t)nrows * dim;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = row0 + (uint32_t)(t / dim), j = (uint32_t)(t % dim);
    const float x = vec[(size_t)r * dim + j];
    out[(size_t)r * dim + narrow_slot(j, dim)] = narrow_cast<T>(x);
    if (!narrow_fits<T>(x)) atomicMin(first_bad, r);
  }
}

template <typename T>
static hipError_t convert_t(const float *d_vec, void *d_out, uint32_t row0, uint32_t nrows, uint32_t dim, uint32_t *d_first_bad, hipStream_t stream) {
  const uint64_t total = (uint64_t)nrows * dim;
  if (total == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((total + 255) / 256, 256u * 64u);
  hipLaunchKernelGGL(narrow_convert_kernel<T>, dim3(grid), dim3(256), 0, stream, d_vec, reinterpret_cast<T *>(d_out), row0, nrows, dim, d_first_bad);
  return hipGetLastError();
}
hipError_t launch_narrow_convert(const float *d_vec, void *d_out, int fmt, uint32_t row0, uint32_t nrows, uint32_t dim, uint32_t *d_first_bad,
                                 hipStream_t stream) {
  return fmt == ROWS_U8 ? convert_t<uint8_t>(d_vec, d_out, row0, nrows, dim, d_first_bad, stream)
                        : convert_t<_Float16>(d_vec, d_out, row0, nrows, dim, d_first_bad, stream);
}

// The inverse: one thread per element of rows [row0, row0 + nrows) of the fp32 array, read from its lane-major slot (u8 -> fp32 and
// fp16 -> fp32 are exact; a -0.0f that went into a u8 copy comes back as +0.0f).
template <typename T>
__global__ void __launch_bounds__(256) narrow_widen_kernel(const T *rows, float *vec, uint32_t row0, uint32_t nrows, uint32_t dim) {
  const uint64_t total = (uint64_t)nrows * dim;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = row0 + (uint32_t)(t / dim), j = (uint32_t)(t % dim);
    vec[(size_t)r * dim + j] = (float)rows[(size_t)r * dim + narrow_slot(j, dim)];
  }
}
template <typename T>
static hipError_t widen_t(const void *d_rows, float *d_vec, uint32_t row0, uint32_t nrows, uint32_t dim, hipStream_t stream) {
  const uint64_t total = (uint64_t)nrows * dim;
  if (total == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((total + 255) / 256, 256u * 64u);
  hipLaunchKernelGGL(narrow_widen_kernel<T>, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const T *>(d_rows), d_vec, row0, nrows, dim);
  return hipGetLastError();
}
hipError_t launch_narrow_widen(const void *d_rows, float *d_vec, int fmt, uint32_t row0, uint32_t nrows, uint32_t dim, hipStream_t stream) {
  return fmt == ROWS_U8 ? widen_t<uint8_t>(d_rows, d_vec, row0, nrows, dim, stream) : widen_t<_Float16>(d_rows, d_vec, row0, nrows, dim, stream);
}

}  // namespace hs
