// index_update.hip -- in-place updates of a resident vanilla index (hs_index_add_points, hs_index_upsert_points,
// hs_index_mark_deleted): the changed nodes of a call arrive as records in ONE staging buffer (one host-to-device copy) and one
// kernel writes them into the index's arrays.
//
// Staging buffer of a call with nrec records, the first `first_row` of them nodes of which only the level-0 list changed, the rest
// nodes that carry a row -- new nodes, and existing nodes that an update or a replacement rewrote: a record's id is any id below
// the row capacity, no id occurs in two records of a call (all sections start 16-byte aligned: the header is 16 bytes, the tile
// stride a multiple of 16 ids, row_words = dim rounded up to a multiple of 4):
//   header  nrec x 4 words   {internal id, delete mark (0 / 1), label low word, label high word}
//   tiles   nrec x stride    the node's level-0 ids padded with 0xFFFFFFFF to the tile stride
//   rows    (nrec - first_row) x row_words   the fp32 row of each record from first_row on
// One wavefront per record: the tile row leaves as 16-byte stores (a row is 64 .. 256 contiguous bytes), the fp32 row -- where the
// index holds fp32 rows -- as 16-byte loads and stores (4-byte ones for dim % 4 != 0, whose rows are not 16-byte aligned), the
// narrow row -- where the index holds a narrow copy -- straight in the lane-major layout of narrow_rows.hpp, each lane packing
// the values of 4 consecutive output bytes into one 32-bit store, and lane 0 writes the label and the mark byte.
#include <hip/hip_runtime.h>

#include "index_update.hpp"
#include "narrow_rows.hpp"

namespace hs {

// the element of the fp32 row that sits at slot o of its narrow row (inverse of narrow_slot)
__device__ inline uint32_t narrow_source(uint32_t o, uint32_t dim) {
  const uint32_t per = dim >> 3, s = o / per, rem = o - s * per;
  return ((rem >> 1) << 4) + 2u * s + (rem & 1u);
}

__device__ inline uint32_t pack4_u8(const float *x, uint32_t o, uint32_t dim) {
  uint32_t w = 0;
  for (uint32_t b = 0; b < 4; b++) w |= (uint32_t)narrow_cast<uint8_t>(x[narrow_source(o + b, dim)]) << (8 * b);
  return w;
}
__device__ inline uint32_t pack2_f16(const float *x, uint32_t o, uint32_t dim) {
  uint32_t w = 0;
  for (uint32_t b = 0; b < 2; b++) {
    const _Float16 h = narrow_cast<_Float16>(x[narrow_source(o + b, dim)]);
    w |= (uint32_t)__builtin_bit_cast(unsigned short, h) << (16 * b);
  }
  return w;
}

__global__ void __launch_bounds__(kUpdateBlock) index_update_kernel(UpdateArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (kUpdateBlock / 64) + (threadIdx.x >> 6);
  if (r >= a.nrec) return;
  const uint32_t *head = a.stage + (size_t)r * 4;
  const uint32_t id = head[0];
  if (id >= a.cap_rows) return;   // (validated on the host; nothing is written outside the arrays whatever the buffer holds)
  // level-0 tile row
  if (a.tile0) {
    const uint4 *src = reinterpret_cast<const uint4 *>(a.stage + (size_t)a.nrec * 4 + (size_t)r * a.stride);
    uint4 *dst = reinterpret_cast<uint4 *>(a.tile0 + (size_t)id * a.stride);
    if (lane < a.stride / 4) dst[lane] = src[lane];
  }
  if (r >= a.first_row) {
    const float *x = a.src_vec ? a.src_vec + (size_t)id * a.dim
                               : reinterpret_cast<const float *>(a.stage + (size_t)a.nrec * (4 + a.stride) + (size_t)(r - a.first_row) * a.row_words);
    if (a.vec) {
      float *dst = a.vec + (size_t)id * a.dim;
      if ((a.dim & 3u) == 0) {
        for (uint32_t c = lane; c < a.dim / 4; c += 64) reinterpret_cast<uint4 *>(dst)[c] = reinterpret_cast<const uint4 *>(x)[c];
      } else {
        for (uint32_t c = lane; c < a.dim; c += 64) dst[c] = x[c];
      }
    }
    if (a.narrow) {   // dim % 16 == 0 (hs_index_set_row_format): a row is a whole number of 32-bit words in both formats
      if (a.fmt == ROWS_U8) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(a.narrow) + (size_t)id * a.dim);
        for (uint32_t w = lane; w < a.dim / 4; w += 64) dst[w] = pack4_u8(x, 4 * w, a.dim);
      } else {
        uint32_t *dst = reinterpret_cast<uint32_t *>(static_cast<_Float16 *>(a.narrow) + (size_t)id * a.dim);
        for (uint32_t w = lane; w < a.dim / 2; w += 64) dst[w] = pack2_f16(x, 2 * w, a.dim);
      }
    }
  }
  if (lane == 0) {
    a.labels[id] = (uint64_t)head[2] | ((uint64_t)head[3] << 32);
    a.deleted[id] = (uint8_t)(head[1] & 1u);
  }
}

hipError_t launch_index_update(const UpdateArgs &a, hipStream_t stream) {
  if (a.nrec == 0) return hipSuccess;
  if (!a.stage || !a.labels || !a.deleted || a.first_row > a.nrec) return hipErrorInvalidValue;
  if (a.tile0 && (a.stride == 0 || (a.stride & 15u) != 0 || a.stride > 64)) return hipErrorInvalidValue;
  if (a.narrow && ((a.dim & 15u) != 0 || (a.fmt != ROWS_U8 && a.fmt != ROWS_F16))) return hipErrorInvalidValue;
  const uint32_t per = kUpdateBlock / 64;
  hipLaunchKernelGGL(index_update_kernel, dim3((a.nrec + per - 1) / per), dim3(kUpdateBlock), 0, stream, a);
  return hipGetLastError();
}

// hs_index_mark_deleted: stage = count ids, then count mark bytes; one thread per mark.
__global__ void __launch_bounds__(256) mark_scatter_kernel(const uint32_t *stage, uint32_t count, uint32_t n, uint8_t *deleted) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= count) return;
  const uint32_t id = stage[t];
  if (id < n) deleted[id] = reinterpret_cast<const uint8_t *>(stage + count)[t];
}

hipError_t launch_mark_scatter(const uint32_t *d_stage, uint32_t count, uint32_t n, uint8_t *d_deleted, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if (!d_stage || !d_deleted) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mark_scatter_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, d_stage, count, n, d_deleted);
  return hipGetLastError();
}

}  // namespace hs
