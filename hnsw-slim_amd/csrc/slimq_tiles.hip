// slimq_tiles.hip -- the arrays of a resident HNSW-SlimQ index gathered on the device: the RaBitQ records from the
// fields of the file image, the fused level-0 tiles from the records and the id tiles, the fused upper-level tiles from the records
// and the upper CSR.  The words are those of slimq_tiles.hpp; every word of every output is written here (hipMalloc memory is not
// zero).  Records are multiples of 16 bytes, so everything moves as uint4 pieces: consecutive lanes take consecutive pieces of a
// node's contiguous output row (slot = piece / (rw/4), part = piece % (rw/4)) -- whole-line stores, 32-112-byte contiguous loads.
// All offsets are 64-bit: n x stride x rw passes 2^32 words at 2.4M rows of d = 768.  Plain loads and stores only, no atomics.
#include <hip/hip_runtime.h>

#include "slimq_engine.hpp"

namespace hs {

static constexpr uint32_t kTileBlock = 256, kTileWaves = kTileBlock / 64;
static constexpr uint32_t kEmptyId = 0xFFFFFFFFu;

// one thread per 16-byte piece of the record array, grid-stride
__global__ __launch_bounds__(kTileBlock) void slimq_records_kernel(const float *__restrict__ factors, const uint32_t *__restrict__ cluster,
                                                                   const uint32_t *__restrict__ code32, uint32_t n, uint32_t nblk,
                                                                   uint32_t rw, uint4 *__restrict__ rec) {
  const uint32_t q4 = rw / 4, cw = 2 * nblk;
  const uint64_t total = (uint64_t)n * q4, step = (uint64_t)gridDim.x * kTileBlock;
  for (uint64_t p = (uint64_t)blockIdx.x * kTileBlock + threadIdx.x; p < total; p += step) {
    const uint64_t i = p / q4;
    const uint32_t part = (uint32_t)(p - i * q4);
    uint4 v;
    if (part == 0) {
      const float *f = factors + i * 3;
      v = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), cluster[i], __float_as_uint(f[2]));
    } else {
      const uint32_t w = 4 * (part - 1);   // first code word of this piece
      const uint32_t *c = code32 + i * cw;
      v.x = w < cw ? c[w] : 0u;
      v.y = w + 1 < cw ? c[w + 1] : 0u;
      v.z = w + 2 < cw ? c[w + 2] : 0u;
      v.w = w + 3 < cw ? c[w + 3] : 0u;
    }
    rec[p] = v;
  }
}

// one wavefront per node, grid-stride: lane j holds the id of slot j (stride <= 64)
__global__ __launch_bounds__(kTileBlock) void slimq_ftile_kernel(const uint4 *__restrict__ rec, const uint32_t *__restrict__ tile0, uint32_t n,
                                                                 uint32_t stride, uint32_t rw, uint4 *__restrict__ ftile) {
  const uint32_t lane = threadIdx.x & 63, q4 = rw / 4, pieces = stride * q4;
  const uint64_t step = (uint64_t)gridDim.x * kTileWaves;
  for (uint64_t i = (uint64_t)blockIdx.x * kTileWaves + (threadIdx.x >> 6); i < n; i += step) {
    const uint32_t my = lane < stride ? tile0[i * stride + lane] : kEmptyId;
    uint4 *row = ftile + i * pieces;
    for (uint32_t p0 = 0; p0 < pieces; p0 += 64) {   // (uniform trip count: every lane takes part in the shuffle)
      const uint32_t p = p0 + lane, slot = min(p / q4, stride - 1), part = p % q4;
      const uint32_t id = (uint32_t)__shfl((int)my, (int)slot);
      if (p >= pieces) continue;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (id < n) v = rec[(uint64_t)id * q4 + part];   // (an empty slot's id is 0xFFFFFFFF >= n)
      if (part == 0) v.w = id;
      row[p] = v;
    }
  }
}

// one wavefront per entry of up_ptr, grid-stride: lane j holds the id of slot j of the list that starts there (up_stride <= 64); the
// entry behind a node's last list -- and the array's last -- starts an empty list (up_ptr repeats there), so its row comes out empty
__global__ __launch_bounds__(kTileBlock) void slimq_uptile_kernel(const uint4 *__restrict__ rec, const uint32_t *__restrict__ up_ptr, uint32_t entries,
                                                                  const uint32_t *__restrict__ cols, const uint32_t *__restrict__ up_base,
                                                                  uint32_t n, uint32_t up_stride, uint32_t rw, uint4 *__restrict__ uptile) {
  const uint32_t lane = threadIdx.x & 63, q4 = rw / 4, uq4 = q4 + 1, pieces = up_stride * uq4;
  const uint64_t step = (uint64_t)gridDim.x * kTileWaves;
  for (uint64_t t = (uint64_t)blockIdx.x * kTileWaves + (threadIdx.x >> 6); t < entries; t += step) {
    const uint32_t s0 = up_ptr[t], e0 = t + 1 < entries ? up_ptr[t + 1] : s0;
    const uint32_t deg = e0 >= s0 ? min(e0 - s0, up_stride) : 0u;
    const uint32_t my = lane < deg ? cols[(uint64_t)s0 + lane] : kEmptyId;
    uint4 *row = uptile + t * pieces;
    for (uint32_t p0 = 0; p0 < pieces; p0 += 64) {
      const uint32_t p = p0 + lane, slot = min(p / uq4, up_stride - 1), part = p % uq4;
      const uint32_t id = (uint32_t)__shfl((int)my, (int)slot);
      if (p >= pieces) continue;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (id < n) {
        if (part < q4) v = rec[(uint64_t)id * q4 + part];
        else v.x = up_base[id];
      }
      if (part == 0) v.w = id;
      row[p] = v;
    }
  }
}

static uint32_t grid_for(uint64_t items, uint32_t per_block) {
  // enough blocks to fill the device several times over, the rest by the grid-stride loops
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, 256u * 64u));
}

hipError_t launch_slimq_records(const float *factors, const uint32_t *cluster, const uint64_t *code, uint32_t n, uint32_t padded, uint32_t *rec,
                                hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t nblk = padded / 64, rw = (4 + 2 * nblk + 3) & ~3u;
  hipLaunchKernelGGL(slimq_records_kernel, dim3(grid_for((uint64_t)n * (rw / 4), kTileBlock)), dim3(kTileBlock), 0, stream, factors, cluster,
                     reinterpret_cast<const uint32_t *>(code), n, nblk, rw, reinterpret_cast<uint4 *>(rec));
  return hipGetLastError();
}

hipError_t launch_slimq_ftile(const uint32_t *rec, const uint32_t *tile0, uint32_t n, uint32_t stride, uint32_t rw, uint32_t *ftile,
                              hipStream_t stream) {
  if (n == 0 || stride == 0) return hipSuccess;
  if (stride > 64 || (rw & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(slimq_ftile_kernel, dim3(grid_for(n, kTileWaves)), dim3(kTileBlock), 0, stream, reinterpret_cast<const uint4 *>(rec), tile0, n,
                     stride, rw, reinterpret_cast<uint4 *>(ftile));
  return hipGetLastError();
}

hipError_t launch_slimq_uptile(const uint32_t *rec, const uint32_t *up_ptr, uint32_t entries, const uint32_t *cols, const uint32_t *up_base,
                               uint32_t n, uint32_t up_stride, uint32_t rw, uint32_t *uptile, hipStream_t stream) {
  if (entries == 0 || up_stride == 0) return hipSuccess;
  if (up_stride > 64 || (rw & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(slimq_uptile_kernel, dim3(grid_for(entries, kTileWaves)), dim3(kTileBlock), 0, stream, reinterpret_cast<const uint4 *>(rec),
                     up_ptr, entries, cols, up_base, n, up_stride, rw, reinterpret_cast<uint4 *>(uptile));
  return hipGetLastError();
}

}  // namespace hs
