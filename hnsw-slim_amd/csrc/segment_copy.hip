// segment_copy.hip -- the two copy kernels of a search queue (hs_queue_*, capi_queue.cpp).
//
// A launch of the queue serves many submissions ("segments"): segment s owns rows [first_row[s], first_row[s + 1]) of the launch.
// The segment table -- first_row[n_seg + 1] and one 64-byte SegEntry per segment (search_queue.hpp) -- is written by the host
// into page-locked memory and read here through its device address; nothing is copied ahead of the kernels.
//
//   hs::gather_rows_kernel      row r of the launch <- row r - first_row[s] of segment s's source; one launch however many
//                               segments.  One wavefront per row.  A source is only known to be 4-byte aligned (a slice of a
//                               caller's tensor): a row moves as 16-byte accesses when its source address and dim * 4 are both
//                               multiples of 16 (the destination row then is too: the array is allocation-aligned), as 4-byte
//                               accesses otherwise.  The filter index of the row, where the launch has filters, goes with it.
//   hs::scatter_results_kernel  the reverse for labels32 / labels64 / dists / counts / stats: one thread per (row, column), columns
//                               0 .. max(k, 4); an output a segment did not ask for is a null pointer in its entry and skipped.
//                               Outputs are only element-aligned, so every access is one element.
//
// The segment of a row is found by binary search over first_row (segment_of_row): in LDS when the launch has at most kSegLds
// segments (each block copies the prefix once), in global memory beyond that.
// Bounds: every row index is < total (checked per row / per thread); a segment's source and outputs hold first_row[s + 1] -
// first_row[s] rows by the contract of hs_queue_submit; the launch arrays hold max_queries >= total rows.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "segment_copy.hpp"

namespace hs {

constexpr uint32_t kCopyThreads = 256, kCopyWaves = kCopyThreads / 64;
constexpr uint32_t kGatherRowsPerBlock = 16;

// The row prefix a block searches: its LDS copy when it fits, else the table itself.
__device__ __forceinline__ const uint32_t *stage_prefix(const uint32_t *first_row, uint32_t n_seg, uint32_t *lds) {
  if (n_seg > kSegLds) return first_row;
  for (uint32_t i = threadIdx.x; i <= n_seg; i += kCopyThreads) lds[i] = first_row[i];
  __syncthreads();
  return lds;
}

__global__ void __launch_bounds__(kCopyThreads) gather_rows_kernel(const uint32_t *first_row, const SegEntry *entries, uint32_t n_seg,
                                                                   uint32_t total, uint32_t dim, float *q, uint32_t *foq) {
  __shared__ uint32_t pre[kSegLds + 1];
  const uint32_t *fr = stage_prefix(first_row, n_seg, pre);
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t r0 = blockIdx.x * kGatherRowsPerBlock, r1 = min(r0 + kGatherRowsPerBlock, total);
  for (uint32_t row = r0 + wv; row < r1; row += kCopyWaves) {
    const uint32_t s = segment_of_row(fr, n_seg, row);
    const uint32_t local = row - fr[s];
    const float *src = entries[s].src + (size_t)local * dim;
    float *dst = q + (size_t)row * dim;
    if ((((uintptr_t)src | ((uintptr_t)dim * 4u)) & 15u) == 0) {
      const float4 *s4 = reinterpret_cast<const float4 *>(src);
      float4 *d4 = reinterpret_cast<float4 *>(dst);
      for (uint32_t i = lane; i < dim / 4; i += 64) d4[i] = s4[i];
    } else {
      for (uint32_t i = lane; i < dim; i += 64) dst[i] = src[i];
    }
    if (foq && lane == 0) {
      const uint32_t *fs = entries[s].foq_src;
      foq[row] = fs ? fs[local] : 0xFFFFFFFFu;   // (no filter named: an index outside every set, reported by the check)
    }
  }
}

__global__ void __launch_bounds__(kCopyThreads) scatter_results_kernel(const uint32_t *first_row, const SegEntry *entries, uint32_t n_seg,
                                                                       uint32_t total, uint32_t k, LaunchArrays a) {
  __shared__ uint32_t pre[kSegLds + 1];
  const uint32_t *fr = stage_prefix(first_row, n_seg, pre);
  const uint32_t width = max(k, 4u);
  const uint64_t cells = (uint64_t)total * width;
  for (uint64_t idx = (uint64_t)blockIdx.x * kCopyThreads + threadIdx.x; idx < cells; idx += (uint64_t)gridDim.x * kCopyThreads) {
    const uint32_t row = (uint32_t)(idx / width), j = (uint32_t)(idx % width);
    const uint32_t s = segment_of_row(fr, n_seg, row);
    const size_t local = row - fr[s];
    const SegEntry *e = entries + s;
    if (j < k) {
      const size_t from = (size_t)row * k + j, to = local * k + j;
      if (a.l32) { uint32_t *o = e->l32; if (o) o[to] = a.l32[from]; }
      if (a.l64) { uint64_t *o = e->l64; if (o) o[to] = a.l64[from]; }
      if (a.dd) { float *o = e->dd; if (o) o[to] = a.dd[from]; }
    }
    if (j == 0 && a.cnt) { uint32_t *o = e->cnt; if (o) o[local] = a.cnt[row]; }
    if (j < 4 && a.stats) { uint32_t *o = e->stats; if (o) o[local * 4 + j] = a.stats[(size_t)row * 4 + j]; }
  }
}

hipError_t launch_gather_rows(const uint32_t *first_row, const SegEntry *entries, uint32_t n_seg, uint32_t total, uint32_t dim,
                              float *q, uint32_t *foq, hipStream_t stream) {
  if (total == 0 || n_seg == 0) return hipSuccess;
  const uint32_t grid = (total + kGatherRowsPerBlock - 1) / kGatherRowsPerBlock;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(kCopyThreads), 0, stream, first_row, entries, n_seg, total, dim, q, foq);
  return hipGetLastError();
}

hipError_t launch_scatter_results(const uint32_t *first_row, const SegEntry *entries, uint32_t n_seg, uint32_t total, uint32_t k,
                                  const LaunchArrays &a, hipStream_t stream) {
  if (total == 0 || n_seg == 0) return hipSuccess;
  const uint64_t cells = (uint64_t)total * std::max(k, 4u);
  const uint32_t grid = (uint32_t)std::min<uint64_t>((cells + kCopyThreads - 1) / kCopyThreads, 4096u);
  hipLaunchKernelGGL(scatter_results_kernel, dim3(grid), dim3(kCopyThreads), 0, stream, first_row, entries, n_seg, total, k, a);
  return hipGetLastError();
}

}  // namespace hs
