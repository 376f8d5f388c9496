// filter_set.hip -- filter sets: nf bitmaps over the n internal ids of an index, resident in HBM (hs_filter_set_*).
//
// Layout: row f = row_words 32-bit words, row_words = ceil(n / 32) rounded up to a multiple of 4 (rows start 16-byte aligned);
// bit i & 31 of word i >> 5 is set iff filter f allows internal id i (what isIdAllowed(label of i) returns: hnswalg.h:442-444,
// hnswalg_slim.h:578-580).  Bits beyond n and the padding words are zero.  Delete marks are NOT folded in: the search kernels
// test "marked deleted or bit clear" (beam_search.hip excl_issue), so a later hs_index_patch that marks nodes needs no rewrite.
//
// Pack: one wavefront turns 512 consecutive ids of one row into 16 words.  Lane l reads byte base + 64 t + l for t = 0..7 -- eight
// independent loads in flight, each a 64-byte run of consecutive addresses whatever the alignment of the row (n is arbitrary, so a
// row of bytes starts anywhere) -- a ballot per t gives two words, and lanes 0..15 store the 16 words as one 64-byte run.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.hpp"
#include "wave_util.hpp"

namespace hs {

constexpr uint32_t kPackThreads = 256, kPackWaves = kPackThreads / 64, kPackIds = 512, kPackWords = kPackIds / 32;

__global__ void __launch_bounds__(kPackThreads) filter_pack_kernel(const uint8_t *allowed, uint32_t *words, uint32_t n, uint32_t row_words) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint8_t *src = allowed + (size_t)blockIdx.y * n;
  uint32_t *dst = words + (size_t)blockIdx.y * row_words;
  const uint32_t chunks = (row_words + kPackWords - 1) / kPackWords;
  for (uint32_t ch = blockIdx.x * kPackWaves + wv; ch < chunks; ch += gridDim.x * kPackWaves) {
    const uint32_t base = ch * kPackIds;
    uint8_t b[8];
#pragma unroll
    for (uint32_t t = 0; t < 8; t++) {
      const uint32_t i = base + 64 * t + lane;
      b[t] = i < n ? src[i] : (uint8_t)0;   // the tail n % 32 and the padding words: zero bits
    }
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8; t++) {
      const unsigned long long m = hs_ballot(b[t] != 0);
      if (lane == 2 * t) mine = (uint32_t)m;
      if (lane == 2 * t + 1) mine = (uint32_t)(m >> 32);
    }
    const uint32_t w = ch * kPackWords + lane;
    if (lane < kPackWords && w < row_words) dst[w] = mine;
  }
}

__global__ void __launch_bounds__(256) filter_unpack_kernel(const uint32_t *row, uint8_t *allowed, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    allowed[i] = (uint8_t)((row[i >> 5] >> (i & 31u)) & 1u);
}

hipError_t launch_filter_pack(const uint8_t *d_allowed, uint32_t *d_words, uint32_t n, uint32_t count, uint32_t row_words, hipStream_t stream) {
  if (count == 0 || row_words == 0) return hipSuccess;
  const uint32_t chunks = (row_words + kPackWords - 1) / kPackWords;
  const uint32_t gx = std::min<uint32_t>((chunks + kPackWaves - 1) / kPackWaves, 1024u);
  for (uint32_t r0 = 0; r0 < count; r0 += 65535u) {   // gridDim.y limit
    const uint32_t rows = std::min<uint32_t>(count - r0, 65535u);
    hipLaunchKernelGGL(filter_pack_kernel, dim3(gx, rows), dim3(kPackThreads), 0, stream, d_allowed + (size_t)r0 * n,
                       d_words + (size_t)r0 * row_words, n, row_words);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_filter_unpack(const uint32_t *d_row, uint8_t *d_allowed, uint32_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(filter_unpack_kernel, dim3(std::min<uint32_t>((n + 255) / 256, 2048u)), dim3(256), 0, stream, d_row, d_allowed, n);
  return hipGetLastError();
}

}  // namespace hs
