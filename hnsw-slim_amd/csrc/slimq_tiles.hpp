// slimq_tiles.hpp -- the arrays a resident HNSW-SlimQ index searches (layout: slimq_engine.hpp), stated on the host: the RaBitQ
// records, the fused level-0 tiles and the fused upper-level tiles.  slimq_tiles.hip writes the same words on the device; these
// functions are the CPU-testable statement of the layout (csrc/slimq_tiles_test.cpp, tests/test_slimq_resident_cpu.py).  No HIP here.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace hs {

static constexpr uint32_t kSlimqEmpty = 0xFFFFFFFFu;   // an empty tile slot's id word; PackedIndex::NONE in up_base

// words of one record: {f_add, f_rescale, cluster id, f_error} + padded/64 u64 sign-code words, rounded up to 16 bytes
inline uint32_t slimq_rec_words(size_t padded) { return (4 + 2 * (uint32_t)(padded / 64) + 3) & ~3u; }

// the upper tiles' stride: max(16, round_up_16(longest upper list)), 0 (no fused upper tiles) without upper lists or beyond 64 ids
inline uint32_t slimq_up_stride(const std::vector<uint32_t> &up_ptr) {
  size_t max_up = 0;
  for (size_t t = 0; t + 1 < up_ptr.size(); t++) max_up = std::max<size_t>(max_up, up_ptr[t + 1] >= up_ptr[t] ? up_ptr[t + 1] - up_ptr[t] : 0);
  if (up_ptr.empty() || max_up > 64) return 0;
  return std::max<uint32_t>(16, (uint32_t)((max_up + 15) / 16 * 16));
}

// rec[i] = {f_add, f_rescale, cluster id, f_error}, the sign-code words, zeros up to the 16-byte multiple
// factors: n x 3 {f_add, f_rescale, f_error}; code: n x padded/64
inline std::vector<uint32_t> slimq_pack_records(const float *factors, const uint32_t *cluster, const uint64_t *code, size_t n, size_t padded) {
  const uint32_t nblk = (uint32_t)(padded / 64), rw = slimq_rec_words(padded);
  std::vector<uint32_t> rec(n * rw, 0u);
  for (size_t i = 0; i < n; i++) {
    uint32_t *r = &rec[i * rw];
    memcpy(r, &factors[i * 3], 4); memcpy(r + 1, &factors[i * 3 + 1], 4);
    r[2] = cluster[i];
    memcpy(r + 3, &factors[i * 3 + 2], 4);
    memcpy(r + 4, &code[i * nblk], 8 * nblk);
  }
  return rec;
}

// ftile[i][j], j < stride: the record of the j-th level-0 neighbour of node i with word 3 = its id; beyond the list all zero with
// word 3 = 0xFFFFFFFF.  row_ptr0 / cols: the level-0 CSR (PackedIndex).  stride == 0: no array.
inline std::vector<uint32_t> slimq_ftile_host(const std::vector<uint32_t> &rec, uint32_t rw, size_t n, const uint32_t *row_ptr0,
                                              const uint32_t *cols, uint32_t stride) {
  std::vector<uint32_t> ft;
  if (!stride) return ft;
  ft.assign(n * stride * rw, 0u);
  for (size_t i = 0; i < n; i++) {
    uint32_t *row = &ft[i * stride * rw];
    const uint32_t deg = row_ptr0[i + 1] - row_ptr0[i];
    for (uint32_t j = 0; j < stride; j++) {
      uint32_t *r = row + (size_t)j * rw;
      if (j < deg) {
        const uint32_t nb = cols[row_ptr0[i] + j];
        memcpy(r, &rec[(size_t)nb * rw], 4 * rw);
        r[3] = nb;
      } else {
        r[3] = kSlimqEmpty;
      }
    }
  }
  return ft;
}

// One row of up_stride slots of rw + 4 words per entry of up_ptr: the row of entry up_base[i] + l - 1 holds level l of node i
// (1 <= l <= level[i]), records as in ftile followed by {up_base[neighbour], 0, 0, 0}; every other slot -- and the whole row of an
// entry no (node, level) owns -- is zero with word 3 = 0xFFFFFFFF.  up_stride == 0: no array.
inline std::vector<uint32_t> slimq_uptile_host(const std::vector<uint32_t> &rec, uint32_t rw, size_t n, const int32_t *level,
                                               const std::vector<uint32_t> &up_base, const std::vector<uint32_t> &up_ptr,
                                               const uint32_t *cols, uint32_t up_stride) {
  std::vector<uint32_t> ut;
  if (!up_stride) return ut;
  const uint32_t urw = rw + 4;
  ut.assign(up_ptr.size() * (size_t)up_stride * urw, 0u);
  for (size_t t = 0; t < up_ptr.size(); t++)
    for (uint32_t j = 0; j < up_stride; j++) ut[(t * up_stride + j) * urw + 3] = kSlimqEmpty;
  for (size_t i = 0; i < n; i++) {
    const uint32_t b = up_base[i];
    if (b == kSlimqEmpty) continue;
    for (int l = 1; l <= level[i]; l++) {
      const uint32_t s0 = up_ptr[b + l - 1], e0 = up_ptr[b + l];
      for (uint32_t j = 0; j < e0 - s0; j++) {
        const uint32_t nb = cols[s0 + j];
        uint32_t *r = &ut[((size_t)(b + l - 1) * up_stride + j) * urw];
        memcpy(r, &rec[(size_t)nb * rw], 4 * rw);
        r[3] = nb;
        r[rw] = up_base[nb];
      }
    }
  }
  return ut;
}

}  // namespace hs
