// host_tiles.hpp -- the tile arrays the host builds from a PackedIndex before an upload: the level-0 id tiles and the upper-level
// {id, up_base} tiles of the greedy descent (engine.hpp).  Host-only: capi_index.cpp uploads what these return, and
// csrc/load_guard_test.cpp runs them under the sanitizers on every graph the loaders accept.  They index with the ids of `p`
// unchecked: the loaders have run index_check.hpp before a PackedIndex exists.
#pragma once
#include "packed_index.hpp"

namespace hs {

// stride of the level-0 tiles: a 64-byte multiple that holds the widest list; 0 = no tiles (a list wider than 64 ids)
inline uint32_t tile_stride_for(size_t max_deg0) { return max_deg0 <= 64 ? std::max<uint32_t>(16, (uint32_t)((max_deg0 + 15) / 16 * 16)) : 0; }

// level-0 adjacency tiles: node i's ids padded with 0xFFFFFFFF to the fixed stride
inline std::vector<uint32_t> build_tile0(const PackedIndex &p, uint32_t stride) {
  std::vector<uint32_t> tile((size_t)p.n * stride, 0xFFFFFFFFu);
  for (size_t i = 0; i < p.n; i++)
    std::copy(p.cols.begin() + p.row_ptr0[i], p.cols.begin() + p.row_ptr0[i + 1], tile.begin() + i * stride);
  return tile;
}

// upper-level tiles for the greedy descent (see engine.hpp): slot t = up_ptr entry t, {neighbour id, the neighbour's up_base}
inline std::vector<uint32_t> build_uptile(const PackedIndex &p, uint32_t &up_stride) {
  up_stride = 0;
  std::vector<uint32_t> ut;
  size_t max_up = 0;
  for (size_t t = 0; t + 1 < p.up_ptr.size(); t++)
    if (p.up_ptr[t + 1] > p.up_ptr[t]) max_up = std::max<size_t>(max_up, p.up_ptr[t + 1] - p.up_ptr[t]);
  if (p.up_ptr.empty() || max_up > 64) return ut;
  up_stride = std::max<uint32_t>(16, (uint32_t)((max_up + 15) / 16 * 16));
  ut.assign(p.up_ptr.size() * (size_t)up_stride * 2, 0xFFFFFFFFu);
  // a node with L upper levels owns L+1 consecutive up_ptr entries (L list starts + one terminator), in id order
  std::vector<uint32_t> owners;
  for (size_t i = 0; i < p.n; i++)
    if (p.up_base[i] != PackedIndex::NONE) owners.push_back((uint32_t)i);
  for (size_t o = 0; o < owners.size(); o++) {
    const uint32_t b0 = p.up_base[owners[o]];
    const uint32_t end = o + 1 < owners.size() ? p.up_base[owners[o + 1]] : (uint32_t)p.up_ptr.size();
    for (uint32_t t = b0; t + 1 < end; t++) {
      const uint32_t s0 = p.up_ptr[t], e0 = p.up_ptr[t + 1];
      for (uint32_t j = 0; j < e0 - s0; j++) {
        const uint32_t nb = p.cols[s0 + j];
        ut[((size_t)t * up_stride + j) * 2] = nb;
        ut[((size_t)t * up_stride + j) * 2 + 1] = p.up_base[nb];
      }
    }
  }
  return ut;
}

// up_base[enterpoint], what the descent starts from (DevIndex::ep_base); NONE for an empty index
inline uint32_t ep_base_of(const PackedIndex &p) { return p.n ? p.up_base[p.enterpoint] : PackedIndex::NONE; }

}  // namespace hs
