// index_check.hpp -- what a graph must satisfy before a kernel (or the host code that packs it for one) may index with its ids,
// counts and levels.  Host-only and free of HIP: every loader calls it ("what a loader guarantees"), and
// csrc/load_guard_test.cpp runs it stand-alone.  The reference validates none of this (a hostile file makes it segfault); the
// contract is this project's.
//
// The preconditions, each with the expression it protects.  n = element count, level(i) = node i's top level.
//   P1 level      level(i) >= 0 for every node; in a HierarchicalNSW image and in caller's arrays also level(i) <= maxlevel.
//                   pack_chal reads 2 * level bytes of offsets and loops l = 1 .. level (packed_index.hpp); convertFromHNSW's
//                   histograms hist[l], l <= level(i), have maxlevel + 1 rows (host_graph.hpp hub_thresholds).  A Slim / SlimQ
//                   node may be taller than maxlevel: patchFromStream adds nodes and leaves maxlevel as it was.
//   P2 enterpoint n > 0: enterpoint < n.
//                   up_base[enterpoint] on the host (host_tiles.hpp ep_base_of); vec[enterpoint * dim], deleted[enterpoint] in
//                   every kernel's prologue (beam_search.hip descend).
//   P3 maxlevel   n > 0: maxlevel >= 0 and level(enterpoint) >= maxlevel.
//                   The descent starts at lvl = maxlevel and reads up_ptr[up_base[cur] + lvl - 1], up_ptr[.. + lvl] and
//                   uptile[(cur_b + lvl - 1) * up_stride + lane] with cur = enterpoint (beam_search.hip, flat_search.hip,
//                   lean_search.hip, slimq_search.hip): in bounds only if the enter point owns a level-maxlevel slot.
//   P4 threshold  threshold_level >= 0.
//                   The descent runs while lvl > threshold_level, the beams from min(threshold_level, maxlevel) down to 1
//                   (beam_search.hip strict kernel): a negative value takes lvl to 0 and below, up_ptr[b + lvl - 1] before b.
//                   Above maxlevel it is harmless (the min).
//   P5 count      every list fits its storage.  HierarchicalNSW: the u16 count word <= maxM0 on level 0, <= maxM above
//                   (from_vanilla copies `count` ids out of a block of that many).  CHAL blob: the u16 offsets are
//                   non-decreasing and <= total, and the blob holds 2 * level + 4 * total bytes (chal_slice below, the one copy
//                   of that test).  Arrays: list_ptr non-decreasing.
//   P6 id         every neighbour id < n, on every level.
//                   vec[id * dim], tile0[id * stride], row_ptr0[id], up_base[id], deleted[id], the visited set; on the host
//                   up_base[nb] in build_uptile and levels[id] in convertFromHNSW.
//   P7 owner      every id in a level-l list (l >= 1) names a node of level >= l.
//                   The descent and the threshold beams move to such an id and read its level-l slot, up_ptr[up_base[id] + l - 1
//                   .. + l]: a shorter node would hand out its successor's slots, the last owner the words past up_ptr's end.
//                   (A level-0 node has up_base NONE, which the kernels test; the rule is stated for every l all the same.)
//                   One exception, in hs_index_patch only: a named node that has no lists at all.  A diff arrives in chunks, each a
//                   stream of its own over the final element count, so an early chunk names new nodes whose records come in a
//                   later one; until then they are zeroed elements without a blob, up_base NONE, which every descent tests
//                   before it reads a slot (`if (b == kNone) continue`, beam_search.hip descend / strict_beam).
//   n == 0        nothing is checked: no kernel is launched on an empty index, and the header words of an empty file (enter point
//                 -1, maxlevel -1 as the reference writes them) are taken as they are.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace hs {

static constexpr const char *kCorruptText = "Index seems to be corrupted or unsupported";

// The level-lvl slice of a CHAL blob ([u16 cumulative offsets x level][u32 ids x total], hnswalg_slim.h:1981-2000) of a node of
// level L with `total` ids; false when the offsets or the blob's size do not allow it (P5).
inline bool chal_slice(int L, size_t total, const std::vector<char> &blob, int lvl, const uint32_t *&ids, size_t &cnt) {
  if (L < 0 || lvl < 0 || lvl > L || blob.size() < 2 * (size_t)L + 4 * total) return false;
  const uint16_t *off = (const uint16_t *)blob.data();
  const size_t s = lvl == 0 ? 0 : off[lvl - 1];
  const size_t e = lvl == L ? total : off[lvl];
  if (e < s || e > total) return false;
  ids = (const uint32_t *)(blob.data() + 2 * (size_t)L) + s;
  cnt = e - s;
  return true;
}

// P1 - P4.  strict_levels: the image is a HierarchicalNSW one (or a caller's arrays), whose levels end at maxlevel.
template <class LevelOf>
inline const char *check_entry(size_t n, uint32_t enterpoint, int maxlevel, int threshold_level, bool strict_levels, LevelOf level_of) {
  if (n == 0) return nullptr;
  for (size_t i = 0; i < n; i++) {
    if (level_of(i) < 0) return "P1 level: a node's level is negative";
    if (strict_levels && level_of(i) > maxlevel) return "P1 level: a node's level is above maxlevel";
  }
  if (enterpoint >= n) return "P2 enterpoint: enter point >= element count";
  if (maxlevel < 0) return "P3 maxlevel: negative with elements present";
  if (level_of(enterpoint) < maxlevel) return "P3 maxlevel: the enter point's level is below maxlevel";
  if (threshold_level < 0) return "P4 threshold: threshold_level is negative";
  return nullptr;
}

// P5 - P7 over every list.  list_of(i, l, ids, cnt) -> false when list l of node i does not fit its storage (P5); it is asked for
// l = 0 .. level(i) of the nodes has_lists(i) says own lists.  unlisted_ok: P7's exception for a patch stream, a named node
// without lists passes whatever its level.  Call after check_entry (levels are >= 0).
template <class LevelOf, class HasLists, class ListOf>
inline const char *check_lists(size_t n, LevelOf level_of, HasLists has_lists, ListOf list_of, bool unlisted_ok = false) {
  for (size_t i = 0; i < n; i++) {
    if (!has_lists(i)) continue;
    const int L = level_of(i);
    for (int l = 0; l <= L; l++) {
      const uint32_t *ids = nullptr;
      size_t cnt = 0;
      if (!list_of(i, l, ids, cnt)) return "P5 count: a list does not fit its storage";
      for (size_t j = 0; j < cnt; j++) {
        uint32_t id;   // (the ids of a CHAL blob lie 2 * level bytes into it: not aligned when the level is odd)
        memcpy(&id, (const char *)ids + 4 * j, 4);
        if (id >= n) return "P6 id: neighbour id >= element count";
        if (l > 0 && level_of(id) < l && !(unlisted_ok && !has_lists(id))) return "P7 owner: an upper list names a node below its level";
      }
    }
  }
  return nullptr;
}

// A graph of CHAL blobs (HierarchicalNSWSlim, HierarchicalNSWSlimQ, a Slim image with a staged patch over it): a node whose blob
// is empty has no lists at all (neighbors == nullptr, hnswalg_slim.h:247-249).
template <class LevelOf, class TotalOf, class BlobOf>
inline const char *check_chal(size_t n, uint32_t enterpoint, int maxlevel, int threshold_level, LevelOf level_of, TotalOf total_of, BlobOf blob_of,
                              bool unlisted_ok = false) {
  if (const char *bad = check_entry(n, enterpoint, maxlevel, threshold_level, false, level_of)) return bad;
  return check_lists(n, level_of, [&](size_t i) { return !blob_of(i).empty(); },
                     [&](size_t i, int l, const uint32_t *&ids, size_t &cnt) { return chal_slice(level_of(i), total_of(i), blob_of(i), l, ids, cnt); },
                     unlisted_ok);
}

}  // namespace hs
