// slimq_prune.hpp -- the closed form of HierarchicalNSWSlimQ's PruneByHeuristic (hnswalg_slimq.h:1334-1362; host_rq_graph.hpp
// prune_slimq) that convert_slimq.hip evaluates a chunk of candidates at a time, shared with its host-only test (slimq_prune_test.cpp).
//
// The reference's loop measures candidate i of the sorted list against the row whose INTERNAL ID is the loop index i, not against
// what it has kept, and only once something has been kept.  Candidate 0 is always kept when Mlim >= 1, so from i = 1 on something
// has been kept and the test of candidate i depends on nothing but i: the kept set is the first Mlim members of
//   {0}  U  { i >= 1 : !(d(row i, row id_i) < key_i) }
// in list order.  (A NaN compares false and keeps the candidate.)  Premise: row i exists, i.e. i < n.  The lists are distinct node
// ids below n -- a source list of node v after the host check of its length, a union after std::unique -- so a list of sz entries
// has sz <= n and i < sz <= n.
#pragma once
#include "hd.hpp"

namespace hs {

static constexpr uint32_t kSlimqPruneChunk = 16;   // candidates tested per round: four passes of four pair distances

// does candidate i survive its own test?  pair_d = d(row i, row id_i), key = its sort key d(node, id_i)
HS_HD bool slimq_keeps(uint32_t i, float pair_d, float key) { return i == 0 || !(pair_d < key); }

// One round over the candidates [base, base + cnt), cnt <= 64: `good` has bit j set when candidate base + j survives.  With kc
// entries kept before the round, candidate base + j goes to slot slimq_slot(good, j, kc) of the kept list when that slot is below
// mlim, and the round leaves slimq_kept_after(good, kc, mlim) entries kept; the loop over rounds runs while that is below mlim.
HS_HD uint32_t slimq_slot(unsigned long long good, uint32_t j, uint32_t kc) { return kc + (uint32_t)__builtin_popcountll(good & ((1ull << j) - 1ull)); }
HS_HD uint32_t slimq_kept_after(unsigned long long good, uint32_t kc, uint32_t mlim) {
  const uint32_t k = kc + (uint32_t)__builtin_popcountll(good);
  return k < mlim ? k : mlim;
}

}  // namespace hs
