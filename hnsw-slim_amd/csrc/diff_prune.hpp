// diff_prune.hpp -- the two orders of hnsw->getNeighborsByHeuristic2 (hnswalg.h:481-523) as convertFromHNSWWithDiff uses it
// (hnswalg_slim.h:1223, 1296), shared by convert_diff.hip and the host test csrc/diff_prune_test.cpp:
//   * the candidate order: queue_closest is a std::priority_queue of (-distance, id) pairs with the default comparison, so the
//     candidates leave it by ascending distance and, among equal distances, LARGER id first -- a total order, any sort gives it;
//   * the pop order of the returned heap: the kept entries are emplaced, in the order they were kept, into a priority_queue that
//     compares distances only (CompareByFirst), and the caller pops it -- farthest first, equal distances in the order
//     libstdc++'s push_heap / pop_heap leave them (heap_emul.hpp).
#pragma once
#include "heap_emul.hpp"

namespace hs {

// a leaves queue_closest before b
HS_HD bool h2_before(const Pair &a, const Pair &b) { return a.d < b.d || (a.d == b.d && a.id > b.id); }

// h[0..kc) = the kept entries in kept order -> h[0..kc) = the same entries with h[kc - 1] the first one popped and h[0] the last:
// emplace one by one (push_heap), then pop_heap until empty (each pop parks the root behind the shrinking heap).
template <class P>
HS_HD void h2_pop_order(P *h, long kc) {
  for (long i = 1; i <= kc; i++) push_heap(h, i, LessD());
  for (long m = kc; m > 1; m--) pop_heap(h, m, LessD());
}

}  // namespace hs
