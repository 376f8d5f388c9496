// sorted_insert.hpp -- insertion into the flat kernel's sorted result set without computing the rank of the new entry.
//
// The set is an array of (key, id) sorted by key, rank r in lane r / S, slot r % S (flat_search.hip).  Inserting (kj, idj) behind
// every entry with key <= kj moves the entries with key > kj up by one rank (the last one falls off the end) and puts the new
// entry in the gap.  Seen from one rank r, with `prev` the entry one rank below (slot s - 1 of the same lane, or slot S - 1 of
// the lane to the left; a key below every key for rank 0):
//
//     key[r] <= kj                  : the entry stays
//     key[r] >  kj, prev.key >  kj  : the entry from one rank below arrives
//     key[r] >  kj, prev.key <= kj  : this is the gap -- the new entry
//
// i.e. key[r] = key[r] > kj ? max(prev.key, kj) : key[r], and the id likewise.  No lane needs the rank of the gap: no ballot,
// no population count, no division by S, no write to a computed lane.  Entries whose key EQUALS kj stay in front of the new one,
// which is where std::upper_bound would put it.
//
// The function is what ONE lane does; the device passes the left neighbour's last slot in through a DPP wave_shr:1, the host test
// (sorted_insert_test.cpp) replays it lane by lane against std::upper_bound + insert.
#pragma once
#include <climits>

#include "hd.hpp"

namespace hs {

static constexpr int kInsertKeyMin = INT_MIN;   // `up_k` of lane 0: below every key (dkey() never yields it)

// tk / ti: this lane's S slots, ascending rank.  (up_k, up_i): slot S - 1 of the lane to the left as it was BEFORE this insertion.
template <int S>
HS_HD void sorted_insert_lane(int (&tk)[S], uint32_t (&ti)[S], const int up_k, const uint32_t up_i, const int kj, const uint32_t idj) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int s = S - 1; s >= 0; s--) {   // downwards: slot s reads slot s - 1 before that one is rewritten
    const int pk = s > 0 ? tk[s - 1] : up_k;
    const uint32_t pi = s > 0 ? ti[s - 1] : up_i;
    const bool gt = tk[s] > kj;
    const int mk = pk > kj ? pk : kj;
    const uint32_t mi = pk > kj ? pi : idj;
    tk[s] = gt ? mk : tk[s];
    ti[s] = gt ? mi : ti[s];
  }
}

}  // namespace hs
