// sorted_insert_test.cpp -- host test of sorted_insert.hpp (the flat kernel's rank-free insertion into its sorted result set).
//
// The lane-wise function is replayed over the 64 lanes of a wave (the DPP wave_shr:1 of the kernel becomes "slot S - 1 of the
// lane to the left, as it was before the insertion") and held against two independent statements of the same operation:
//   * the reference: std::upper_bound + insert into a vector of 64 * S entries, the last one dropped -- an entry whose key equals
//     existing keys lands behind them;
//   * the rank path the kernel used before: pos = number of keys <= kj, everything from pos up moves one rank, (kj, idj) at pos.
// Cases per S in {1, 2, 3, 4, 6, 8}: full sets and sets padded with the kernel's (+inf key, done-flag id) entries, keys drawn from
// a wide range and from a handful of values (ties), keys equal to existing keys, to the smallest key, to the key of the last rank
// (the bound) and -- which the kernel never inserts, but the function must still get right -- beyond it; negative keys (inner
// product); sequences of 1..8 insertions in a row.  Every rank of both arrays (keys AND ids) is compared after every insertion.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sorted_insert.hpp"

namespace {

constexpr int kInf = 0x7F800000;          // flat_search.hip: kFKeyInf
constexpr uint32_t kDone = 0x80000000u;   // flat_search.hip: kFDone

struct Entry { int k; uint32_t i; };
bool operator==(const Entry &a, const Entry &b) { return a.k == b.k && a.i == b.i; }

template <int S>
void lanewise_insert(std::vector<Entry> &set, int kj, uint32_t idj) {
  int tk[64][S];
  uint32_t ti[64][S];
  for (int l = 0; l < 64; l++)
    for (int s = 0; s < S; s++) { tk[l][s] = set[l * S + s].k; ti[l][s] = set[l * S + s].i; }
  // every lane sees its left neighbour's OLD last slot
  int upk[64];
  uint32_t upi[64];
  for (int l = 0; l < 64; l++) {
    upk[l] = l == 0 ? hs::kInsertKeyMin : tk[l - 1][S - 1];
    upi[l] = l == 0 ? 0u : ti[l - 1][S - 1];
  }
  for (int l = 0; l < 64; l++) hs::sorted_insert_lane<S>(tk[l], ti[l], upk[l], upi[l], kj, idj);
  for (int l = 0; l < 64; l++)
    for (int s = 0; s < S; s++) set[l * S + s] = Entry{tk[l][s], ti[l][s]};
}

void reference_insert(std::vector<Entry> &set, int kj, uint32_t idj) {
  auto at = std::upper_bound(set.begin(), set.end(), kj, [](int key, const Entry &e) { return key < e.k; });
  set.insert(at, Entry{kj, idj});
  set.pop_back();
}

void rank_insert(std::vector<Entry> &set, int kj, uint32_t idj) {
  size_t pos = 0;
  for (const Entry &e : set) pos += e.k <= kj ? 1 : 0;
  if (pos >= set.size()) return;
  for (size_t r = set.size() - 1; r > pos; r--) set[r] = set[r - 1];
  set[pos] = Entry{kj, idj};
}

template <int S>
long run(std::mt19937 &rng) {
  const int N = 64 * S;
  long checks = 0;
  for (int round = 0; round < 400; round++) {
    // a sorted set: `fill` real entries, padding behind them
    const int fill_kind = round % 4;
    const int fill = fill_kind == 0 ? N : fill_kind == 1 ? 0 : fill_kind == 2 ? 1 + (int)(rng() % (unsigned)(N - 1)) : N - 1;
    const int span_kind = (round / 4) % 3;   // wide range | a handful of values | negative and positive
    auto draw = [&]() -> int {
      if (span_kind == 0) return (int)(rng() % 0x7F000000u);
      if (span_kind == 1) return 1000 + (int)(rng() % 5u);
      return (int)(rng() % 2001u) - 1000;
    };
    std::vector<Entry> set((size_t)N, Entry{kInf, kDone});
    for (int r = 0; r < fill; r++) set[(size_t)r] = Entry{draw(), (uint32_t)(rng() % 1000000u) | ((rng() & 1u) ? kDone : 0u)};
    std::stable_sort(set.begin(), set.begin() + fill, [](const Entry &a, const Entry &b) { return a.k < b.k; });
    std::vector<Entry> ref = set, old = set;
    const int n_ins = 1 + round % 8;
    for (int j = 0; j < n_ins; j++) {
      int kj;
      switch (rng() % 6u) {
        case 0: kj = ref[(size_t)(rng() % (unsigned)N)].k; break;   // equal to an existing key (padding's +inf included)
        case 1: kj = ref[(size_t)N - 1].k; break;                    // equal to the key of the last rank
        case 2: kj = ref[0].k; break;                                // equal to the smallest key
        case 3: kj = ref[0].k == hs::kInsertKeyMin + 1 ? ref[0].k : ref[0].k - 1; break;   // in front of everything
        default: kj = draw(); break;
      }
      const uint32_t idj = 2000000u + (uint32_t)j;
      lanewise_insert<S>(set, kj, idj);
      reference_insert(ref, kj, idj);
      rank_insert(old, kj, idj);
      for (int r = 0; r < N; r++) {
        if (!(set[(size_t)r] == ref[(size_t)r]) || !(old[(size_t)r] == ref[(size_t)r])) {
          std::printf("FAIL S=%d round=%d insert=%d key=%d rank=%d: lane-wise (%d,%u) rank path (%d,%u) reference (%d,%u)\n", S, round, j, kj, r,
                      set[(size_t)r].k, set[(size_t)r].i, old[(size_t)r].k, old[(size_t)r].i, ref[(size_t)r].k, ref[(size_t)r].i);
          std::exit(1);
        }
        checks++;
      }
    }
  }
  return checks;
}

}  // namespace

int main() {
  std::mt19937 rng(20240611u);
  long checks = 0;
  checks += run<1>(rng);
  checks += run<2>(rng);
  checks += run<3>(rng);
  checks += run<4>(rng);
  checks += run<6>(rng);
  checks += run<8>(rng);
  std::printf("sorted_insert ok: S in {1,2,3,4,6,8}, %ld rank comparisons\n", checks);
  return 0;
}
