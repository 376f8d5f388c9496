// diff_prune_test.cpp -- host-only test of csrc/diff_prune.hpp, the two orders of getNeighborsByHeuristic2 that convert_diff.hip
// shares with the host: the candidate order (ascending distance, larger id first) and the pop order of the returned heap
// (push_heap / pop_heap emulation), against the heuristic written with std::priority_queue as hnswalg.h:481-523 writes it.
// Lists full of equal distances -- stars whose spokes all sit at one distance from the centre -- of M - 1, M, M + 1, 33 and 64
// ids, unions of `limit` and `limit + 1` ids, and random small-integer points (ties and pruning mixed).
// Build: g++ -std=c++17 -O2 diff_prune_test.cpp -o diff_prune_test   (also with -fsanitize=address,undefined)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <queue>
#include <random>
#include <vector>

#include "diff_prune.hpp"

using hs::Pair;
typedef std::pair<float, uint32_t> pfi;
struct CompareByFirst { bool operator()(const pfi &a, const pfi &b) const { return a.first < b.first; } };
typedef std::priority_queue<pfi, std::vector<pfi>, CompareByFirst> MaxQ;

static size_t g_dim;
static std::vector<float> g_rows;
static float dist(uint32_t a, uint32_t b) {
  float r = 0;
  for (size_t k = 0; k < g_dim; k++) { const float t = g_rows[a * g_dim + k] - g_rows[b * g_dim + k]; r += t * t; }
  return r;
}

// the reference's shape: heap in, heap out, then the caller's pops
static std::vector<uint32_t> by_priority_queue(uint32_t v, const std::vector<uint32_t> &ids, size_t M) {
  MaxQ top;
  for (uint32_t u : ids) top.emplace(dist(v, u), u);
  if (top.size() >= M) {
    std::priority_queue<pfi> closest;
    std::vector<pfi> ret;
    while (!top.empty()) { closest.emplace(-top.top().first, top.top().second); top.pop(); }
    while (!closest.empty()) {
      if (ret.size() >= M) break;
      const pfi cur = closest.top();
      const float dq = -cur.first;
      closest.pop();
      bool good = true;
      for (const pfi &s : ret)
        if (dist(s.second, cur.second) < dq) { good = false; break; }
      if (good) ret.push_back(cur);
    }
    for (const pfi &p : ret) top.emplace(-p.first, p.second);
  }
  std::vector<uint32_t> out;
  while (!top.empty()) { out.push_back(top.top().second); top.pop(); }
  return out;
}

// the kernels' shape: sort by the candidate order, sequential keep, emulated pop order
static std::vector<uint32_t> by_shared_code(uint32_t v, const std::vector<uint32_t> &ids, size_t M, bool &passed_through) {
  std::vector<Pair> arr;
  for (uint32_t u : ids) arr.push_back(Pair{dist(v, u), u});
  passed_through = arr.size() < M;
  std::vector<Pair> kept;
  if (passed_through) {
    kept = arr;   // the heap as it was filled: emplaces in list order
  } else {
    std::sort(arr.begin(), arr.end(), hs::h2_before);
    for (const Pair &c : arr) {
      if (kept.size() >= M) break;
      bool good = true;
      for (const Pair &s : kept)
        if (dist(s.id, c.id) < c.d) { good = false; break; }
      if (good) kept.push_back(c);
    }
  }
  hs::h2_pop_order(kept.data(), (long)kept.size());
  std::vector<uint32_t> out;
  for (size_t j = kept.size(); j-- > 0;) out.push_back(kept[j].id);
  return out;
}

static int check(const char *what, uint32_t v, const std::vector<uint32_t> &ids, size_t M, size_t &cases) {
  bool pt = false;
  const std::vector<uint32_t> want = by_priority_queue(v, ids, M), got = by_shared_code(v, ids, M, pt);
  cases++;
  if (want != got) {
    printf("MISMATCH %s: %zu ids, M = %zu\n", what, ids.size(), M);
    return 1;
  }
  return 0;
}

int main() {
  int bad = 0;
  size_t cases = 0;
  // stars: node 0 in the centre, spoke s at +-3 on axis s % dim -- every spoke at distance 9, spokes 18 or 36 apart
  g_dim = 32;
  g_rows.assign(65 * g_dim, 10.f);
  for (uint32_t s = 0; s < 64; s++) g_rows[(1 + s) * g_dim + s % g_dim] += s < g_dim ? 3.f : -3.f;
  const size_t M = 16, limit = 32;
  std::mt19937 rng(7);
  for (size_t n : {M - 1, M, M + 1, (size_t)33, (size_t)64, limit, limit + 1}) {
    std::vector<uint32_t> ids(n);
    for (size_t i = 0; i < n; i++) ids[i] = (uint32_t)(1 + i);
    for (int rep = 0; rep < 20; rep++) {
      for (size_t m : {M, limit, (size_t)8, (size_t)4}) bad += check("star", 0, ids, m, cases);
      std::shuffle(ids.begin(), ids.end(), rng);   // the source lists of phase 1 come in any order
    }
  }
  // small-integer points: equal distances and pruning mixed
  g_dim = 3;
  const uint32_t np = 200;
  g_rows.resize(np * g_dim);
  for (float &x : g_rows) x = (float)(int)(rng() % 7);
  for (int rep = 0; rep < 400; rep++) {
    const size_t n = 1 + rng() % 64;
    std::vector<uint32_t> all(np);
    for (uint32_t i = 0; i < np; i++) all[i] = i;
    std::shuffle(all.begin(), all.end(), rng);
    const uint32_t v = all.back();
    std::vector<uint32_t> ids(all.begin(), all.begin() + n);
    std::sort(ids.begin(), ids.end());   // the re-prune's emplace order (ascending id)
    for (size_t m : {(size_t)4, (size_t)8, M, limit}) bad += check("grid", v, ids, m, cases);
  }
  if (bad) { printf("diff_prune FAILED: %d of %zu cases\n", bad, cases); return 1; }
  printf("diff_prune ok: %zu cases\n", cases);
  return 0;
}
