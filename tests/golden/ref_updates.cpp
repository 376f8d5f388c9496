// tests/golden/ref_updates.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product, never run by a test).
//
// A driver of our own around the reference's vanilla hnswlib headers, which make_golden_updates.py compiles by -I from where
// they lie: it loads an index file, applies a list of operations through the reference's own addPoint / markDelete /
// unmarkDelete / resizeIndex (hnswalg.h:689-717, 923-1001, 1025-1272), saves (saveIndex), then searches the index it holds.
//
//   ref_updates <l2|ip> <dim> <in.index> <max_elements> <allow_replace_deleted 0|1> <ops.bin> <rows.f32> <out.index>
//               <queries.f32> <nq> <res.bin> <k> <ef> [ef...] [-- <steps_dir> <checkpoint> [checkpoint...]]
//
// ops.bin : n_ops x 4 little-endian u64 {kind, label or new capacity, replace flag, row index}; kinds add = 0, mark = 1,
//           unmark = 2, resize = 3 (the list hs_hnsw_replay takes).  rows.f32: the rows the add operations index, row-major.
// res.bin : what the oracle's reference driver writes for `search`: u32 nq, u32 k, u32 n_ef, then per ef: u32 ef, per query:
//           u32 cnt, u32 n_dist_calls, cnt x {f32 dist, u64 label} in priority_queue pop order (farthest first).
// With `-- steps_dir checkpoints`: after operation i (from 0) the index is saved as <steps_dir>/op<i>.bin, so that the caller can
// digest every state; a checkpoint c means "after the first c operations", where the searches above also run into
// <steps_dir>/res<c>.bin; and <steps_dir>/facts.u32 receives per operation 8 x u32 {flagged add that reused a vacancy, internal id
// the operation named or wrote (~0 for a resize), that id's level, enter point before the operation, element count, marks and
// capacity after it, max level after it}.
#include "hnswlib.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

static long g_dist_calls = 0;
static hnswlib::DISTFUNC<float> g_real_fn = nullptr;
static float counting_fn(const void *a, const void *b, const void *p) {
  g_dist_calls++;
  return g_real_fn(a, b, p);
}

template <typename T>
static std::vector<T> slurp(const char *path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::vector<T> out(raw.size() / sizeof(T));
  memcpy(out.data(), raw.data(), out.size() * sizeof(T));
  return out;
}

// searchKnn of every query at every ef, with the distance calls counted; the index's own distance function is put back.
static void search_all(hnswlib::HierarchicalNSW<float> &index, const std::vector<float> &Q, uint32_t nq, size_t dim, uint32_t k,
                       const std::vector<uint32_t> &efs, const std::string &path) {
  g_real_fn = index.fstdistfunc_;
  index.fstdistfunc_ = counting_fn;
  std::ofstream out(path, std::ios::binary);
  const uint32_t nef = efs.size();
  out.write((const char *)&nq, 4); out.write((const char *)&k, 4); out.write((const char *)&nef, 4);
  for (uint32_t ef : efs) {
    index.setEf(ef);
    out.write((const char *)&ef, 4);
    for (uint32_t i = 0; i < nq; i++) {
      g_dist_calls = 0;
      auto res = index.searchKnn(Q.data() + (size_t)i * dim, k);
      const uint32_t cnt = res.size(), calls = g_dist_calls;
      out.write((const char *)&cnt, 4); out.write((const char *)&calls, 4);
      while (!res.empty()) {
        const float d = res.top().first;
        const uint64_t label = res.top().second;
        out.write((const char *)&d, 4); out.write((const char *)&label, 8);
        res.pop();
      }
    }
  }
  index.fstdistfunc_ = g_real_fn;
}

int main(int argc, char **argv) {
  if (argc < 14) { fprintf(stderr, "usage: see the head of ref_updates.cpp\n"); return 2; }
  const std::string metric = argv[1];
  const size_t dim = atoll(argv[2]);
  hnswlib::SpaceInterface<float> *space =
      metric == "ip" ? (hnswlib::SpaceInterface<float> *)new hnswlib::InnerProductSpace(dim) : new hnswlib::L2Space(dim);
  hnswlib::HierarchicalNSW<float> index(space, argv[3], false, (size_t)atoll(argv[4]), atoi(argv[5]) != 0);
  const std::vector<uint64_t> ops = slurp<uint64_t>(argv[6]);
  const std::vector<float> rows = slurp<float>(argv[7]);
  const std::vector<float> Q = slurp<float>(argv[9]);
  const uint32_t nq = atoi(argv[10]), k = atoi(argv[12]);
  std::vector<uint32_t> efs;
  int a = 13;
  for (; a < argc && strcmp(argv[a], "--"); a++) efs.push_back(atoi(argv[a]));
  std::string steps;
  std::vector<size_t> checkpoints;
  if (a + 1 < argc) {
    steps = argv[a + 1];
    for (a += 2; a < argc; a++) checkpoints.push_back(atoll(argv[a]));
  }
  std::vector<uint32_t> facts;
  size_t reused = 0;
  for (size_t o = 0; o + 3 < ops.size(); o += 4) {
    const uint64_t kind = ops[o], arg = ops[o + 1], flag = ops[o + 2], row = ops[o + 3];
    const uint32_t ep_before = index.enterpoint_node_;
    uint32_t took = 0;
    if (kind == 0) {
      const size_t before = index.cur_element_count, lookup_before = index.label_lookup_.size();
      index.addPoint(rows.data() + row * dim, arg, flag != 0);
      if (flag && index.cur_element_count == before && index.label_lookup_.size() == lookup_before) { reused++; took = 1; }
    } else if (kind == 1) {
      index.markDelete(arg);
    } else if (kind == 2) {
      index.unmarkDelete(arg);
    } else if (kind == 3) {
      index.resizeIndex(arg);
    } else {
      fprintf(stderr, "bad op kind %llu\n", (unsigned long long)kind);
      return 2;
    }
    if (!steps.empty()) {
      const size_t i = o / 4;
      const uint32_t id = kind == 3 ? ~0u : index.label_lookup_.at(arg);
      const uint32_t fact[8] = {took, id, kind == 3 ? 0u : (uint32_t)index.element_levels_[id], ep_before, (uint32_t)index.cur_element_count,
                                (uint32_t)index.num_deleted_, (uint32_t)index.max_elements_, (uint32_t)index.maxlevel_};
      facts.insert(facts.end(), fact, fact + 8);
      index.saveIndex(steps + "/op" + std::to_string(i) + ".bin");
      for (size_t c : checkpoints)
        if (c == i + 1) search_all(index, Q, nq, dim, k, efs, steps + "/res" + std::to_string(c) + ".bin");
    }
  }
  if (!steps.empty()) {
    std::ofstream f(steps + "/facts.u32", std::ios::binary);
    f.write((const char *)facts.data(), facts.size() * 4);
  }
  index.saveIndex(argv[8]);
  printf("n=%zu max=%zu deleted=%zu maxlevel=%d ep=%u flagged adds that did not grow the index=%zu\n", (size_t)index.cur_element_count,
         (size_t)index.max_elements_, (size_t)index.num_deleted_, index.maxlevel_, index.enterpoint_node_, reused);
  search_all(index, Q, nq, dim, k, efs, argv[11]);
  return 0;
}
