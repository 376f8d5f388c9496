// tests/facade_exact.cpp -- searchKnnExact / searchKnnExactBatch through the facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h): the exact
// scan over the rows of a resident index.  One searchKnnExact call per query, taking turns between no functor and two functors (the
// functors go through the one-row filter-set cache that searchKnn(q, k, isIdAllowed) uses), then the whole batch unfiltered.
// usage: facade_exact <hnsw|slim> <index.bin> <dim> <queries.f32> <nq> <k> <out.bin>
//   out.bin: per query u32 count, count x {f32 dist, u64 label} closest first; then the batch: nq*k u64 labels, nq*k f32 dists, nq u32 counts
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

struct EveryOther : hnswlib::BaseFilterFunctor {
  bool operator()(hnswlib::labeltype id) override { return id % 2 == 0; }
};
struct NotThirds : hnswlib::BaseFilterFunctor {
  bool operator()(hnswlib::labeltype id) override { return id % 3 != 0; }
};

template <class Index>
static int run(Index &ix, const std::vector<float> &Q, size_t dim, size_t nq, size_t k, std::ofstream &out) {
  EveryOther f0;
  NotThirds f1;
  hnswlib::BaseFilterFunctor *fs[3] = {nullptr, &f0, &f1};
  for (size_t i = 0; i < nq; i++) {
    auto pq = ix.searchKnnExact(Q.data() + i * dim, k, fs[i % 3]);
    std::vector<std::pair<float, hnswlib::labeltype>> r;
    while (!pq.empty()) { r.push_back(pq.top()); pq.pop(); }   // farthest first, ties by the larger label first
    std::reverse(r.begin(), r.end());
    const uint32_t c = (uint32_t)r.size();
    out.write((const char *)&c, 4);
    for (auto &p : r) { const uint64_t l = p.second; out.write((const char *)&p.first, 4); out.write((const char *)&l, 8); }
  }
  std::vector<uint64_t> labels(nq * k);
  std::vector<float> dists(nq * k);
  std::vector<uint32_t> counts(nq);
  ix.searchKnnExactBatch(Q.data(), nq, k, labels.data(), dists.data(), counts.data());
  out.write((const char *)labels.data(), labels.size() * 8);
  out.write((const char *)dists.data(), dists.size() * 4);
  out.write((const char *)counts.data(), counts.size() * 4);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 8) return 2;
  const std::string mode = argv[1];
  const size_t dim = atoi(argv[3]), nq = atoi(argv[5]), k = atoi(argv[6]);
  std::vector<float> Q(nq * dim);
  std::ifstream(argv[4], std::ios::binary).read((char *)Q.data(), Q.size() * 4);
  hnswlib::L2Space space(dim);
  std::ofstream out(argv[7], std::ios::binary);
  if (mode == "slim") {
    hnswlib::HierarchicalNSWSlim<float> ix(&space, argv[2]);
    return run(ix, Q, dim, nq, k, out);
  }
  hnswlib::HierarchicalNSW<float> ix(&space, argv[2]);
  return run(ix, Q, dim, nq, k, out);
}
