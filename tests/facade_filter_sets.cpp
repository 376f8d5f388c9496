// tests/facade_filter_sets.cpp -- searchKnn(q, k, isIdAllowed) through the facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h): the functor's
// answers are cached as a one-row device filter set (hs_filter_set_*).  Two functors alternate over the queries, one searchKnn
// call per query, as a caller written against the reference's hnswlib API would issue them.
// usage: facade_filter_sets <hnsw|slim> <index.bin> <dim> <queries.f32> <nq> <k> <ef> <out.bin>
//   out.bin, per query: u32 count, count x {f32 dist, u64 label} closest first, u64 device bytes of the cached filter set
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
static int run(Index &ix, const std::vector<float> &Q, size_t dim, size_t nq, size_t k, size_t ef, std::ofstream &out) {
  ix.setEf(ef);
  EveryOther f0;
  NotThirds f1;
  for (size_t i = 0; i < nq; i++) {
    hnswlib::BaseFilterFunctor *f = (i & 1) ? (hnswlib::BaseFilterFunctor *)&f1 : (hnswlib::BaseFilterFunctor *)&f0;
    auto r = ix.searchKnnCloserFirst(Q.data() + i * dim, k, f);
    const uint32_t c = (uint32_t)r.size();
    out.write((const char *)&c, 4);
    for (auto &p : r) { const uint64_t l = p.second; out.write((const char *)&p.first, 4); out.write((const char *)&l, 8); }
    const uint64_t bytes = ix.filterCacheBytes();
    out.write((const char *)&bytes, 8);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 9) return 2;
  const std::string mode = argv[1];
  const size_t dim = atoi(argv[3]), nq = atoi(argv[5]), k = atoi(argv[6]), ef = atoi(argv[7]);
  std::vector<float> Q(nq * dim);
  std::ifstream(argv[4], std::ios::binary).read((char *)Q.data(), Q.size() * 4);
  hnswlib::L2Space space(dim);
  std::ofstream out(argv[8], std::ios::binary);
  if (mode == "slim") {
    hnswlib::HierarchicalNSWSlim<float> ix(&space, argv[2]);
    return run(ix, Q, dim, nq, k, ef, out);
  }
  hnswlib::HierarchicalNSW<float> ix(&space, argv[2]);
  return run(ix, Q, dim, nq, k, ef, out);
}
