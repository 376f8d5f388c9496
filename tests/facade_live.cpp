// tests/facade_live.cpp -- a resident vanilla index that changes, through the facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h):
// loadIndex with room, markDelete, searchKnnBatch, the reference's exception texts, unmarkDelete, getDataByLabel, addPoint until
// the index is full (and once more), searchKnnBatch, saveIndex.
// usage: facade_live <index.bin> <dim> <max_elements> <rows.f32> <nrows> <first_label> <queries.f32> <nq> <k> <every> <out.bin> <saved.bin>
//   marks the labels every/2, every/2 + every, ... below the loaded count; adds row i as label first_label + i
//   out.bin: {nq*k u64 labels, nq*k f32 dists, nq u32 counts} after the marks, dim f32 of getDataByLabel(1), the same triple after
//   the adds;  stdout: one line "what: text" per provoked exception, then "counts: <elements> <max> <deleted>"
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

template <class F>
static void expect_throw(const char *what, F f) {
  try {
    f();
    printf("%s: (no exception)\n", what);
  } catch (std::runtime_error &e) {
    printf("%s: %s\n", what, e.what());
  }
}

// facade_live grow <rows.f32> <n> <dim> <n_first> <saved.bin>: the build-then-search caller that goes on adding -- constructor with
// max_elements = n (M 16, ef_construction 100, branching "4", seed 100), addPoint of the first n_first rows, one searchKnn, addPoint
// of the rest (incremental: the index is resident by then), saveIndex
static int grow(int argc, char **argv) {
  if (argc < 7) return 2;
  const size_t n = atoi(argv[3]), dim = atoi(argv[4]), n_first = atoi(argv[5]);
  std::vector<float> rows(n * dim);
  std::ifstream(argv[2], std::ios::binary).read((char *)rows.data(), rows.size() * 4);
  hnswlib::L2Space space(dim);
  hnswlib::HierarchicalNSW<float> ix(&space, n, 16, 100, "4", 100);
  for (size_t i = 0; i < n_first; i++) ix.addPoint(rows.data() + i * dim, i);
  auto pq = ix.searchKnn(rows.data(), 5);
  if (pq.size() != 5 || ix.getCurrentElementCount() != n_first || ix.getMaxElements() != n) return 3;
  for (size_t i = n_first; i < n; i++) ix.addPoint(rows.data() + i * dim, i);
  if (ix.getCurrentElementCount() != n) return 4;
  ix.saveIndex(argv[6]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::string(argv[1]) == "grow") return grow(argc, argv);
  if (argc < 13) return 2;
  const size_t dim = atoi(argv[2]), cap = atoi(argv[3]), nrows = atoi(argv[5]), first_label = atoi(argv[6]), nq = atoi(argv[8]), k = atoi(argv[9]),
               every = atoi(argv[10]);
  std::vector<float> rows(nrows * dim), Q(nq * dim);
  std::ifstream(argv[4], std::ios::binary).read((char *)rows.data(), rows.size() * 4);
  std::ifstream(argv[7], std::ios::binary).read((char *)Q.data(), Q.size() * 4);
  hnswlib::L2Space space(dim);
  hnswlib::HierarchicalNSW<float> ix(&space, argv[1], false, cap);
  ix.setEf(32);
  std::ofstream out(argv[11], std::ios::binary);
  std::vector<uint64_t> labels(nq * k);
  std::vector<float> dists(nq * k);
  std::vector<uint32_t> counts(nq);
  auto search = [&]() {
    ix.searchKnnBatch(Q.data(), nq, k, labels.data(), dists.data(), counts.data());
    out.write((const char *)labels.data(), labels.size() * 8);
    out.write((const char *)dists.data(), dists.size() * 4);
    out.write((const char *)counts.data(), counts.size() * 4);
  };
  const size_t n0 = ix.getCurrentElementCount();
  for (size_t l = every / 2; l < n0; l += every) ix.markDelete(l);
  if (ix.getDeletedCount() != (n0 - every / 2 + every - 1) / every) return 3;
  search();
  expect_throw("mark twice", [&]() { ix.markDelete(every / 2); });
  expect_throw("unmark unmarked", [&]() { ix.unmarkDelete(every / 2 + 1); });
  expect_throw("mark unknown", [&]() { ix.markDelete(first_label + nrows + 7); });
  expect_throw("data of a deleted label", [&]() { (void)ix.getDataByLabel<float>(every / 2); });
  for (size_t l = every / 2; l < n0; l += every) ix.unmarkDelete(l);
  if (ix.getDeletedCount() != 0) return 4;
  const std::vector<float> row = ix.getDataByLabel<float>(1);
  out.write((const char *)row.data(), row.size() * 4);
  for (size_t i = 0; i < nrows; i++) ix.addPoint(rows.data() + i * dim, first_label + i);
  expect_throw("add beyond max_elements", [&]() { ix.addPoint(rows.data(), first_label + nrows); });
  search();
  ix.saveIndex(argv[12]);
  printf("counts: %zu %zu %zu\n", ix.getCurrentElementCount(), ix.getMaxElements(), ix.getDeletedCount());
  return 0;
}
