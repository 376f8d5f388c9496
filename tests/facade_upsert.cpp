// tests/facade_upsert.cpp -- upsert, replace_deleted and resizeIndex through the facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h), as a
// caller of hnswlib's own API writes them: the allow_replace_deleted constructor flag, addPoint of an existing label,
// addPoint(.., true), markDelete, resizeIndex, saveIndex, and the reference's exception texts.
// usage: facade_upsert <index.bin> <dim> <max_elements> <ops.u64> <n_ops> <rows.f32> <queries.f32> <nq> <k> <out.bin> <saved.bin>
//   ops.u64: n_ops x {kind, label or new capacity, replace flag, row index} (add 0, mark 1, unmark 2, resize 3: hs_hnsw_replay's list)
//   The index is loaded with allow_replace_deleted = true and takes the operations; saved.bin is its saveIndex, out.bin
//   {nq*k u64 labels, nq*k f32 dists, nq u32 counts} of searchKnnBatch at ef 32 afterwards.
//   stdout: one line "what: text" per provoked exception and per check.
#include <cstdio>
#include <cstring>
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

template <typename T>
static std::vector<T> slurp(const char *path) {
  std::ifstream in(path, std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::vector<T> out(raw.size() / sizeof(T));
  memcpy(out.data(), raw.data(), out.size() * sizeof(T));
  return out;
}

int main(int argc, char **argv) {
  if (argc < 12) return 2;
  const size_t dim = atoi(argv[2]), cap = atoi(argv[3]), n_ops = atoi(argv[5]), nq = atoi(argv[8]), k = atoi(argv[9]);
  const std::vector<uint64_t> ops = slurp<uint64_t>(argv[4]);
  const std::vector<float> rows = slurp<float>(argv[6]), Q = slurp<float>(argv[7]);
  if (ops.size() < 4 * n_ops || Q.size() < nq * dim) return 2;
  hnswlib::L2Space space(dim);
  {
    hnswlib::HierarchicalNSW<float> off(&space, argv[1], false, cap);   // the constructor flag left at false
    expect_throw("replace without the flag", [&]() { off.addPoint(rows.data(), 999999, true); });
  }
  hnswlib::HierarchicalNSW<float> ix(&space, argv[1], false, cap, true);
  uint64_t last_marked = 0;
  for (size_t o = 0; o < n_ops; o++) {
    const uint64_t kind = ops[4 * o], arg = ops[4 * o + 1], flag = ops[4 * o + 2], row = ops[4 * o + 3];
    if (kind == 0) ix.addPoint(rows.data() + row * dim, arg, flag != 0);
    else if (kind == 1) { ix.markDelete(arg); last_marked = arg; }
    else if (kind == 2) ix.unmarkDelete(arg);
    else ix.resizeIndex(arg);
  }
  ix.saveIndex(argv[11]);
  ix.setEf(32);
  std::vector<uint64_t> labels(nq * k);
  std::vector<float> dists(nq * k);
  std::vector<uint32_t> counts(nq);
  ix.searchKnnBatch(Q.data(), nq, k, labels.data(), dists.data(), counts.data());
  std::ofstream out(argv[10], std::ios::binary);
  out.write((const char *)labels.data(), labels.size() * 8);
  out.write((const char *)dists.data(), dists.size() * 4);
  out.write((const char *)counts.data(), counts.size() * 4);
  out.close();
  // refusals (each leaves the index as it was), then growth beyond the loaded capacity
  expect_throw("update of a deleted label", [&]() { ix.addPoint(rows.data(), last_marked); });
  expect_throw("resize below the count", [&]() { ix.resizeIndex(10); });
  const size_t n = ix.getCurrentElementCount();
  ix.resizeIndex(n);
  expect_throw("add beyond max_elements", [&]() { ix.addPoint(rows.data(), 777001); });
  ix.resizeIndex(n + 1);
  ix.addPoint(rows.data() + dim, 777001);
  const std::vector<float> back = ix.getDataByLabel<float>(777001);
  const bool grown = ix.getCurrentElementCount() == n + 1 && ix.getMaxElements() == n + 1 && !memcmp(back.data(), rows.data() + dim, dim * 4);
  printf("after resize: %s\n", grown ? "ok" : "WRONG");
  {
    // an index loaded without room keeps no host image: resizeIndex loads its file again with the new capacity
    hnswlib::HierarchicalNSW<float> full(&space, argv[1]);
    const size_t n0 = full.getCurrentElementCount();
    full.setEf(48);
    full.resizeIndex(n0 + 5);
    full.addPoint(rows.data(), 777002);
    full.addPoint(rows.data() + dim, 3);   // an update
    const std::vector<float> r3 = full.getDataByLabel<float>(3);
    const bool ok = full.getCurrentElementCount() == n0 + 1 && full.getMaxElements() == n0 + 5 && full.ef_ == 48 && !memcmp(r3.data(), rows.data() + dim, dim * 4);
    printf("resize of an index loaded full: %s\n", ok ? "ok" : "WRONG");
    hnswlib::HierarchicalNSW<float> marked(&space, argv[1]);
    marked.markDelete(4);
    expect_throw("resize of an index loaded full after a mark", [&]() { marked.resizeIndex(n0 + 5); });
  }
  return 0;
}
