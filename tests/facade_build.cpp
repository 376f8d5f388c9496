// tests/facade_build.cpp -- a build-then-search caller whose deferred build runs on the device, through the facade
// (hnsw-slim_amd/hnswlib/hnswlib_amd.h): constructor, addPoint loop, setBuildOnDevice, searchKnnBatch, saveIndex.
// usage: facade_build <rows.f32> <n> <dim> <M> <efc> <device (-1: setBuildOnDevice is not called)> <batch_max> <queries.f32> <nq> <k> <out.bin> <saved.bin>
//   row i is added as label 1000 + i; out.bin: {nq*k u64 labels, nq*k f32 dists, nq u32 counts} at ef 64
//   stdout: "build: <used_gpu> <batches> <flagged_rows>"
#include <cstdio>
#include <fstream>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

int main(int argc, char **argv) {
  if (argc < 13) return 2;
  const size_t n = atoi(argv[2]), dim = atoi(argv[3]), M = atoi(argv[4]), efc = atoi(argv[5]), batch_max = atoi(argv[7]), nq = atoi(argv[9]),
               k = atoi(argv[10]);
  const int device = atoi(argv[6]);
  std::vector<float> rows(n * dim), Q(nq * dim);
  std::ifstream(argv[1], std::ios::binary).read((char *)rows.data(), rows.size() * 4);
  std::ifstream(argv[8], std::ios::binary).read((char *)Q.data(), Q.size() * 4);
  hnswlib::L2Space space(dim);
  hnswlib::HierarchicalNSW<float> ix(&space, n, M, efc, "4", 100);
  if (device >= 0) ix.setBuildOnDevice(device, batch_max);
  for (size_t i = 0; i < n; i++) ix.addPoint(rows.data() + i * dim, 1000 + i);
  ix.setEf(64);
  std::vector<uint64_t> labels(nq * k);
  std::vector<float> dists(nq * k);
  std::vector<uint32_t> counts(nq);
  ix.searchKnnBatch(Q.data(), nq, k, labels.data(), dists.data(), counts.data());
  std::ofstream out(argv[11], std::ios::binary);
  out.write((const char *)labels.data(), labels.size() * 8);
  out.write((const char *)dists.data(), dists.size() * 4);
  out.write((const char *)counts.data(), counts.size() * 4);
  ix.saveIndex(argv[12]);
  const hs_batch_build_stats &st = ix.buildStats();
  printf("build: %d %llu %llu\n", (int)st.used_gpu, (unsigned long long)st.batches, (unsigned long long)st.flagged_rows);
  return 0;
}
