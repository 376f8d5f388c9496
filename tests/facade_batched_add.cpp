// tests/facade_batched_add.cpp -- a caller that grows a resident index by a block of rows through the facade
// (hnsw-slim_amd/hnswlib/hnswlib_amd.h): loadIndex with room, setBuildOnDevice, addPoints, searchKnnBatch, saveIndex.
// usage: facade_batched_add <index.bin> <max_elements> <rows.f32> <count> <dim> <device (-1: setBuildOnDevice is not called)> <batch_max>
//                           <queries.f32> <nq> <k> <out.bin> <saved.bin>
//   row i is added as label 5000 + i; out.bin: {nq*k u64 labels, nq*k f32 dists, nq u32 counts} at ef 64
//   stdout: "add: <used_gpu> <batches> <flagged_rows> <element count>"
#include <cstdio>
#include <fstream>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

int main(int argc, char **argv) {
  if (argc < 13) return 2;
  const size_t max_elements = atoi(argv[2]), count = atoi(argv[4]), dim = atoi(argv[5]), batch_max = atoi(argv[7]), nq = atoi(argv[9]),
               k = atoi(argv[10]);
  const int device = atoi(argv[6]);
  std::vector<float> rows(count * dim), Q(nq * dim);
  std::ifstream(argv[3], std::ios::binary).read((char *)rows.data(), rows.size() * 4);
  std::ifstream(argv[8], std::ios::binary).read((char *)Q.data(), Q.size() * 4);
  std::vector<hnswlib::labeltype> labels(count);
  for (size_t i = 0; i < count; i++) labels[i] = 5000 + i;
  hnswlib::L2Space space(dim);
  hnswlib::HierarchicalNSW<float> ix(&space, argv[1], false, max_elements);
  if (device >= 0) ix.setBuildOnDevice(device, batch_max);
  ix.addPoints(rows.data(), labels.data(), count);
  ix.setEf(64);
  std::vector<uint64_t> out_labels(nq * k);
  std::vector<float> dists(nq * k);
  std::vector<uint32_t> counts(nq);
  ix.searchKnnBatch(Q.data(), nq, k, out_labels.data(), dists.data(), counts.data());
  std::ofstream out(argv[11], std::ios::binary);
  out.write((const char *)out_labels.data(), out_labels.size() * 8);
  out.write((const char *)dists.data(), dists.size() * 4);
  out.write((const char *)counts.data(), counts.size() * 4);
  ix.saveIndex(argv[12]);
  const hs_batch_build_stats &st = ix.buildStats();
  printf("add: %d %llu %llu %zu\n", (int)st.used_gpu, (unsigned long long)st.batches, (unsigned long long)st.flagged_rows, ix.getCurrentElementCount());
  return 0;
}
