// tests/facade_rq_build.cpp -- the build chain of the reference's SlimQ strategy (include/strategy/hnsw_slimq_strategy.h:53-57,
// 106-158) through the facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h): rabitqlib::hnsw::HierarchicalNSW's constructor, construct() on
// the device, save(), HierarchicalNSWSlimQ::convertFromHNSW, saveIndex, setDataset, setEf, searchKnn(q, K, result).
// usage: facade_rq_build <rows.f32> <n> <dim> <M> <efc> <device (-1: setBuildOnDevice is not called)> <batch_max> <centroids.f32> <n_centroids>
//                        <queries.f32> <nq> <k> <ef> <out.bin> <saved_hnsw.bin> <saved_slimq.bin>
//   out.bin: nq*k u32 labels; stdout: "build: <used_gpu> <batches> <flagged_rows>"
#include <cstdio>
#include <fstream>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

int main(int argc, char **argv) {
  if (argc < 17) return 2;
  const size_t n = atoi(argv[2]), dim = atoi(argv[3]), M = atoi(argv[4]), efc = atoi(argv[5]), batch_max = atoi(argv[7]), nc = atoi(argv[9]),
               nq = atoi(argv[11]), k = atoi(argv[12]), ef = atoi(argv[13]);
  const int device = atoi(argv[6]);
  std::vector<float> rows(n * dim), cen(nc * dim), Q(nq * dim);
  std::ifstream(argv[1], std::ios::binary).read((char *)rows.data(), rows.size() * 4);
  std::ifstream(argv[8], std::ios::binary).read((char *)cen.data(), cen.size() * 4);
  std::ifstream(argv[10], std::ios::binary).read((char *)Q.data(), Q.size() * 4);
  hnswlib::L2Space l2space(dim);
  hnswlib::HierarchicalNSWSlimQ<float> hnsw_slimq(&l2space, n, M, efc);
  auto *hnsw = new rabitqlib::hnsw::HierarchicalNSW(n, dim, 4, M, efc, 100, rabitqlib::METRIC_L2);
  if (device >= 0) hnsw->setBuildOnDevice(device, batch_max);
  hnsw->construct(nc, cen.data(), n, rows.data(), nullptr, 0, true);
  hnsw->save(argv[15]);
  hnsw_slimq.convertFromHNSW(hnsw);
  hnsw_slimq.saveIndex(argv[16]);
  hnsw_slimq.setDataset(rows.data(), n, dim);
  hnsw_slimq.setEf(ef);
  std::vector<hnswlib::tableint> labels(nq * k);
  for (size_t i = 0; i < nq; i++) hnsw_slimq.searchKnn(Q.data() + i * dim, k, labels.data() + i * k);
  std::ofstream(argv[14], std::ios::binary).write((const char *)labels.data(), labels.size() * 4);
  const hs_batch_build_stats &st = hnsw->buildStats();
  printf("build: %d %llu %llu\n", (int)st.used_gpu, (unsigned long long)st.batches, (unsigned long long)st.flagged_rows);
  delete hnsw;
  return 0;
}
