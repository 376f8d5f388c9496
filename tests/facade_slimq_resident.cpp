// tests/facade_slimq_resident.cpp -- the SlimQ chain through the facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h) with no file on the way:
// under setBuildOnDevice, rabitqlib::hnsw::HierarchicalNSW::construct keeps its graph in memory, HierarchicalNSWSlimQ<float>::
// convertFromHNSW makes a resident index from it, setDataset and searchKnn follow -- and neither object holds a temporary file.  The
// answers are those of an index loaded from saveIndex's file, and save() of the graph is what the file-based build writes.
// usage: facade_slimq_resident <scratch dir> [device]      stdout ends with "facade_slimq_resident ok"; exit status 1 otherwise
#include <cstdio>
#include <fstream>
#include <iterator>
#include <random>
#include <string>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

#define CHECK(c)                                                           \
  do {                                                                     \
    if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

static std::vector<char> slurp(const std::string &p) {
  std::ifstream in(p, std::ios::binary);
  return std::vector<char>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const int device = argc > 2 ? atoi(argv[2]) : 0;
  const size_t n = 2000, dim = 96, M = 16, efc = 64, nc = 6, nq = 64, k = 10;
  std::mt19937 gen(7);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<float> cen(nc * dim), rows(n * dim), q(nq * dim);
  for (float &x : cen) x = nd(gen);
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < dim; j++) rows[i * dim + j] = cen[(i % nc) * dim + j] + 0.35f * nd(gen);
  for (size_t i = 0; i < nq; i++)
    for (size_t j = 0; j < dim; j++) q[i * dim + j] = rows[(i * 31 % n) * dim + j] + 0.1f * nd(gen);

  hnswlib::L2Space space(dim);
  rabitqlib::hnsw::HierarchicalNSW hnsw(n, dim, 4, M, efc, 100, rabitqlib::METRIC_L2);
  hnsw.setBuildOnDevice(device);
  hnsw.construct(nc, cen.data(), n, rows.data(), nullptr, 8, true);
  CHECK(hnsw.buildStats().used_gpu == 1 && hnsw.graph() != nullptr);
  hnswlib::HierarchicalNSWSlimQ<float> index(&space, n, M, efc);
  index.setBuildOnDevice(device);
  index.convertFromHNSW(&hnsw);
  CHECK(index.convertStats().graph_used_gpu == 1 && index.convertStats().records_used_gpu == 1);
  index.setDataset(rows.data(), n, dim);
  index.setEf(64);
  std::vector<hnswlib::tableint> got(nq * k), one(k), want(nq * k);
  index.searchKnnBatch(q.data(), nq, k, got.data());
  index.searchKnn(q.data(), k, one.data());
  CHECK(std::equal(one.begin(), one.end(), got.begin()));
  // no file so far
  CHECK(hnsw.tempFile().empty() && index.tempFile().empty() && index.path().empty());

  // saveIndex writes the index's host image; an index loaded from that file answers the same
  const std::string qp = dir + "/resident.slimq", gp = dir + "/graph.bin", gp2 = dir + "/graph_file_build.bin";
  index.saveIndex(qp);
  CHECK(hnsw.tempFile().empty() && index.tempFile().empty());
  hnswlib::HierarchicalNSWSlimQ<float> loaded(&space, qp);
  loaded.setDataset(rows.data(), n, dim);
  loaded.setEf(64);
  loaded.searchKnnBatch(q.data(), nq, k, want.data());
  CHECK(got == want);
  CHECK(index.deviceBytes() == loaded.deviceBytes() && index.indexSize() == loaded.indexSize());

  // save() of the graph in memory: the bytes of the file-based batched build
  hnsw.save(gp.c_str());
  hs_batch_build_opts o{};
  o.device = device; o.threads = 8;
  CHECK(hs_build_rabitq_hnsw_batched(rows.data(), n, dim, HS_METRIC_L2, M, efc, 100, &o, gp2.c_str(), nullptr) == HS_OK);
  CHECK(slurp(gp) == slurp(gp2) && !slurp(gp).empty());
  CHECK(hnsw.tempFile().empty());
  // the host conversion still reads a file: graphPath() materialises one on demand, and the index it leads to is the same
  hnswlib::HierarchicalNSWSlimQ<float> on_host(&space, n, M, efc);
  on_host.convertFromHNSW(&hnsw);
  CHECK(!hnsw.tempFile().empty() && slurp(hnsw.tempFile()) == slurp(gp));
  const std::string qh = dir + "/host.slimq";
  on_host.saveIndex(qh);
  CHECK(slurp(qh) == slurp(qp));
  printf("facade_slimq_resident ok\n");
  return 0;
}
