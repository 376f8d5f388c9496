// tests/facade_slimq_convert.cpp -- HierarchicalNSWSlimQ::convertFromHNSW through the facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h)
// both ways: construct -> convertFromHNSW -> saveIndex once as the facade always did (two host calls through a temporary file) and
// once after setBuildOnDevice(device) (both steps on the device, chained in memory), and the two saved files compared.
// usage: facade_slimq_convert <rows.f32> <n> <dim> <M> <efc> <metric 0|1> <device> <centroids.f32> <n_centroids> <host_slimq.bin> <device_slimq.bin>
//   stdout: "convert: <graph_used_gpu> <records_used_gpu> <files equal 0|1>"; exit status 1 when the files differ
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

static std::vector<char> slurp(const char *p) {
  std::ifstream in(p, std::ios::binary);
  return std::vector<char>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
  if (argc < 12) return 2;
  const size_t n = atoi(argv[2]), dim = atoi(argv[3]), M = atoi(argv[4]), efc = atoi(argv[5]), nc = atoi(argv[9]);
  const int metric = atoi(argv[6]), device = atoi(argv[7]);
  std::vector<float> rows(n * dim), cen(nc * dim);
  std::ifstream(argv[1], std::ios::binary).read((char *)rows.data(), rows.size() * 4);
  std::ifstream(argv[8], std::ios::binary).read((char *)cen.data(), cen.size() * 4);
  hnswlib::L2Space l2space(dim);
  hnswlib::InnerProductSpace ipspace(dim);
  hnswlib::SpaceInterface<float> *space = metric ? (hnswlib::SpaceInterface<float> *)&ipspace : (hnswlib::SpaceInterface<float> *)&l2space;
  rabitqlib::hnsw::HierarchicalNSW hnsw(n, dim, 4, M, efc, 100, metric ? rabitqlib::METRIC_IP : rabitqlib::METRIC_L2);
  hnsw.construct(nc, cen.data(), n, rows.data(), nullptr, 1, true);
  hnswlib::HierarchicalNSWSlimQ<float> on_host(space, n, M, efc), on_device(space, n, M, efc);
  on_host.convertFromHNSW(&hnsw);
  on_host.saveIndex(argv[10]);
  on_device.setBuildOnDevice(device);
  on_device.convertFromHNSW(&hnsw);
  on_device.saveIndex(argv[11]);
  const hs_slimq_convert_stats &st = on_device.convertStats();
  const bool equal = slurp(argv[10]) == slurp(argv[11]);
  printf("convert: %d %d %d\n", st.graph_used_gpu, st.records_used_gpu, (int)equal);
  return equal ? 0 : 1;
}
