// tests/facade_narrow.cpp -- narrow rows through the hnswlib facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h): a build-then-search
// caller (include/strategy/hnsw_strategy.h:24-40 + hnsw_slim_strategy.h:83-103) on integer rows that asks for u8 rows.
// usage: facade_narrow <base.f32> <n> <dim> <queries.f32> <nq> <k> <ef> <out.u32>
// out: 6 words {slim rowFormat(), slim kernel is hs::flat_kernel_u8, vanilla rowFormat() before its build, after it, vanilla kernel
//      is hs::flat_kernel_u8, HierarchicalNSWSlimQ::setRowFormat threw}, then nq x k Slim labels (searchKnnBatch, nearest first),
//      then nq x k vanilla labels (searchKnnBatch; ~0 where fewer than k were found).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

static std::vector<float> read_f32(const char *p, size_t n) {
  std::vector<float> v(n);
  std::ifstream in(p, std::ios::binary);
  in.read((char *)v.data(), n * 4);
  return v;
}

int main(int argc, char **argv) {
  if (argc < 9) return 2;
  const size_t n = atoll(argv[2]), dim = atoll(argv[3]), nq = atoll(argv[5]), k = atoll(argv[6]), ef = atoll(argv[7]);
  const auto B = read_f32(argv[1], n * dim), Q = read_f32(argv[4], nq * dim);
  hnswlib::L2Space space(dim);
  uint32_t head[6] = {0, 0, 0, 0, 0, 0};
  try {
    hnswlib::HierarchicalNSW<float> hnsw(&space, n, 16, 100, "4");
    for (size_t i = 0; i < n; i++) hnsw.addPoint(B.data() + i * dim, i);
    hnsw.setRowFormat(HS_ROWS_U8);   // before the deferred build: applied once the index exists
    head[2] = (uint32_t)hnsw.rowFormat();
    hnswlib::HierarchicalNSWSlim<float> slim(&space, n, 16, 100);
    slim.convertFromHNSW(&hnsw);
    slim.setRowFormat(HS_ROWS_U8);
    slim.setEf(ef);
    hnsw.setEf(ef);
    std::vector<hnswlib::tableint> s_lab(nq * k);
    slim.searchKnnBatch(Q.data(), nq, k, s_lab.data());
    head[0] = (uint32_t)slim.rowFormat();
    head[1] = !strcmp(hs_last_kernel(slim.handle()), "hs::flat_kernel_u8");
    std::vector<uint64_t> h_lab(nq * k);
    std::vector<float> h_d(nq * k);
    std::vector<uint32_t> h_cnt(nq);
    hnsw.searchKnnBatch(Q.data(), nq, k, h_lab.data(), h_d.data(), h_cnt.data());
    head[3] = (uint32_t)hnsw.rowFormat();
    head[4] = !strcmp(hs_last_kernel(hnsw.handle()), "hs::flat_kernel_u8");
    try {
      hnswlib::HierarchicalNSWSlimQ<float> q(&space);
      q.setRowFormat(HS_ROWS_U8);
    } catch (std::runtime_error &) {
      head[5] = 1;
    }
    std::ofstream out(argv[8], std::ios::binary);
    out.write((char *)head, sizeof head);
    out.write((char *)s_lab.data(), 4 * nq * k);
    std::vector<uint32_t> h32(nq * k);
    for (size_t i = 0; i < nq * k; i++) h32[i] = (uint32_t)h_lab[i];
    out.write((char *)h32.data(), 4 * nq * k);
  } catch (std::exception &e) {
    fprintf(stderr, "facade_narrow: %s\n", e.what());
    return 1;
  }
  return 0;
}
