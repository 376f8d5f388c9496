// tests/facade_f32_free.cpp -- an fp32-free index through the hnswlib facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h): the caller of
// tests/facade_narrow.cpp that also drops the fp32 rows, so that every kernel reads the u8 copy.
// usage: facade_f32_free <base.f32> <n> <dim> <queries.f32> <nq> <k> <ef> <out.u32>
// out: 8 words {slim f32Resident() after the drop, slim kernel is hs::flat_kernel_u8, slim kernel with the exact order on is
//      hs::strict_kernel_u8, vanilla f32Resident() before its build (asked for: false), after it, vanilla kernel is
//      hs::flat_kernel_u8, setF32Resident(false) on an fp32-format index threw, HierarchicalNSWSlimQ::setF32Resident threw}, then
//      nq x k Slim labels (searchKnnBatch, nearest first), nq x k Slim labels in the reference's array order (exact order), then
//      nq x k vanilla labels (searchKnnBatch; ~0 where fewer than k were found).
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
  uint32_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  try {
    hnswlib::HierarchicalNSW<float> hnsw(&space, n, 16, 100, "4");
    for (size_t i = 0; i < n; i++) hnsw.addPoint(B.data() + i * dim, i);
    hnsw.setRowFormat(HS_ROWS_U8);   // before the deferred build: both applied once the index exists
    hnsw.setF32Resident(false);
    head[3] = hnsw.f32Resident() ? 1 : 0;
    hnswlib::HierarchicalNSWSlim<float> slim(&space, n, 16, 100);
    slim.convertFromHNSW(&hnsw);
    try {
      slim.setF32Resident(false);   // still in fp32 format: refused
    } catch (std::runtime_error &) {
      head[6] = 1;
      slim.setF32Resident(true);
    }
    slim.setRowFormat(HS_ROWS_U8);
    slim.setF32Resident(false);
    slim.setEf(ef);
    hnsw.setEf(ef);
    std::vector<hnswlib::tableint> s_lab(nq * k), s_exact(nq * k);
    slim.searchKnnBatch(Q.data(), nq, k, s_lab.data());
    head[0] = slim.f32Resident() ? 1 : 0;
    head[1] = !strcmp(hs_last_kernel(slim.handle()), "hs::flat_kernel_u8");
    hs_set_exact_order(slim.handle(), 1);
    slim.searchKnnBatch(Q.data(), nq, k, s_exact.data());
    head[2] = !strcmp(hs_last_kernel(slim.handle()), "hs::strict_kernel_u8");
    std::vector<uint64_t> h_lab(nq * k);
    std::vector<float> h_d(nq * k);
    std::vector<uint32_t> h_cnt(nq);
    hnsw.searchKnnBatch(Q.data(), nq, k, h_lab.data(), h_d.data(), h_cnt.data());
    head[4] = hnsw.f32Resident() ? 1 : 0;
    head[5] = !strcmp(hs_last_kernel(hnsw.handle()), "hs::flat_kernel_u8");
    try {
      hnswlib::HierarchicalNSWSlimQ<float> q(&space);
      q.setF32Resident(false);
    } catch (std::runtime_error &) {
      head[7] = 1;
    }
    std::ofstream out(argv[8], std::ios::binary);
    out.write((char *)head, sizeof head);
    out.write((char *)s_lab.data(), 4 * nq * k);
    out.write((char *)s_exact.data(), 4 * nq * k);
    std::vector<uint32_t> h32(nq * k);
    for (size_t i = 0; i < nq * k; i++) h32[i] = (uint32_t)h_lab[i];
    out.write((char *)h32.data(), 4 * nq * k);
  } catch (std::exception &e) {
    fprintf(stderr, "facade_f32_free: %s\n", e.what());
    return 1;
  }
  return 0;
}
