// update_records_test.cpp -- host-only test of csrc/update_records.hpp, the record builder of the write path for changed nodes
// (capi_resident.cpp), under AddressSanitizer / UBSan: a small PackedIndex with lists of every length up to the tile stride, ids
// given unsorted and with repeats, at dim 10 (rows of 4-byte granularity, row_words rounded up), 20 and 32; every word of the
// staging buffer is checked against the layout index_update.hip reads.
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined update_records_test.cpp -o update_records_test
#include <cstdio>

#include "update_records.hpp"

using namespace hs;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (dim %zu)\n", __FILE__, __LINE__, #c, dim); return 1; } } while (0)

static int run(size_t dim, uint32_t stride) {
  const size_t n = 40;
  PackedIndex p;
  p.n = n; p.dim = dim;
  p.row_ptr0.assign(1, 0);
  std::vector<float> rows(n * dim);
  for (size_t i = 0; i < n; i++) {
    for (size_t j = 0; j < i % (stride + 1); j++) p.cols.push_back((uint32_t)((i * 7 + j) % n));   // lists of 0 .. stride ids
    p.row_ptr0.push_back((uint32_t)p.cols.size());
    p.labels.push_back(0x100000000ull * (i + 1) + 1000 + i);
    p.deleted.push_back(i % 3 == 0);
    for (size_t j = 0; j < dim; j++) rows[i * dim + j] = (float)(i * 100 + j);
  }
  size_t reads = 0;
  auto row_of = [&](uint32_t i) { reads++; return &rows[i * dim]; };
  const std::vector<uint32_t> changed = {31, 5, 17, 5, 39, 0, 17, 33}, with_row = {33, 12, 39, 12, 8};
  const std::vector<uint32_t> want = {0, 5, 17, 31, /* rows: */ 8, 12, 33, 39};
  const size_t first_row = 4, row_words = (dim + 3) / 4 * 4;
  for (int with_rows = 1; with_rows >= 0; with_rows--) {
    UpdateRecords r;
    reads = 0;
    CHECK(build_update_records(p, stride, n, changed, with_row, with_rows != 0, row_of, r));
    CHECK(r.nrec == want.size() && r.first_row == first_row && r.row_words == row_words && row_words % 4 == 0 && row_words >= dim);
    CHECK(r.stage.size() == want.size() * (4 + stride) + (with_rows ? (want.size() - first_row) * row_words : 0));
    CHECK(reads == (with_rows ? want.size() - first_row : 0));
    for (size_t k = 0; k < want.size(); k++) {
      const uint32_t id = want[k], *h = &r.stage[k * 4], *t = &r.stage[want.size() * 4 + k * stride];
      CHECK(h[0] == id && h[1] == p.deleted[id] && (((uint64_t)h[3] << 32) | h[2]) == p.labels[id]);
      const uint32_t deg = p.row_ptr0[id + 1] - p.row_ptr0[id];
      for (uint32_t j = 0; j < stride; j++) CHECK(t[j] == (j < deg ? p.cols[p.row_ptr0[id] + j] : 0xFFFFFFFFu));
      if (!with_rows || k < first_row) continue;
      const uint32_t *x = &r.stage[want.size() * (4 + stride) + (k - first_row) * row_words];
      CHECK(memcmp(x, &rows[id * dim], 4 * dim) == 0);
      for (size_t j = dim; j < row_words; j++) CHECK(x[j] == 0);
    }
  }
  // an id at or beyond the limit is refused, in either list, and the output is left alone
  UpdateRecords keep;
  keep.stage.assign(3, 7u); keep.nrec = 9;
  CHECK(!build_update_records(p, stride, n, {1, (uint32_t)n}, {2}, true, row_of, keep));
  CHECK(!build_update_records(p, stride, n, {1}, {2, 0xFFFFFFFFu}, true, row_of, keep));
  CHECK(!build_update_records(p, stride, 17, {1, 17}, {}, true, row_of, keep));
  CHECK(keep.nrec == 9 && keep.stage == std::vector<uint32_t>(3, 7u));
  // an empty change set builds an empty buffer
  UpdateRecords none;
  CHECK(build_update_records(p, stride, n, {}, {}, true, row_of, none));
  CHECK(none.stage.empty() && none.nrec == 0 && none.first_row == 0);
  // only rows / only lists
  UpdateRecords only;
  CHECK(build_update_records(p, stride, n, {}, {9, 3, 9}, true, row_of, only) && only.nrec == 2 && only.first_row == 0 && only.stage[0] == 3 && only.stage[4] == 9);
  CHECK(build_update_records(p, stride, n, {9, 3, 9}, {}, true, row_of, only) && only.nrec == 2 && only.first_row == 2 && only.stage.size() == 2 * (4 + (size_t)stride));
  return 0;
}

// PackedIndex::repeats_id0 (the pack-time scan behind the launch plan's has_dup0): a repeat in neighbouring positions, at both ends of a
// 64-id list, a self-loop and an id shared by two lists (neither is a repeat), an empty index.
static int run_repeats() {
  const size_t dim = 0;
  auto make = [](const std::vector<std::vector<uint32_t>> &lists) {
    PackedIndex p;
    p.n = lists.size();
    p.row_ptr0.assign(1, 0);
    for (const auto &l : lists) {
      p.cols.insert(p.cols.end(), l.begin(), l.end());
      p.row_ptr0.push_back((uint32_t)p.cols.size());
    }
    return p;
  };
  std::vector<uint32_t> wide(64);
  for (uint32_t j = 0; j < 64; j++) wide[j] = j + 1;
  std::vector<std::vector<uint32_t>> g(70);
  g[0] = wide;
  CHECK(!make(g).repeats_id0());
  g[0][63] = g[0][0];
  CHECK(make(g).repeats_id0());
  g[0] = wide;
  g[5] = {5, 6};          // a self-loop
  g[6] = {5, 7}; g[7] = {5, 6};   // ids shared between lists
  CHECK(!make(g).repeats_id0());
  g[69] = {3, 3};
  CHECK(make(g).repeats_id0());
  g[69] = {3, 4, 3};
  CHECK(make(g).repeats_id0());
  g[69] = {69, 69};
  CHECK(make(g).repeats_id0());
  CHECK(!make({}).repeats_id0() && !make({{}}).repeats_id0() && make({{0, 0}}).repeats_id0());
  printf("repeats_id0 ok\n");
  return 0;
}

int main() {
  if (run_repeats()) return 1;
  size_t checked = 0;
  for (size_t dim : {10, 20, 32})
    for (uint32_t stride : {16u, 32u, 64u}) {
      if (run(dim, stride)) return 1;
      checked++;
    }
  printf("update_records ok: %zu shapes\n", checked);
  return 0;
}
