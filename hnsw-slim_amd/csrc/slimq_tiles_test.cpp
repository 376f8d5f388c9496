// slimq_tiles_test.cpp -- host-only test of the layout functions of slimq_tiles.hpp (built with AddressSanitizer / UBSan): hand-made
// graphs at the sizes where the tile assembly takes another path, every word of the three arrays checked against its definition.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "slimq_tiles.hpp"

using namespace hs;

#define CHECK(c)                                                           \
  do {                                                                     \
    if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } \
  } while (0)

typedef std::vector<std::vector<std::vector<uint32_t>>> Lists;   // lists[i][l]; an empty lists[i]: a node without a blob

struct Csr {
  std::vector<uint32_t> row_ptr0, cols, up_base, up_ptr;
  std::vector<int32_t> level;
  size_t max_deg0 = 0;
};
// PackedIndex::pack_chal's order: level-0 lists first, then the upper lists node by node with one trailing entry each
static Csr pack(const Lists &g, const std::vector<int32_t> &level) {
  Csr c;
  const size_t n = g.size();
  c.level = level;
  c.row_ptr0.assign(n + 1, 0);
  c.up_base.assign(n, kSlimqEmpty);
  for (size_t i = 0; i < n; i++) {
    if (!g[i].empty()) {
      c.cols.insert(c.cols.end(), g[i][0].begin(), g[i][0].end());
      c.max_deg0 = std::max(c.max_deg0, g[i][0].size());
    }
    c.row_ptr0[i + 1] = (uint32_t)c.cols.size();
  }
  for (size_t i = 0; i < n; i++) {
    if (g[i].size() < 2) continue;
    c.up_base[i] = (uint32_t)c.up_ptr.size();
    for (size_t l = 1; l < g[i].size(); l++) {
      c.up_ptr.push_back((uint32_t)c.cols.size());
      c.cols.insert(c.cols.end(), g[i][l].begin(), g[i][l].end());
    }
    c.up_ptr.push_back((uint32_t)c.cols.size());
  }
  return c;
}

static void run(const char *name, const Lists &g, std::vector<int32_t> level, size_t dim, uint32_t want_stride, uint32_t want_up) {
  const size_t n = g.size(), padded = (dim + 63) / 64 * 64, nblk = padded / 64;
  if (level.empty())
    for (const auto &l : g) level.push_back(l.empty() ? 0 : (int32_t)l.size() - 1);
  std::mt19937_64 gen(n * 131 + dim);
  std::vector<float> factors(n * 3);
  std::vector<uint32_t> cluster(n);
  std::vector<uint64_t> code(n * nblk);
  for (auto &f : factors) f = (float)(gen() % 2001) / 100.f - 10.f;
  for (auto &c : cluster) c = (uint32_t)(gen() % 7);
  for (auto &c : code) c = gen();
  const uint32_t rw = slimq_rec_words(padded);
  CHECK(rw % 4 == 0 && rw >= 4 + 2 * nblk && rw < 4 + 2 * nblk + 4);
  const std::vector<uint32_t> rec = slimq_pack_records(factors.data(), cluster.data(), code.data(), n, padded);
  CHECK(rec.size() == n * rw);
  for (size_t i = 0; i < n; i++) {
    const uint32_t *r = &rec[i * rw];
    float f[3];
    memcpy(&f[0], r, 4); memcpy(&f[1], r + 1, 4); memcpy(&f[2], r + 3, 4);
    CHECK(f[0] == factors[i * 3] && f[1] == factors[i * 3 + 1] && f[2] == factors[i * 3 + 2] && r[2] == cluster[i]);
    for (size_t b = 0; b < nblk; b++) CHECK(r[4 + 2 * b] == (uint32_t)code[i * nblk + b] && r[5 + 2 * b] == (uint32_t)(code[i * nblk + b] >> 32));
    for (uint32_t w = 4 + 2 * (uint32_t)nblk; w < rw; w++) CHECK(r[w] == 0);
  }
  const Csr c = pack(g, level);
  const uint32_t stride = c.max_deg0 <= 64 ? std::max<uint32_t>(16, (uint32_t)((c.max_deg0 + 15) / 16 * 16)) : 0;
  CHECK(stride == want_stride);
  const std::vector<uint32_t> ft = slimq_ftile_host(rec, rw, n, c.row_ptr0.data(), c.cols.data(), stride);
  CHECK(ft.size() == n * stride * rw);
  for (size_t i = 0; i < n && stride; i++)
    for (uint32_t j = 0; j < stride; j++) {
      const uint32_t *r = &ft[(i * stride + j) * rw];
      const bool live = !g[i].empty() && j < g[i][0].size();
      const uint32_t nb = live ? g[i][0][j] : kSlimqEmpty;
      CHECK(r[3] == nb);
      for (uint32_t w = 0; w < rw; w++)
        if (w != 3) CHECK(r[w] == (live ? rec[(size_t)nb * rw + w] : 0u));
    }
  const uint32_t up = slimq_up_stride(c.up_ptr);
  CHECK(up == want_up);
  const std::vector<uint32_t> ut = slimq_uptile_host(rec, rw, n, c.level.data(), c.up_base, c.up_ptr, c.cols.data(), up);
  const uint32_t urw = rw + 4;
  CHECK(ut.size() == (up ? c.up_ptr.size() * up * urw : 0));
  if (up) {
    std::vector<const std::vector<uint32_t> *> owner(c.up_ptr.size(), nullptr);
    for (size_t i = 0; i < n; i++)
      for (size_t l = 1; l < g[i].size(); l++) owner[c.up_base[i] + l - 1] = &g[i][l];
    for (size_t t = 0; t < c.up_ptr.size(); t++)
      for (uint32_t j = 0; j < up; j++) {
        const uint32_t *r = &ut[(t * up + j) * urw];
        const bool live = owner[t] && j < owner[t]->size();
        const uint32_t nb = live ? (*owner[t])[j] : kSlimqEmpty;
        CHECK(r[3] == nb);
        for (uint32_t w = 0; w < rw; w++)
          if (w != 3) CHECK(r[w] == (live ? rec[(size_t)nb * rw + w] : 0u));
        CHECK(r[rw] == (live ? c.up_base[nb] : 0u) && r[rw + 1] == 0 && r[rw + 2] == 0 && r[rw + 3] == 0);
      }
  }
  printf("  %-14s n = %zu dim = %zu rw = %u stride = %u up_stride = %u\n", name, n, dim, rw, stride, up);
}

static Lists ring(uint32_t n, uint32_t deg) {
  Lists g(n);
  for (uint32_t i = 0; i < n; i++) {
    g[i].resize(1);
    for (uint32_t j = 0; j < deg; j++) g[i][0].push_back((i + 1 + j) % n);
  }
  return g;
}
static std::vector<uint32_t> iota(uint32_t a, uint32_t b) {
  std::vector<uint32_t> v;
  for (uint32_t i = a; i < b; i++) v.push_back(i);
  return v;
}

int main() {
  run("single", Lists(1), {0}, 64, 16, 0);
  run("empty_level2", Lists{{{1, 2}, {1, 2}, {1}}, {}, {{0, 1}, {1, 0}, {1}}, {{0, 1, 2}}}, {2, 2, 2, 0}, 64, 16, 16);
  run("deg16", ring(20, 16), {}, 128, 16, 0);
  run("deg17", ring(20, 17), {}, 128, 32, 0);
  {
    Lists g(65, {{0}});
    g[0] = {iota(1, 65)};
    run("hub64", g, {}, 64, 64, 0);
  }
  {
    Lists g(66, {{0}});
    g[0] = {iota(1, 66)};
    run("hub65", g, {}, 64, 0, 0);
  }
  {
    Lists g(66, {{0}, {0}});
    g[0] = {{1}, iota(1, 66)};
    run("upper65", g, {}, 64, 16, 0);
  }
  {
    Lists g(21, {{0}, {0}});
    g[0] = {{1, 2}, iota(1, 18), {1}};
    g[1] = {{0}, {0}, {0}};
    for (int i = 18; i < 21; i++) g[i] = {{0, 1}};
    run("upper17_d192", g, {}, 192, 16, 32);
  }
  printf("slimq_tiles ok\n");
  return 0;
}
