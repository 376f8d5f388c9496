// load_guard_test.cpp -- host-only run of everything the host does with a graph file before an upload, built with AddressSanitizer
// and UBSan (Makefile target load_guard_test): load (which runs index_check.hpp) -> pack (packed_index.hpp) -> upper-level tiles ->
// level-0 tiles -> the enter point's up_base (host_tiles.hpp).  tests/test_load_guard_cpu.py hands it a manifest of the files of
// tests/hostile_graphs.py, one "kind dim accept|refuse path" per line: a file to refuse must be refused by the loader with the
// reference's text -- before any code has indexed with one of its ids, or a sanitizer report ends the run -- and a file to accept
// must run the whole chain clean.
//   load_guard_test <manifest>
//   load_guard_test --time     parse + pack of a synthetic 200 000-node M = 16 vanilla image, and the check's share of it
//                              (meant for a build without sanitizers: make load_guard_time)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "host_tiles.hpp"
#include "rabitq_host.hpp"

using namespace hs;

static size_t chain(const PackedIndex &p) {
  uint32_t up_stride = 0;
  const std::vector<uint32_t> ut = build_uptile(p, up_stride);
  const uint32_t stride = tile_stride_for(p.max_deg0);
  const std::vector<uint32_t> t0 = stride ? build_tile0(p, stride) : std::vector<uint32_t>();
  return ut.size() + t0.size() + (ep_base_of(p) != PackedIndex::NONE) + (p.repeats_id0() ? 1 : 0);
}

// the whole chain on one file; throws what the loader throws
static size_t run(const std::string &kind, size_t dim, const BinSource &src) {
  PackedIndex p;
  if (kind == "hnsw") {
    VanillaGraph g;
    g.load(src, METRIC_L2, dim);
    p.from_vanilla(g);
  } else if (kind == "slim") {
    SlimGraph g;
    g.load(src, METRIC_L2, dim);
    p.from_slim(g);
  } else {
    SlimQGraph q;
    q.load(src, METRIC_L2, dim);
    p.kind = 2; p.n = q.count; p.dim = q.dim; p.maxlevel = q.maxlevel; p.threshold_level = q.threshold_level; p.enterpoint = q.enterpoint;
    p.pack_chal([&](size_t i) { return (int)q.level[i]; }, [&](size_t i) { return (size_t)q.total(i); },
                [&](size_t i) -> const std::vector<char> & { return q.blobs[i]; });
  }
  return chain(p);
}

static int time_it() {
  const size_t n = 200000, d = 16, M = 16;
  VanillaGraph g;
  g.init(n, d, METRIC_L2, M, 100, "4");
  std::default_random_engine gen(100);
  std::vector<int> lv(n);
  int top = 0;
  uint32_t ep = 0;
  for (size_t i = 0; i < n; i++) {
    lv[i] = level_from(gen, g.mult);
    if (lv[i] > top) { top = lv[i]; ep = (uint32_t)i; }
  }
  std::vector<std::vector<uint32_t>> at_least(top + 1);
  for (size_t i = 0; i < n; i++)
    for (int l = 0; l <= lv[i]; l++) at_least[l].push_back((uint32_t)i);
  uint32_t s = 12345;
  auto rnd = [&](size_t m) { s = s * 1664525u + 1013904223u; return (size_t)(s >> 4) % m; };
  for (size_t i = 0; i < n; i++) {
    g.levels[i] = lv[i];
    if (lv[i]) g.links[i].assign(g.size_links_up * lv[i] + 1, 0);
    for (int l = 0; l <= lv[i]; l++) {
      uint32_t *ll = g.list_at((uint32_t)i, l);
      const size_t c = std::min<size_t>(l ? g.maxM : g.maxM0, at_least[l].size());
      VanillaGraph::set_cnt(ll, (uint16_t)c);
      for (size_t j = 0; j < c; j++) ll[1 + j] = at_least[l][rnd(at_least[l].size())];
    }
  }
  g.count = n; g.maxlevel = top; g.enterpoint = ep;
  char tmpl[] = "/tmp/load_guard_XXXXXX";
  if (!mkdtemp(tmpl)) { printf("mkdtemp failed\n"); return 2; }
  const std::string path = std::string(tmpl) + "/synthetic.bin";
  g.save(path);
  std::ifstream f(path, std::ios::binary);
  const std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  double best_all = 1e30, best_check = 1e30;
  size_t sink = 0;
  for (int rep = 0; rep < 5; rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    VanillaGraph h;
    h.load(BinSource(bytes.data(), bytes.size()), METRIC_L2, d);
    PackedIndex p;
    p.from_vanilla(h);
    const auto t1 = std::chrono::steady_clock::now();
#ifndef HS_LOAD_GUARD_PARENT
    sink += h.check() != nullptr;
#endif
    const auto t2 = std::chrono::steady_clock::now();
    sink += p.cols.size();
    best_all = std::min(best_all, std::chrono::duration<double, std::milli>(t1 - t0).count());
    best_check = std::min(best_check, std::chrono::duration<double, std::milli>(t2 - t1).count());
  }
  remove(path.c_str());
  remove(tmpl);
  printf("synthetic vanilla image: %zu nodes, M %zu, %zu bytes, maxlevel %d (%zu)\n", n, M, bytes.size(), top, sink);
  printf("parse + pack: %.1f ms (best of 5); the check alone: %.1f ms\n", best_all, best_check);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && std::string(argv[1]) == "--time") return time_it();
  if (argc != 2) { printf("usage: load_guard_test <manifest> | --time\n"); return 2; }
  std::ifstream man(argv[1]);
  std::string line;
  int fails = 0;
  size_t files = 0, refused = 0;
  while (std::getline(man, line)) {
    std::istringstream is(line);
    std::string kind, expect, path;
    size_t dim = 0;
    if (!(is >> kind >> dim >> expect >> path)) continue;
    files++;
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    for (int from_mem = 0; from_mem < 2; from_mem++) {   // the file, and the same bytes in memory (an exactly sized heap block)
      std::string what;
      try {
        run(kind, dim, from_mem ? BinSource(bytes.data(), bytes.size()) : BinSource(path));
      } catch (std::exception &e) {
        what = e.what();
      }
      const bool ok = expect == "refuse" ? what == kCorruptText : what.empty();
      if (!ok) { fails++; printf("FAIL %s (%s, expected to %s): '%s'\n", path.c_str(), kind.c_str(), expect.c_str(), what.c_str()); }
    }
    refused += expect == "refuse";
  }
  printf("%zu files, %zu of them refused, %d failures\n", files, refused, fails);
  return fails ? 1 : 0;
}
