// rq_batch_build_test.cpp -- host-only test of the batched build of HNSW-SlimQ's base graph (host_rq_batch_build.hpp), built with
// AddressSanitizer and UBSan (Makefile target rq_batch_build_test): batch_max = 1 against RqGraph::rq_build with one thread, the
// default schedule and a small batch_max at 1 and 4 threads against each other, byte for byte, on integer rows (plenty of equal
// distances, which this builder decides by id), both metrics, at a dimension with whole packets and a tail and at one below a packet.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_rq_batch_build.hpp"

using namespace hs;

static std::vector<char> slurp(const std::string &p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
  const size_t n = 700, M = 6, efC = 40, seed = 100;
  char tmpl[] = "/tmp/rq_batch_build_test_XXXXXX";
  if (!mkdtemp(tmpl)) { printf("mkdtemp failed\n"); return 2; }
  const std::string dir = tmpl, a = dir + "/a.bin", b = dir + "/b.bin";
  size_t compared = 0;
  for (size_t d : {(size_t)12, (size_t)37}) {
    std::vector<float> base(n * d);
    uint32_t s = 12345;
    for (float &x : base) { s = s * 1664525u + 1013904223u; x = (float)((s >> 8) % 64) - 20.f; }
    for (int metric = 0; metric < 2; metric++) {
      {
        RqGraph g;
        g.rq_build(base.data(), n, d, (Metric)metric, M, efC, seed, 1);
        g.save(a);
      }
      {
        RqGraph g;
        BatchBuildStats st;
        rq_batch_build_host(g, base.data(), n, d, (Metric)metric, M, efC, seed, 4, 0, 1, &st);
        g.save(b);
        CHECK(st.batches == n, "batch_max 1: %zu batches", st.batches);
      }
      CHECK(slurp(a) == slurp(b), "d %zu metric %d: batch_max 1 differs from the serial build", d, metric);
      compared += slurp(a).size();
      for (size_t batch_max : {(size_t)0, (size_t)7}) {
        for (int threads : {1, 4}) {
          RqGraph g;
          BatchBuildStats st;
          rq_batch_build_host(g, base.data(), n, d, (Metric)metric, M, efC, seed, threads, 0, batch_max, &st);
          g.save(threads == 1 ? a : b);
          CHECK(st.batches < n && g.count == n, "batch_max %zu: %zu batches, count %zu", batch_max, st.batches, g.count);
        }
        CHECK(slurp(a) == slurp(b), "d %zu metric %d batch_max %zu: 1 and 4 threads differ", d, metric, batch_max);
        compared += slurp(a).size();
      }
    }
  }
  remove(a.c_str()); remove(b.c_str()); remove(dir.c_str());
  if (fails) return 1;
  printf("rq_batch_build ok: %zu bytes compared\n", compared);
  return 0;
}
