// batch_build_test.cpp -- host-only test of the batched build (host_batch_build.hpp), built with AddressSanitizer and UBSan
// (Makefile target batch_build_test): batch_max = 1 against VanillaGraph::build with one thread, the default schedule and a small
// batch_max at 1 and 4 threads against each other, byte for byte, on integer rows (plenty of equal distances), both metrics;
// and the schedule's sums and cuts.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_batch_build.hpp"

using namespace hs;

static std::vector<char> slurp(const std::string &p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
  const size_t n = 700, d = 12, M = 6, efC = 40, seed = 100;
  std::vector<float> base(n * d);
  uint32_t s = 12345;
  for (float &x : base) { s = s * 1664525u + 1013904223u; x = (float)((s >> 8) % 64); }
  std::vector<uint64_t> labels(n);
  for (size_t i = 0; i < n; i++) labels[i] = 1000 + 3 * i;
  char tmpl[] = "/tmp/batch_build_test_XXXXXX";
  if (!mkdtemp(tmpl)) { printf("mkdtemp failed\n"); return 2; }
  const std::string dir = tmpl, a = dir + "/a.bin", b = dir + "/b.bin";
  size_t compared = 0;
  for (int metric = 0; metric < 2; metric++) {
    {
      VanillaGraph g;
      g.build(base.data(), n, d, (Metric)metric, M, efC, "4", seed, 1, labels.data());
      g.save(a);
    }
    {
      VanillaGraph g;
      BatchBuildStats st;
      batch_build_host(g, base.data(), n, d, (Metric)metric, M, efC, "4", seed, 4, labels.data(), 0, 1, &st);
      g.save(b);
      CHECK(st.batches == n, "batch_max 1: %zu batches", st.batches);
    }
    CHECK(slurp(a) == slurp(b), "metric %d: batch_max 1 differs from the serial build", metric);
    compared += slurp(a).size();
    for (size_t batch_max : {(size_t)0, (size_t)7}) {
      for (int threads : {1, 4}) {
        VanillaGraph g;
        BatchBuildStats st;
        batch_build_host(g, base.data(), n, d, (Metric)metric, M, efC, "4", seed, threads, labels.data(), 0, batch_max, &st);
        g.save(threads == 1 ? a : b);
        CHECK(st.batches < n && g.count == n, "batch_max %zu: %zu batches, count %zu", batch_max, st.batches, g.count);
      }
      CHECK(slurp(a) == slurp(b), "metric %d batch_max %zu: 1 and 4 threads differ", metric, batch_max);
      compared += slurp(a).size();
    }
  }
  {
    const std::vector<int> lv = draw_levels(5000, branching_mult("4", M), seed);
    for (size_t div : {(size_t)0, (size_t)1, (size_t)4})
      for (size_t cap : {(size_t)0, (size_t)1, (size_t)50}) {
        const std::vector<BatchStep> steps = batch_schedule(lv.data(), lv.size(), div, cap);
        size_t done = 0;
        int top = -1;
        uint32_t ep = (uint32_t)-1;
        for (const BatchStep &st : steps) {
          CHECK(st.begin == done && st.size >= 1 && st.ep == ep && st.top == top, "schedule (%zu, %zu): batch at %u", div, cap, st.begin);
          for (uint32_t k = 0; k < st.size; k++)
            if (lv[st.begin + k] > top) {
              CHECK(k + 1 == st.size, "schedule (%zu, %zu): row %u raises the level inside its batch", div, cap, st.begin + k);
              top = lv[st.begin + k];
              ep = st.begin + k;
            }
          done += st.size;
        }
        CHECK(done == lv.size(), "schedule (%zu, %zu): %zu rows", div, cap, done);
      }
  }
  remove(a.c_str()); remove(b.c_str()); remove(dir.c_str());
  if (fails) return 1;
  printf("batch_build ok: %zu bytes compared\n", compared);
  return 0;
}
