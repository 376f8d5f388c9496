// resume_test.cpp -- host-only test of resume() (host_update.hpp), built with AddressSanitizer and UBSan (Makefile
// target resume_test): a graph built in one go against the same graph built as a prefix, saved, loaded with room, its level
// generator put where the prefix build left it, and resumed -- from 1, 10 and n / 2 points, with delete marks set before the
// resume, and the refused over-capacity resume.  The saved files must be equal byte for byte.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_update.hpp"

using namespace hs;

static std::vector<char> slurp(const std::string &p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

int main() {
  const size_t n = 400, d = 12, M = 6, efC = 40, seed = 100;
  std::vector<float> base(n * d);
  uint32_t s = 12345;
  for (float &x : base) { s = s * 1664525u + 1013904223u; x = (float)((s >> 8) % 64); }   // integer rows: plenty of equal distances
  std::vector<uint64_t> labels(n);
  for (size_t i = 0; i < n; i++) labels[i] = 1000 + 3 * i;
  char tmpl[] = "/tmp/resume_test_XXXXXX";
  if (!mkdtemp(tmpl)) { printf("mkdtemp failed\n"); return 2; }
  const std::string dir = tmpl, whole = dir + "/whole.bin", part = dir + "/part.bin", out = dir + "/out.bin";
  size_t compared = 0;
  for (int metric = 0; metric < 2; metric++) {
    {
      VanillaGraph g;
      g.build(base.data(), n, d, (Metric)metric, M, efC, "4", seed, 1, labels.data());
      g.save(whole);
    }
    const std::vector<char> want = slurp(whole);
    for (size_t n0 : {(size_t)1, (size_t)10, n / 2}) {
      {
        VanillaGraph g;
        g.build(base.data(), n0, d, (Metric)metric, M, efC, "4", seed, 1, labels.data());
        g.save(part);
      }
      VanillaGraph g;
      g.load(part, (Metric)metric, d, n);
      CHECK(g.count == n0 && g.max_elements == n, "load with room: count %zu max %zu", g.count, g.max_elements);
      seed_levels(g, seed, n0);
      std::vector<uint32_t> touched;
      g.touched0 = &touched;
      // in two calls: the generator carries over
      const size_t mid = n0 + (n - n0) / 3;
      resume(g, base.data() + n0 * d, labels.data() + n0, mid - n0, 1);
      resume(g, base.data() + mid * d, labels.data() + mid, n - mid, 1);
      g.touched0 = nullptr;
      g.save(out);
      const std::vector<char> got = slurp(out);
      CHECK(got == want, "metric %d n0 %zu: resumed file differs from the one-shot build (%zu vs %zu bytes)", metric, n0, got.size(), want.size());
      for (uint32_t t : touched) CHECK(t < n, "touched id %u out of range", t);
      CHECK(!touched.empty(), "no level-0 list recorded as touched");
      compared += got.size();
      bool threw = false;
      try { resume(g, base.data(), labels.data(), 1, 1); } catch (std::runtime_error &e) { threw = std::string(e.what()) == "The number of elements exceeds the specified limit"; }
      CHECK(threw, "a resume beyond max_elements must be refused");
    }
    // marks set before the resume: the resumed graph equals the graph that took the same marks at the same point of a single run
    {
      const size_t n0 = n / 2;
      VanillaGraph a;
      a.init(n, d, (Metric)metric, M, efC, "4");
      seed_levels(a, seed, 0);
      resume(a, base.data(), labels.data(), n0, 1);
      a.save(part);
      for (uint32_t i = 0; i < n0; i += 3) a.set_deleted(i, true);
      a.set_deleted(a.enterpoint, true);
      resume(a, base.data() + n0 * d, labels.data() + n0, n - n0, 1);
      a.save(whole);
      VanillaGraph b;
      b.load(part, (Metric)metric, d, n);
      for (uint32_t i = 0; i < n0; i += 3) b.set_deleted(i, true);
      b.set_deleted(b.enterpoint, true);
      seed_levels(b, seed, n0);
      resume(b, base.data() + n0 * d, labels.data() + n0, n - n0, 1);
      b.save(out);
      CHECK(slurp(out) == slurp(whole), "metric %d: resume over delete marks differs", metric);
      CHECK(b.num_deleted() == a.num_deleted() && b.num_deleted() > 0, "marks lost");
      compared += slurp(out).size();
    }
  }
  remove(whole.c_str()); remove(part.c_str()); remove(out.c_str()); remove(dir.c_str());
  if (fails) return 1;
  printf("resume ok: %zu bytes compared\n", compared);
  return 0;
}
