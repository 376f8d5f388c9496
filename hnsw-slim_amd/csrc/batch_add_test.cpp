// batch_add_test.cpp -- host-only test of the batched add into a loaded graph (batch_add_host, host_batch_build.hpp),
// built with AddressSanitizer and UBSan (Makefile target batch_add_test).  On integer rows (plenty of equal distances), both metrics:
//   * a build split at a batch boundary of its schedule -- the prefix built, saved, loaded with room, the generator seeded, the rest
//     added -- against the whole build, byte for byte, at several boundaries and with the changed level-0 lists collected;
//   * batch_max = 1 against resume() with one thread;
//   * an add that begins off a boundary at 1 and 4 workers against each other.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_batch_build.hpp"
#include "host_update.hpp"

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
  char tmpl[] = "/tmp/batch_add_test_XXXXXX";
  if (!mkdtemp(tmpl)) { printf("mkdtemp failed\n"); return 2; }
  const std::string dir = tmpl, w = dir + "/w.bin", p = dir + "/p.bin", a = dir + "/a.bin", b = dir + "/b.bin";
  size_t compared = 0;
  for (int metric = 0; metric < 2; metric++) {
    std::vector<BatchStep> steps;
    {
      VanillaGraph g;
      batch_build_host(g, base.data(), n, d, (Metric)metric, M, efC, "4", seed, 4, labels.data(), 0, 0, nullptr);
      g.save(w);
      steps = batch_schedule(draw_levels(n, g.mult, seed).data(), n, 0, 0);
    }
    // split equals whole: a one-row prefix, the first boundaries, then every ninth
    for (size_t bi = 1; bi < steps.size(); bi += bi < 4 ? 1 : 9) {
      const size_t n0 = steps[bi].begin;
      {
        VanillaGraph g;
        batch_build_host(g, base.data(), n0, d, (Metric)metric, M, efC, "4", seed, 4, labels.data(), 0, 0, nullptr);
        g.save(p);
      }
      VanillaGraph g;
      g.load(p, (Metric)metric, d, n);
      seed_levels(g, seed, n0);
      std::vector<uint32_t> touched;
      BatchBuildStats st;
      g.touched0 = &touched;
      batch_add_host(g, base.data() + n0 * d, labels.data() + n0, n - n0, 4, 0, 0, &st);
      g.touched0 = nullptr;
      g.save(a);
      CHECK(st.batches == steps.size() - bi && g.count == n, "split at %zu: %zu batches, count %zu", n0, st.batches, g.count);
      CHECK(slurp(a) == slurp(w), "metric %d: split at %zu differs from the whole build", metric, n0);
      bool in_range = !touched.empty();
      for (uint32_t t : touched) in_range = in_range && t < n;
      CHECK(in_range, "split at %zu: touched0 empty or out of range", n0);
      compared += slurp(a).size();
    }
    // batch_max = 1 equals resume(); an off-boundary add does not depend on the workers
    const size_t n0 = 333;
    {
      VanillaGraph g;
      g.build(base.data(), n0, d, (Metric)metric, M, efC, "4", seed, 1, labels.data());
      g.save(p);
    }
    {
      VanillaGraph g;
      g.load(p, (Metric)metric, d, n);
      seed_levels(g, seed, n0);
      resume(g, base.data() + n0 * d, labels.data() + n0, n - n0, 1);
      g.save(a);
    }
    {
      VanillaGraph g;
      BatchBuildStats st;
      g.load(p, (Metric)metric, d, n);
      seed_levels(g, seed, n0);
      batch_add_host(g, base.data() + n0 * d, labels.data() + n0, n - n0, 4, 0, 1, &st);
      g.save(b);
      CHECK(st.batches == n - n0, "batch_max 1: %zu batches", st.batches);
    }
    CHECK(slurp(a) == slurp(b), "metric %d: batch_max 1 differs from resume()", metric);
    compared += slurp(a).size();
    for (int threads : {1, 4}) {
      VanillaGraph g;
      BatchBuildStats st;
      g.load(p, (Metric)metric, d, n);
      seed_levels(g, seed, n0);
      batch_add_host(g, base.data() + n0 * d, labels.data() + n0, n - n0, threads, 0, 0, &st);
      g.save(threads == 1 ? a : b);
      CHECK(st.batches < n - n0 && g.count == n, "off boundary: %zu batches, count %zu", st.batches, g.count);
    }
    CHECK(slurp(a) == slurp(b), "metric %d: off-boundary add differs between 1 and 4 workers", metric);
    compared += slurp(a).size();
  }
  {   // batch_schedule_from started at the empty graph is batch_schedule; started at a boundary it is the rest of it
    const std::vector<int> lv = draw_levels(5000, branching_mult("4", M), seed);
    const std::vector<BatchStep> all = batch_schedule(lv.data(), lv.size(), 0, 0);
    const std::vector<BatchStep> from0 = batch_schedule_from(lv.data(), lv.size(), 0, (uint32_t)-1, -1, 0, 0);
    CHECK(from0.size() == all.size(), "batch_schedule_from(0): %zu batches of %zu", from0.size(), all.size());
    for (size_t bi = 1; bi < all.size(); bi += 7) {
      const size_t n0 = all[bi].begin;
      const std::vector<BatchStep> rest = batch_schedule_from(lv.data() + n0, lv.size() - n0, n0, all[bi].ep, all[bi].top, 0, 0);
      bool same = rest.size() == all.size() - bi;
      for (size_t k = 0; same && k < rest.size(); k++)
        same = rest[k].begin == all[bi + k].begin && rest[k].size == all[bi + k].size && rest[k].ep == all[bi + k].ep && rest[k].top == all[bi + k].top;
      CHECK(same, "batch_schedule_from(%zu) is not the rest of the schedule", n0);
    }
  }
  for (const std::string &f : {w, p, a, b}) remove(f.c_str());
  remove(dir.c_str());
  if (fails) return 1;
  printf("batch_add ok: %zu bytes compared\n", compared);
  return 0;
}
