// upsert_test.cpp -- host-only test of VanillaGraph's update path (host_update.hpp: updatePoint, repairConnectionsForUpdate,
// addPoint with replace_deleted, mark / unmark with deleted_elements, resizeIndex), built with AddressSanitizer and UBSan (Makefile
// target upsert_test) and run as its own binary.  It replays an operation list as hs_hnsw_replay does -- loadIndex, the operations,
// saveIndex -- and compares the saved file with the expected one byte for byte; then once more from a fresh load, and the two runs
// must agree.  Every id handed to the touched0 hook must be a node of the index, and after every operation each node whose level-0
// list (count, ids[:count]) differs from what it was before the operation must be among the ids the hook received during it or be
// the id the operation returned: the device copy of a resident index rewrites exactly those tiles.
// usage: upsert_test <index.bin> <metric 0|1> <dim> <max_elements> <allow_replace_deleted 0|1> <ops.u64> <rows.f32> <expected.bin>
//   ops.u64: n x {kind, label or new capacity, replace flag, row index}; kinds add = 0, mark = 1, unmark = 2, resize = 3
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "host_update.hpp"

using namespace hs;

template <typename T>
static std::vector<T> slurp(const std::string &p) {
  std::ifstream f(p, std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> out(raw.size() / sizeof(T));
  memcpy(out.data(), raw.data(), out.size() * sizeof(T));
  return out;
}

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// level-0 list of every node as (count, ids[:count])
static std::vector<std::vector<uint32_t>> lists0(const VanillaGraph &g) {
  std::vector<std::vector<uint32_t>> out(g.count);
  for (size_t i = 0; i < g.count; i++) {
    const uint32_t *l = g.list_at((uint32_t)i, 0);
    out[i].assign(l + 1, l + 1 + VanillaGraph::cnt_of(l));
  }
  return out;
}

static std::vector<char> replay(const char *index, int metric, size_t dim, size_t max_elements, bool allow, const std::vector<uint64_t> &ops,
                                const std::vector<float> &rows, const std::string &out, size_t *n_touched) {
  VanillaGraph g;
  g.load(index, (Metric)metric, dim, max_elements);
  set_allow_replace(g, allow);
  std::unordered_map<uint64_t, uint32_t> lookup;
  for (size_t i = 0; i < g.count; i++) lookup[g.label((uint32_t)i)] = (uint32_t)i;
  std::vector<uint32_t> touched;
  g.touched0 = &touched;
  VanillaGraph::Visited vl;
  std::vector<std::vector<uint32_t>> before = lists0(g);
  for (size_t o = 0; o + 3 < ops.size(); o += 4) {
    const uint64_t kind = ops[o], arg = ops[o + 1], flag = ops[o + 2], row = ops[o + 3];
    const size_t touched_before = touched.size();
    std::set<uint32_t> may_change;
    if (kind == 0) {
      CHECK((row + 1) * dim <= rows.size(), "operation %zu names row %llu beyond the rows", o / 4, (unsigned long long)row);
      const uint32_t id = upsert(g, rows.data() + row * dim, arg, flag != 0, lookup, vl);
      CHECK(id < g.count && g.label(id) == arg && lookup.at(arg) == id && !g.deleted(id), "operation %zu: label %llu not at id %u", o / 4, (unsigned long long)arg, id);
      CHECK(!memcmp(g.vec(id), rows.data() + row * dim, 4 * dim), "operation %zu: row not stored", o / 4);
      may_change.insert(id);
    } else if (kind == 1) {
      mark(g, lookup.at(arg));
    } else if (kind == 2) {
      unmark(g, lookup.at(arg));
    } else {
      resize(g, arg);
    }
    may_change.insert(touched.begin() + touched_before, touched.end());
    std::vector<std::vector<uint32_t>> after = lists0(g);
    for (size_t i = 0; i < after.size(); i++)
      if ((i >= before.size() ? !after[i].empty() : after[i] != before[i]) && !may_change.count((uint32_t)i)) {
        CHECK(false, "operation %zu (kind %llu) changed the level-0 list of node %zu, which is neither touched nor returned", o / 4,
              (unsigned long long)kind, i);
        break;
      }
    before.swap(after);
  }
  g.touched0 = nullptr;
  for (uint32_t t : touched) CHECK(t < g.count, "touched id %u out of range", t);
  *n_touched = touched.size();
  size_t marked = 0;
  for (uint32_t id : g.deleted_elements) { CHECK(id < g.count && g.deleted(id), "deleted_elements holds the unmarked id %u", id); marked++; }
  CHECK(!allow || marked == g.num_deleted(), "deleted_elements holds %zu ids, the index %zu marks", marked, g.num_deleted());
  g.save(out);
  return slurp<char>(out);
}

int main(int argc, char **argv) {
  if (argc < 9) { printf("usage: see the head of upsert_test.cpp\n"); return 2; }
  const int metric = atoi(argv[2]);
  const size_t dim = atoll(argv[3]), max_elements = atoll(argv[4]);
  const bool allow = atoi(argv[5]) != 0;
  const std::vector<uint64_t> ops = slurp<uint64_t>(argv[6]);
  const std::vector<float> rows = slurp<float>(argv[7]);
  const std::vector<char> want = slurp<char>(argv[8]);
  char tmpl[] = "/tmp/upsert_test_XXXXXX";
  if (!mkdtemp(tmpl)) { printf("mkdtemp failed\n"); return 2; }
  const std::string dir = tmpl, out = dir + "/out.bin";
  size_t t1 = 0, t2 = 0;
  const std::vector<char> a = replay(argv[1], metric, dim, max_elements, allow, ops, rows, out, &t1);
  const std::vector<char> b = replay(argv[1], metric, dim, max_elements, allow, ops, rows, out, &t2);
  CHECK(a == want, "replayed file differs from the expected one (%zu vs %zu bytes)", a.size(), want.size());
  CHECK(a == b && t1 == t2, "two replays of the same list differ");
  CHECK(t1 > 0, "no level-0 list recorded as touched");
  // the refusals of the update path, on a fresh load
  {
    VanillaGraph g;
    g.load(argv[1], (Metric)metric, dim, 0);
    std::unordered_map<uint64_t, uint32_t> lookup;
    for (size_t i = 0; i < g.count; i++) lookup[g.label((uint32_t)i)] = (uint32_t)i;
    VanillaGraph::Visited vl;
    auto text = [&](auto fn) -> std::string { try { fn(); } catch (std::runtime_error &e) { return e.what(); } return "(no exception)"; };
    uint32_t u = 0;   // an element the loaded graph does not mark
    while (u < g.count && g.deleted(u)) u++;
    CHECK(u < g.count, "every element of the loaded graph is marked");
    const size_t marks0 = g.num_deleted(), count0 = g.count;
    const uint64_t first = g.label(u);
    CHECK(g.deleted_elements.empty(), "deleted_elements filled although replacement is off");
    CHECK(text([&]() { upsert(g, rows.data(), first, true, lookup, vl); }) == "Replacement of deleted elements is disabled in constructor", "flag without allow");
    CHECK(text([&]() { upsert(g, rows.data(), ~0ull, false, lookup, vl); }) == "The number of elements exceeds the specified limit", "append to a full index");
    CHECK(text([&]() { resize(g, g.count - 1); }) == "Cannot resize, max element is less than the current number of elements", "resize below the count");
    set_allow_replace(g, true);
    CHECK(g.deleted_elements.size() == marks0, "deleted_elements holds %zu ids after a load with %zu marks", g.deleted_elements.size(), marks0);
    mark(g, u);
    CHECK(g.deleted_elements.size() == marks0 + 1 && g.deleted_elements.count(u), "the new mark is not in deleted_elements");
    CHECK(text([&]() { upsert(g, rows.data(), first, false, lookup, vl); }) ==
              "Can't use addPoint to update deleted elements if replacement of deleted elements is enabled.", "update of a marked label");
    CHECK(text([&]() { mark(g, u); }) == "The requested to delete element is already deleted", "mark twice");
    const uint32_t v = *g.deleted_elements.begin();   // the slot the reference's rule hands out: u itself when u is the only mark
    const uint64_t gone = g.label(v);
    CHECK(marks0 != 0 || v == u, "the only vacancy is not the one just marked");
    const uint32_t got = upsert(g, rows.data(), ~0ull, true, lookup, vl);   // the full index still takes a replacement
    CHECK(got == v && g.label(v) == ~0ull && !g.deleted(v) && g.deleted_elements.size() == marks0 && !g.deleted_elements.count(v) &&
              !lookup.count(gone) && lookup.at(~0ull) == v && g.count == count0 && g.num_deleted() == marks0,
          "replacement on a full index");
  }
  remove(out.c_str()); remove(dir.c_str());
  if (fails) return 1;
  printf("upsert ok: %zu bytes compared, %zu touched\n", a.size(), t1);
  return 0;
}
