// host_graph.hpp -- the code that decides the bytes of a built HNSW file and of a converted Slim file, and nothing else (the
// benchmark keys its cached dataset and index by this file; DESIGN.md "Host code layout"):
//   * VanillaGraph : hnswlib::HierarchicalNSW memory image; serial-reproducible builder (harness, restating
//                    hnswalg.h:229-322, 481-687, 1248-1376) + saveIndex/loadIndex (hnswalg.h:748-893).  A serial build writes
//                    a file byte-identical to the reference's (tests/test_host_cpu.py vs tests/golden/*.hnsw.bin).
//   * SlimGraph    : hnswlib::HierarchicalNSWSlim image: convertFromHNSW (hnswalg_slim.h:836-1108),
//                    saveIndex/loadIndex (hnswalg_slim.h:717-815).
// Everything else about these two images is free functions in headers of their own: resume and the update path
// (host_update.hpp), the SlimQ base graph and its conversion (host_rq_graph.hpp), convertFromHNSWWithDiff / genPatch
// (slim_diff.hpp), the device conversions (slim_convert_gpu.hpp), the packed form the GPU consumes (packed_index.hpp).
// Index construction/pruning is harness for the search path (SURVEY.md 2, rows 5-6 "harness"); it is CPU code.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <mutex>
#include <queue>
#include <random>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

#include "dist_recipe.hpp"
#include "host_parallel.hpp"
#include "index_check.hpp"

namespace hs {

using pairfi = std::pair<float, uint32_t>;
struct CmpFirst { bool operator()(const pairfi &a, const pairfi &b) const { return a.first < b.first; } };  // hnswalg.h:176-182
using MaxQ = std::priority_queue<pairfi, std::vector<pairfi>, CmpFirst>;

// Where a serialized index comes from: a file, or the same bytes already in host memory (hs_index_load_mem).
struct BinSource {
  std::string path;
  const char *mem = nullptr;
  size_t len = 0;
  BinSource(const std::string &p) : path(p) {}
  BinSource(const char *p) : path(p) {}
  BinSource(const void *m, size_t n) : mem((const char *)m), len(n) {}
};
struct MemBuf : std::streambuf {
  MemBuf(const char *b, size_t n) { setg(const_cast<char *>(b), const_cast<char *>(b), const_cast<char *>(b) + n); }
  pos_type seekoff(off_type off, std::ios_base::seekdir dir, std::ios_base::openmode) override {
    char *base = eback(), *end = egptr();
    char *to = dir == std::ios_base::beg ? base + off : dir == std::ios_base::end ? end + off : gptr() + off;
    if (to < base || to > end) return pos_type(off_type(-1));
    setg(base, to, end);
    return pos_type(to - base);
  }
  pos_type seekpos(pos_type pos, std::ios_base::openmode m) override { return seekoff(off_type(pos), std::ios_base::beg, m); }
};
struct BinReader {
  std::ifstream file;
  MemBuf mb;
  std::istream mem_in;
  std::istream &in;
  explicit BinReader(const BinSource &s) : mb(s.mem, s.mem ? s.len : 0), mem_in(&mb), in(s.mem ? mem_in : static_cast<std::istream &>(file)) {
    if (!s.mem) {
      file.open(s.path, std::ios::binary);
      if (!file.is_open()) throw std::runtime_error("Cannot open file");
    }
  }
  template <typename T> T pod() {
    T v;
    in.read((char *)&v, sizeof(T));
    if (!in) throw std::runtime_error("Index seems to be corrupted or unsupported");
    return v;
  }
  void bytes(void *dst, size_t n) {
    in.read((char *)dst, n);
    if (!in) throw std::runtime_error("Index seems to be corrupted or unsupported");
  }
};
template <typename T> static void put(std::ostream &o, const T &v) { o.write((const char *)&v, sizeof(T)); }

// getRandomLevel (hnswalg.h:217-221): one draw of `gen`
template <class Gen>
inline int level_from(Gen &gen, double mult) {
  std::uniform_real_distribution<double> distribution(0.0, 1.0);
  return (int)(-log(distribution(gen)) * mult);
}

inline double branching_mult(const std::string &bf, size_t) {  // hnswalg.h:143-158
  if (bf == "e") return 1 / log(M_E);
  if (bf == "sqrt") return 1 / log(sqrt(2.0) / (sqrt(2.0) - 1));
  try {
    return 1 / log(std::stod(bf));
  } catch (const std::invalid_argument &) {
    throw std::runtime_error("Invalid branching factor: " + bf);
  } catch (const std::out_of_range &) {
    throw std::runtime_error("Branching factor out of range: " + bf);
  }
}

// ------------------------------------------------------------------------------------------------
struct VanillaGraph {
  size_t max_elements = 0, count = 0, dim = 0;
  size_t M = 0, maxM = 0, maxM0 = 0, efC = 0;
  size_t size_links0 = 0, size_per_el = 0, offsetData = 0, label_offset = 0, size_links_up = 0;
  double mult = 0;
  int maxlevel = -1;
  uint32_t enterpoint = (uint32_t)-1;
  Metric metric = METRIC_L2;
  std::vector<char> level0;                 // max_elements * size_per_el
  std::vector<std::vector<char>> links;     // per element: level * size_links_up (+1 as the reference mallocs)
  std::vector<int> levels;
  std::unique_ptr<std::mutex[]> locks;
  std::mutex global;
  // when set: every node whose level-0 list connect() or the update path wrote (new and updated nodes included)
  std::vector<uint32_t> *touched0 = nullptr;
  std::mutex touched_mu;
  // State that only host_update.hpp reads; load() resets the generator.
  // level_generator_ as the reference holds it -- default-constructed after loadIndex (the loading constructor, hnswalg.h:78-83,
  // seeds nothing), seeded by the building constructor (:113)
  std::default_random_engine level_gen;
  // allow_replace_deleted_ and deleted_elements (hnswalg.h:70-73).  The set is the reference's own container type on purpose:
  // `*deleted_elements.begin()` decides which slot addPoint(.., true) reuses, and that is a property of libstdc++'s hash table
  // and of the sequence of inserts and erases, which host_update.hpp keeps as the reference's.
  bool allow_replace = false;
  std::unordered_set<uint32_t> deleted_elements;

  void init(size_t n, size_t d, Metric m, size_t M_, size_t efC_, const std::string &bf) {
    max_elements = n; dim = d; metric = m;
    M = M_ > 10000 ? 10000 : M_;           // hnswalg.h:97-107
    maxM = M; maxM0 = 2 * M;
    efC = std::max(efC_, M);
    size_links0 = maxM0 * 4 + 4;            // hnswalg.h:116
    size_per_el = size_links0 + 4 * d + 8;
    offsetData = size_links0;
    label_offset = size_links0 + 4 * d;
    size_links_up = maxM * 4 + 4;           // hnswalg.h:141-142
    mult = branching_mult(bf, M);
    level0.assign(n * size_per_el, 0);
    links.assign(n, {});
    levels.assign(n, 0);
    locks.reset(new std::mutex[n]);
    count = 0; maxlevel = -1; enterpoint = (uint32_t)-1;
  }
  char *el(uint32_t i) { return level0.data() + (size_t)i * size_per_el; }
  const char *el(uint32_t i) const { return level0.data() + (size_t)i * size_per_el; }
  const float *vec(uint32_t i) const { return (const float *)(el(i) + offsetData); }
  uint64_t label(uint32_t i) const { uint64_t l; memcpy(&l, el(i) + label_offset, 8); return l; }
  uint32_t *list_at(uint32_t i, int level) {  // hnswalg.h:543-547: [u16 cnt][u16][u32 ids...]
    return level == 0 ? (uint32_t *)el(i) : (uint32_t *)(links[i].data() + (size_t)(level - 1) * size_links_up);
  }
  const uint32_t *list_at(uint32_t i, int level) const { return const_cast<VanillaGraph *>(this)->list_at(i, level); }
  static uint16_t cnt_of(const uint32_t *l) { return *(const uint16_t *)l; }       // hnswalg.h:1012-1014
  static void set_cnt(uint32_t *l, uint16_t c) { *(uint16_t *)l = c; }              // hnswalg.h:1016-1018
  bool deleted(uint32_t i) const { return (((const unsigned char *)el(i))[2] & 1) != 0; }
  float dist(const float *a, const float *b) const { return host_dist(metric, a, b, dim); }

  struct Visited {
    std::vector<uint16_t> mass; uint16_t cur = 0;
    void begin(size_t n) {
      if (mass.size() != n) { mass.assign(n, 0); cur = 0; }
      if (++cur == 0) { std::fill(mass.begin(), mass.end(), 0); cur = 1; }
    }
  };

  // searchBaseLayer (hnswalg.h:229-322): build-time beam with ef_construction.
  MaxQ search_layer(uint32_t ep, const float *q, int layer, Visited &vl) {
    vl.begin(max_elements);
    MaxQ top, cand;
    float lower;
    if (!deleted(ep)) {
      float d = dist(q, vec(ep));
      top.emplace(d, ep);
      lower = d;
      cand.emplace(-d, ep);
    } else {
      lower = std::numeric_limits<float>::max();
      cand.emplace(-lower, ep);
    }
    vl.mass[ep] = vl.cur;
    while (!cand.empty()) {
      pairfi c = cand.top();
      if ((-c.first) > lower && top.size() == efC) break;
      cand.pop();
      uint32_t node = c.second;
      std::unique_lock<std::mutex> lk(locks[node]);
      const uint32_t *l = list_at(node, layer);
      size_t n = cnt_of(l);
      for (size_t j = 0; j < n; j++) {
        uint32_t id = l[1 + j];
        if (vl.mass[id] == vl.cur) continue;
        vl.mass[id] = vl.cur;
        float d = dist(q, vec(id));
        if (top.size() < efC || lower > d) {
          cand.emplace(-d, id);
          if (!deleted(id)) top.emplace(d, id);
          if (top.size() > efC) top.pop();
          if (!top.empty()) lower = top.top().first;
        }
      }
    }
    return top;
  }

  // getNeighborsByHeuristic2 (hnswalg.h:481-523)
  void heuristic(MaxQ &top, size_t Mlim) const {
    if (top.size() < Mlim) return;
    std::priority_queue<pairfi> closest;  // default pair ordering, as the reference
    std::vector<pairfi> keep;
    while (!top.empty()) { closest.emplace(-top.top().first, top.top().second); top.pop(); }
    while (!closest.empty()) {
      if (keep.size() >= Mlim) break;
      pairfi cur = closest.top();
      float dq = -cur.first;
      closest.pop();
      bool good = true;
      for (const pairfi &s : keep) {
        float d = dist(vec(s.second), vec(cur.second));
        if (d < dq) { good = false; break; }
      }
      if (good) keep.push_back(cur);
    }
    for (const pairfi &p : keep) top.emplace(-p.first, p.second);
  }

  // mutuallyConnectNewElement (hnswalg.h:549-687).  is_update (:575-577, 584, 591, 624-636): cur_c's list may hold ids -- it is
  // shortened with the count alone, the old ids stay behind it and saveIndex writes them -- and a neighbour that already lists
  // cur_c is left as it is.
  uint32_t connect(uint32_t cur_c, MaxQ &top, int level, bool is_update = false) {
    size_t Mcurmax = level ? maxM : maxM0;
    heuristic(top, M);
    if (top.size() > M) throw std::runtime_error("Should be not be more than M_ candidates returned by the heuristic");
    std::vector<uint32_t> sel;
    sel.reserve(M);
    while (!top.empty()) { sel.push_back(top.top().second); top.pop(); }
    uint32_t next_ep = sel.back();
    if (level == 0 && touched0) {
      std::lock_guard<std::mutex> g(touched_mu);
      touched0->push_back(cur_c);
      touched0->insert(touched0->end(), sel.begin(), sel.end());
    }
    {
      uint32_t *l = list_at(cur_c, level);
      if (*l && !is_update) throw std::runtime_error("The newly inserted element should have blank link list");
      set_cnt(l, sel.size());
      for (size_t i = 0; i < sel.size(); i++) {
        if (l[1 + i] && !is_update) throw std::runtime_error("Possible memory corruption");
        if (level > levels[sel[i]]) throw std::runtime_error("Trying to make a link on a non-existent level");
        l[1 + i] = sel[i];
      }
    }
    for (size_t i = 0; i < sel.size(); i++) {
      std::unique_lock<std::mutex> lk(locks[sel[i]]);
      uint32_t *lo = list_at(sel[i], level);
      size_t sz = cnt_of(lo);
      if (sz > Mcurmax) throw std::runtime_error("Bad value of sz_link_list_other");
      if (sel[i] == cur_c) throw std::runtime_error("Trying to connect an element to itself");
      if (level > levels[sel[i]]) throw std::runtime_error("Trying to make a link on a non-existent level");
      uint32_t *data = lo + 1;
      bool present = false;
      if (is_update)
        for (size_t j = 0; j < sz; j++)
          if (data[j] == cur_c) { present = true; break; }
      if (present) continue;
      if (sz < Mcurmax) {
        data[sz] = cur_c;
        set_cnt(lo, sz + 1);
      } else {
        float dmax = dist(vec(cur_c), vec(sel[i]));
        MaxQ cands;
        cands.emplace(dmax, cur_c);
        for (size_t j = 0; j < sz; j++) cands.emplace(dist(vec(data[j]), vec(sel[i])), data[j]);
        heuristic(cands, Mcurmax);
        int idx = 0;
        while (!cands.empty()) { data[idx++] = cands.top().second; cands.pop(); }
        set_cnt(lo, idx);
      }
    }
    return next_ep;
  }

  // The greedy walk of the upper levels: from (cur, curdist) down levels from .. to + 1, moving to whichever neighbour dist_to(id)
  // puts nearer, until none is.  lock: addPoint's walk (hnswalg.h:1300-1326), which holds the node's lock and range-checks each
  // candidate; repairConnectionsForUpdate's (:1166-1190) does neither.
  template <class DistTo>
  void descend(uint32_t &cur, float &curdist, int from, int to, bool lock, DistTo dist_to) {
    for (int level = from; level > to; level--) {
      bool changed = true;
      while (changed) {
        changed = false;
        std::unique_lock<std::mutex> lk;
        if (lock) lk = std::unique_lock<std::mutex>(locks[cur]);
        const uint32_t *l = list_at(cur, level);
        const int n = cnt_of(l);
        for (int i = 0; i < n; i++) {
          const uint32_t cand = l[1 + i];
          if (lock && cand > max_elements) throw std::runtime_error("cand error");
          const float d = dist_to(cand);
          if (d < curdist) { curdist = d; cur = cand; changed = true; }
        }
      }
    }
  }

  // The head of addPoint for a new element (hnswalg.h:1281-1298): its lock, the global lock (kept only while the element may
  // raise the maximum level), the cleared element with label, row and upper lists; `ep` is the enter point it starts from.
  struct Insert {
    std::unique_lock<std::mutex> lock_el, templock;
    int maxlevelcopy;
    uint32_t ep;
  };
  Insert begin_insert(const float *x, uint64_t label, uint32_t cur_c, int curlevel) {
    Insert in;
    in.lock_el = std::unique_lock<std::mutex>(locks[cur_c]);
    levels[cur_c] = curlevel;
    in.templock = std::unique_lock<std::mutex>(global);
    in.maxlevelcopy = maxlevel;
    if (curlevel <= in.maxlevelcopy) in.templock.unlock();
    in.ep = enterpoint;
    memset(el(cur_c), 0, size_per_el);
    memcpy(el(cur_c) + label_offset, &label, 8);
    memcpy(el(cur_c) + offsetData, x, 4 * dim);
    if (curlevel) links[cur_c].assign(size_links_up * curlevel + 1, 0);
    return in;
  }
  // Its tail (:1362-1374): the first element, or one above the maximum level, becomes the enter point.
  void adopt_entry(uint32_t cur_c, int curlevel, const Insert &in) {
    if ((int32_t)in.ep == -1) {
      enterpoint = 0;
      maxlevel = curlevel;
    }
    if (curlevel > in.maxlevelcopy) {
      enterpoint = cur_c;
      maxlevel = curlevel;
    }
  }

  // addPoint(data, label, level=-1) for a NEW label (hnswalg.h:1248-1376). cur_c and its level are
  // supplied by the caller so that serial and parallel builds assign ids == insertion index.
  void add_point(const float *x, uint64_t label, uint32_t cur_c, int curlevel, Visited &vl) {
    const Insert in = begin_insert(x, label, cur_c, curlevel);
    if ((int32_t)in.ep != -1) {
      uint32_t currObj = in.ep;
      if (curlevel < in.maxlevelcopy) {
        float curdist = dist(x, vec(currObj));
        descend(currObj, curdist, in.maxlevelcopy, curlevel, true, [&](uint32_t id) { return dist(x, vec(id)); });
      }
      bool epDeleted = deleted(in.ep);
      for (int level = std::min(curlevel, in.maxlevelcopy); level >= 0; level--) {
        MaxQ top = search_layer(currObj, x, level, vl);
        if (epDeleted) {
          top.emplace(dist(x, vec(in.ep)), in.ep);
          if (top.size() > efC) top.pop();
        }
        currObj = connect(cur_c, top, level);
      }
    }
    adopt_entry(cur_c, curlevel, in);
  }

  // Build over rows 0..n-1 with labels == row index.  Levels are drawn up front from the reference's
  // generator in row order (std::default_random_engine seeded `seed`, hnswalg.h:113,217-221), so a
  // threads==1 build reproduces the reference's serial addPoint loop bit for bit; threads>1 keeps
  // ids == labels (the reference's parallel build does not, hnswalg.h:1279-1281) but the graph then
  // depends on thread timing, exactly as upstream hnswlib.
  void build(const float *base, size_t n, size_t d, Metric m, size_t M_, size_t efC_, const std::string &bf,
             size_t seed, int threads, const uint64_t *labels = nullptr) {
    init(n, d, m, M_, efC_, bf);
    std::default_random_engine gen;
    gen.seed(seed);
    std::vector<int> lv(n);
    for (size_t i = 0; i < n; i++) lv[i] = level_from(gen, mult);
    if (threads < 1) threads = 1;
    std::vector<Visited> vl(threads);
    const size_t serial_head = threads > 1 ? std::min<size_t>(n, 1) : n;
    // threads > 1: the first point of the empty graph serially, the rest in parallel
    for (size_t i = 0; i < serial_head; i++) { count = i + 1; add_point(base + i * d, labels ? labels[i] : i, (uint32_t)i, lv[i], vl[0]); }
    count = n;
    parallel_for(n - serial_head, threads, 1, [&](size_t k, int tid) {
      const size_t i = serial_head + k;
      add_point(base + i * d, labels ? labels[i] : i, (uint32_t)i, lv[i], vl[tid]);
    });
  }

  void set_deleted(uint32_t i, bool on) {   // markDeletedInternal / unmarkDeletedInternal's byte (hnswalg.h:946-947, 989-990)
    unsigned char *b = (unsigned char *)el(i) + 2;
    *b = on ? (*b | 1) : (*b & ~1);
  }
  void note_touched0(uint32_t i) {
    if (!touched0) return;
    std::lock_guard<std::mutex> g(touched_mu);
    touched0->push_back(i);
  }

  void save(const std::string &path) const {  // hnswalg.h:748-779
    std::ofstream o(path, std::ios::binary);
    if (!o.is_open()) throw std::runtime_error("Cannot open file");
    put<uint64_t>(o, 0);  // offsetLevel0_
    put<uint64_t>(o, max_elements);
    put<uint64_t>(o, count);
    put<uint64_t>(o, size_per_el);
    put<uint64_t>(o, label_offset);
    put<uint64_t>(o, offsetData);
    put<int32_t>(o, maxlevel);
    put<uint32_t>(o, enterpoint);
    put<uint64_t>(o, maxM);
    put<uint64_t>(o, maxM0);
    put<uint64_t>(o, M);
    put<double>(o, mult);
    put<uint64_t>(o, efC);
    o.write(level0.data(), count * size_per_el);
    for (size_t i = 0; i < count; i++) {
      uint32_t sz = levels[i] > 0 ? size_links_up * levels[i] : 0;
      put<uint32_t>(o, sz);
      if (sz) o.write(links[i].data(), sz);
    }
  }

  void load(const BinSource &src, Metric m, size_t d, size_t max_elements_i = 0) {  // hnswalg.h:781-893
    BinReader r(src);
    r.in.seekg(0, r.in.end);
    std::streamoff total = r.in.tellg();
    r.in.seekg(0, r.in.beg);
    uint64_t off0 = r.pod<uint64_t>();
    uint64_t file_max = r.pod<uint64_t>();
    count = r.pod<uint64_t>();
    max_elements = max_elements_i < count ? file_max : max_elements_i;
    size_per_el = r.pod<uint64_t>();
    label_offset = r.pod<uint64_t>();
    offsetData = r.pod<uint64_t>();
    maxlevel = r.pod<int32_t>();
    enterpoint = r.pod<uint32_t>();
    maxM = r.pod<uint64_t>();
    maxM0 = r.pod<uint64_t>();
    M = r.pod<uint64_t>();
    mult = r.pod<double>();
    efC = r.pod<uint64_t>();
    metric = m; dim = d;
    size_links0 = maxM0 * 4 + 4;
    size_links_up = maxM * 4 + 4;
    if (off0 != 0 || offsetData != size_links0 || size_per_el != size_links0 + 4 * d + 8 ||
        (std::streamoff)(96 + count * size_per_el) > total)
      throw std::runtime_error("Index seems to be corrupted or unsupported");
    level0.assign(std::max<size_t>(max_elements, count) * size_per_el, 0);
    r.bytes(level0.data(), count * size_per_el);
    links.assign(std::max<size_t>(max_elements, count), {});
    levels.assign(std::max<size_t>(max_elements, count), 0);
    for (size_t i = 0; i < count; i++) {
      uint32_t sz = r.pod<uint32_t>();
      if (sz) {
        if (sz % size_links_up) throw std::runtime_error("Index seems to be corrupted or unsupported");
        levels[i] = sz / size_links_up;
        links[i].resize(sz + 1);
        r.bytes(links[i].data(), sz);
      }
    }
    if (r.in.tellg() != total) throw std::runtime_error("Index seems to be corrupted or unsupported");  // :835-836
    if (check()) throw std::runtime_error(kCorruptText);   // before any caller indexes with an id, a count or a level of the file
    locks.reset(new std::mutex[std::max<size_t>(max_elements, count)]);
    level_gen = std::default_random_engine();
  }
  size_t num_deleted() const { size_t c = 0; for (size_t i = 0; i < count; i++) c += deleted(i); return c; }
  // The first precondition of index_check.hpp this image violates, nullptr when it is safe to pack and to search.
  const char *check() const {
    auto level_of = [&](size_t i) { return levels[i]; };
    if (const char *bad = check_entry(count, enterpoint, maxlevel, 0, true, level_of)) return bad;
    return check_lists(count, level_of, [](size_t) { return true; }, [&](size_t i, int l, const uint32_t *&ids, size_t &cnt) {
      const uint32_t *ll = list_at((uint32_t)i, l);
      cnt = cnt_of(ll);
      ids = ll + 1;
      return cnt <= (l ? maxM : maxM0);
    });
  }
};


struct SlimParams {
  int threshold_level = 0;
  float top_pct0 = 0.02f, top_pct = 0.02f;                 // alpha_0, alpha
  size_t top_M0 = 32, low_m0 = 8, top_M = 16, low_m = 4;   // M_h0, M_l0, M_h, M_l
};

struct SlimGraph {
  size_t count = 0, dim = 0, size_per_el = 0;
  size_t maxM = 0, maxM0 = 0, M = 0, efC = 0;
  int maxlevel = 0, threshold_level = 0;
  uint32_t enterpoint = 0;
  bool has_deleted = false;
  Metric metric = METRIC_L2;
  std::vector<char> elements;            // count * (24 + 4*dim): [i32 level][u32 total][u64 label][8B ptr][data]
  std::vector<std::vector<char>> blobs;  // [u16 cum_off[level]][u32 ids[total]]

  const char *el(uint32_t i) const { return elements.data() + (size_t)i * size_per_el; }
  int32_t level(uint32_t i) const { int32_t v; memcpy(&v, el(i), 4); return v; }
  uint32_t total(uint32_t i) const { uint32_t v; memcpy(&v, el(i) + 4, 4); return v; }
  uint64_t label(uint32_t i) const { uint64_t v; memcpy(&v, el(i) + 8, 8); return v; }
  const float *vec(uint32_t i) const { return (const float *)(el(i) + 24); }
  bool deleted(uint32_t i) const { return (((const unsigned char *)el(i))[6] & 1) != 0; }  // hnswalg_slim.h:1776-1781

  // PruneByHeuristic (hnswalg_slim.h:836-865): input sorted ascending by distance.
  static void prune(const VanillaGraph &g, const std::vector<pairfi> &sorted, std::vector<uint32_t> &out, size_t Mlim) {
    out.clear();
    for (const pairfi &cur : sorted) {
      if (out.size() >= Mlim) break;
      bool good = true;
      for (uint32_t kept : out) {
        float d = g.dist(g.vec(kept), g.vec(cur.second));
        if (d < cur.first) { good = false; break; }
      }
      if (good) out.push_back(cur.second);
    }
  }

  // degree histograms per level (:904-922) and hub thresholds (:923-945)
  static std::vector<size_t> hub_thresholds(const VanillaGraph &g, const SlimParams &p) {
    const int maxlevel = g.maxlevel;
    const size_t n = g.count, maxM0 = g.maxM0;
    std::vector<std::vector<size_t>> hist(maxlevel + 1, std::vector<size_t>(maxM0 + 2, 0));
    std::vector<size_t> level_cnts(maxlevel + 1, 0);
    for (size_t i = 0; i < n; i++) {
      for (int l = 1; l <= g.levels[i]; l++) { level_cnts[l]++; hist[l][VanillaGraph::cnt_of(g.list_at(i, l))]++; }
      hist[0][VanillaGraph::cnt_of(g.list_at(i, 0))]++;
    }
    std::vector<size_t> thr(maxlevel + 1, 0);
    // NB: level_cnts[0] is never incremented by the reference (:910-912 start at l=1), so topN==0
    // at level 0, `acc >= topN` holds at the first bucket and thr[0] = maxM0+1: no level-0 list is
    // ever classed as a hub (every node is pruned to M_l0).  Mirrored, not fixed.
    size_t acc = 0, topN = (size_t)(level_cnts[0] * p.top_pct0 + 0.5);
    for (size_t d = hist[0].size() - 1; d > 0; --d) { acc += hist[0][d]; if (acc >= topN) { thr[0] = d; break; } }
    for (int l = 1; l <= maxlevel; l++) {
      acc = 0; topN = (size_t)(level_cnts[l] * p.top_pct + 0.5);
      for (size_t d = hist[l].size() - 1; d > 0; --d) { acc += hist[l][d]; if (acc >= topN) { thr[l] = d; break; } }
    }
    return thr;
  }
  void take_header(const VanillaGraph &g, const SlimParams &p) {
    count = g.count; dim = g.dim; metric = g.metric;
    has_deleted = g.num_deleted() > 0;
    maxM = g.maxM; maxM0 = g.maxM0; M = g.M; efC = g.efC;
    maxlevel = g.maxlevel; enterpoint = g.enterpoint; threshold_level = p.threshold_level;
    size_per_el = 24 + 4 * dim;
  }
  // Element i from its final per-level lists (after the re-prune): hierarchical filter (:1063-1084), offsets, blob (:1085-1106).
  template <class GetList>
  void assemble_node(const VanillaGraph &g, size_t i, const GetList &list_of) {
    char *e = elements.data() + i * size_per_el;
    int32_t L = g.levels[i];
    memcpy(e, &L, 4);
    memcpy(e + 24, g.vec(i), 4 * dim);
    uint64_t lab = g.label(i);
    memcpy(e + 8, &lab, 8);
    std::vector<uint32_t> nbrs_out;
    std::vector<uint16_t> offs;
    for (int l = 0; l <= L; l++) {
      size_t cnt = 0;
      const uint32_t *nbrs = list_of(i, l, cnt);
      if (l == threshold_level) {
        nbrs_out.insert(nbrs_out.end(), nbrs, nbrs + cnt);
      } else {  // hierarchical pruning: keep neighbours whose own top level == l (:1072-1083)
        for (size_t j = 0; j < cnt; j++)
          if (g.levels[nbrs[j]] == l) nbrs_out.push_back(nbrs[j]);
      }
      offs.push_back((uint16_t)nbrs_out.size());
    }
    uint32_t total = nbrs_out.size();
    memcpy(e + 4, &total, 4);
    if (total == 0) return;  // neighbors pointer stays null (:1091-1094)
    blobs[i].resize(2 * (size_t)L + 4 * (size_t)total);
    memcpy(blobs[i].data(), offs.data(), 2 * (size_t)L);
    memcpy(blobs[i].data() + 2 * (size_t)L, nbrs_out.data(), 4 * (size_t)total);
  }

  // convertFromHNSW (hnswalg_slim.h:867-1108) with prune(g, sorted, out, Mlim) as its PruneByHeuristic and D(a, b) as the distance
  // between two nodes (hnsw->fstdistfunc_, :977-979); host_rq_graph.hpp runs the same passes with HNSW-SlimQ's pair.
  void convert(const VanillaGraph &g, const SlimParams &p, int threads) {
    convert(g, p, threads,
            [](const VanillaGraph &gg, const std::vector<pairfi> &sorted, std::vector<uint32_t> &out, size_t Mlim) { prune(gg, sorted, out, Mlim); },
            [&](uint32_t a, uint32_t b) { return g.dist(g.vec(a), g.vec(b)); });
  }
  template <class Prune, class Dist>
  void convert(const VanillaGraph &g, const SlimParams &p, int threads, Prune prune, Dist D) {
    take_header(g, p);
    const size_t n = count;
    const std::vector<size_t> thr = hub_thresholds(g, p);
    std::vector<std::vector<std::vector<uint32_t>>> nn(n), rev(n);
    auto par = [&](auto fn) { parallel_for(n, threads, 64, [&](size_t v, int) { fn(v); }); };
    par([&](size_t v) {  // :951-986
      int L = g.levels[v];
      nn[v].resize(L + 1); rev[v].resize(L + 1);
      std::vector<pairfi> heap;
      for (int l = 0; l <= L; l++) {
        const uint32_t *ll = g.list_at(v, l);
        size_t size = VanillaGraph::cnt_of(ll);
        size_t M0 = l == 0 ? (size > thr[l] ? p.top_M0 : p.low_m0) : (size > thr[l] ? p.top_M : p.low_m);
        heap.resize(size);
        for (size_t j = 0; j < size; j++) heap[j] = {D(v, ll[1 + j]), ll[1 + j]};
        std::sort(heap.begin(), heap.end(), CmpFirst());
        prune(g, heap, nn[v][l], M0);
      }
    });
    for (size_t v = 0; v < n; v++)  // reverse edges (:988-998); serial: order of emplace_back is irrelevant after the sort below
      for (int l = 0; l <= g.levels[v]; l++)
        for (uint32_t u : nn[v][l]) rev[u][l].push_back(v);
    par([&](size_t v) {  // union + sort + unique (:999-1012)
      for (int l = 0; l <= g.levels[v]; l++) {
        auto &a = nn[v][l];
        a.insert(a.end(), rev[v][l].begin(), rev[v][l].end());
        std::sort(a.begin(), a.end());
        a.erase(std::unique(a.begin(), a.end()), a.end());
      }
    });
    elements.assign(n * size_per_el, 0);
    blobs.assign(n, {});
    par([&](size_t i) {  // :1014-1107
      std::vector<pairfi> heap;
      for (int l = 0; l <= g.levels[i]; l++) {
        auto &nbrs = nn[i][l];
        size_t limit = l == 0 ? maxM0 : maxM;
        if (nbrs.size() > limit) {  // re-prune (:1038-1062)
          heap.resize(nbrs.size());
          for (size_t j = 0; j < nbrs.size(); j++) heap[j] = {D((uint32_t)i, nbrs[j]), nbrs[j]};
          std::sort(heap.begin(), heap.end(), CmpFirst());
          prune(g, heap, nbrs, limit);
        }
      }
      assemble_node(g, i, [&](size_t v, int l, size_t &cnt) { cnt = nn[v][l].size(); return nn[v][l].data(); });
    });
  }

  void save(const std::string &path) const {  // hnswalg_slim.h:717-751
    std::ofstream o(path, std::ios::binary);
    if (!o.is_open()) throw std::runtime_error("Cannot open file");
    put<uint64_t>(o, count); put<uint64_t>(o, size_per_el);
    put<uint64_t>(o, 8); put<uint64_t>(o, 4); put<uint64_t>(o, 24); put<uint64_t>(o, 16);
    put<int32_t>(o, maxlevel); put<int32_t>(o, threshold_level); put<uint32_t>(o, enterpoint);
    put<uint64_t>(o, maxM); put<uint64_t>(o, maxM0); put<uint64_t>(o, M); put<uint64_t>(o, efC);
    put<uint8_t>(o, has_deleted ? 1 : 0);
    o.write(elements.data(), count * size_per_el);
    for (size_t i = 0; i < count; i++) {
      uint32_t sz = 2 * (uint32_t)level(i) + 4 * total(i);  // get_neighbor_size (:652-661)
      put<uint32_t>(o, sz);
      if (sz && total(i) != 0) o.write(blobs[i].data(), sz);
    }
  }

  void load(const BinSource &src, Metric m, size_t d) {  // hnswalg_slim.h:753-815
    BinReader r(src);
    metric = m; dim = d;
    count = r.pod<uint64_t>();
    size_per_el = r.pod<uint64_t>();
    uint64_t label_off = r.pod<uint64_t>(), off_total = r.pod<uint64_t>(), off_data = r.pod<uint64_t>(), off_nb = r.pod<uint64_t>();
    maxlevel = r.pod<int32_t>();
    threshold_level = r.pod<int32_t>();
    enterpoint = r.pod<uint32_t>();
    maxM = r.pod<uint64_t>(); maxM0 = r.pod<uint64_t>(); M = r.pod<uint64_t>(); efC = r.pod<uint64_t>();
    has_deleted = r.pod<uint8_t>() != 0;
    if (label_off != 8 || off_total != 4 || off_data != 24 || off_nb != 16 || size_per_el != 24 + 4 * d)
      throw std::runtime_error("Index seems to be corrupted or unsupported");
    elements.resize(count * size_per_el);
    r.bytes(elements.data(), elements.size());
    blobs.assign(count, {});
    for (size_t i = 0; i < count; i++) {
      uint32_t sz = r.pod<uint32_t>();
      if (total(i) == 0) continue;   // no blob follows (save() above; hnswalg_slim.h:745-748)
      if (level(i) < 0 || sz != 2 * (uint64_t)level(i) + 4 * (uint64_t)total(i)) throw std::runtime_error("Index seems to be corrupted or unsupported");
      blobs[i].resize(sz);
      r.bytes(blobs[i].data(), sz);
    }
    if (check()) throw std::runtime_error(kCorruptText);   // before any caller indexes with an id, an offset or a level of the file
  }
  // The first precondition of index_check.hpp this image violates, nullptr when it is safe to pack and to search.
  const char *check() const {
    return check_chal(count, enterpoint, maxlevel, threshold_level, [&](size_t i) { return (int)level((uint32_t)i); },
                      [&](size_t i) { return (size_t)total((uint32_t)i); }, [&](size_t i) -> const std::vector<char> & { return blobs[i]; });
  }
};

}  // namespace hs
