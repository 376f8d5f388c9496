// hnswlib_amd.h -- header-only C++ facade that re-creates the part of the reference's hnswlib API that
// sits on the searchKnn hot path, on top of the C ABI in include/hnsw_slim_amd.h (libhnsw_slim_amd.so).
//
// A caller written against the reference (include/strategy/hnsw_slim_strategy.h:38-114,
// hnsw_slim_server.cc:59-81) keeps its code: same namespace, class names, method names, argument meaning,
// exception type and messages.  What changes is where the work runs: loadIndex uploads the index to one
// MI355X, searchKnn runs the HIP beam-search kernel, and the new searchKnnBatch() is the fast entry
// (one wavefront per query; a single-query searchKnn is a batch of one and pays a kernel launch).
//
// Mirrors (paths relative to /root/reference/third_party/hnswlib/):
//   hnswlib.h:125-221        labeltype, BaseFilterFunctor, DISTFUNC, SpaceInterface, AlgorithmInterface
//   space_l2.h:208-253       L2Space            space_ip.h:342-398  InnerProductSpace
//   hnswalg.h:17-19,78-83,184,781,1378          HierarchicalNSW<float>
//   hnswalg_slim.h:28-30,83-87,149-152,193,753,867,1907,2030   HierarchicalNSWSlim<float>
// Filter functors are host callbacks: the facade evaluates one once per element into an allowed-array
// (cached per functor object) and calls hs_search_batch_filtered.
// HierarchicalNSW<float> also changes while resident: addPoint on an index with room -- of a new label, of an
// existing one (the reference's update) and with replace_deleted under the allow_replace_deleted constructor flag -- markDelete /
// unmarkDelete, resizeIndex, getDataByLabel, saveIndex (hnswalg.h:689-717, 896-1272, 1248-1376, 748-779).
// HierarchicalNSWSlim<float> is also the patch server's index: convertFromHNSWWithDiff from a resident
// HierarchicalNSW<float> and genPatch (hnswalg_slim.h:1110-1751), feeding patchFromStream clients.
// HierarchicalNSWSlimQ<float> has the strategy's build side too: rabitqlib::hnsw::HierarchicalNSW's constructor,
// construct and save (third_party/rabitqlib/index/hnsw/hnsw.hpp:427-500, 667-704) and convertFromHNSW(rabitqlib's index).
// Not provided: updateNeighborProbability other than 1.0, addPoint on Slim / SlimQ indexes, stop conditions.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <fstream>
#include <queue>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_set>
#include <utility>
#include <vector>

#include <unistd.h>

#include "../../include/hnsw_slim_amd.h"
#include "../csrc/dist_recipe.hpp"

namespace hnswlib {

typedef size_t labeltype;
typedef unsigned int tableint;

class BaseFilterFunctor {
 public:
  virtual bool operator()(hnswlib::labeltype) { return true; }
  virtual ~BaseFilterFunctor() {}
};

template <typename MTYPE>
using DISTFUNC = MTYPE (*)(const void *, const void *, const void *);

template <typename MTYPE>
class SpaceInterface {
 public:
  virtual size_t get_data_size() = 0;
  virtual DISTFUNC<MTYPE> get_dist_func() = 0;
  virtual void *get_dist_func_param() = 0;
  virtual ~SpaceInterface() {}
};

// The host-side distance functions are the same operation-for-operation recipes the kernel uses
// (dist_recipe.hpp), so values computed through the space agree bit for bit with search results.
class L2Space : public SpaceInterface<float> {
  size_t data_size_, dim_;
  static float fn(const void *a, const void *b, const void *p) {
    return hs::host_dist(hs::METRIC_L2, (const float *)a, (const float *)b, *(const size_t *)p);  // every dim
  }
 public:
  explicit L2Space(size_t dim) : data_size_(dim * sizeof(float)), dim_(dim) {}
  size_t get_data_size() override { return data_size_; }
  DISTFUNC<float> get_dist_func() override { return fn; }
  void *get_dist_func_param() override { return &dim_; }
};
class InnerProductSpace : public SpaceInterface<float> {
  size_t data_size_, dim_;
  static float fn(const void *a, const void *b, const void *p) {
    return hs::host_dist(hs::METRIC_IP, (const float *)a, (const float *)b, *(const size_t *)p);  // every dim
  }
 public:
  explicit InnerProductSpace(size_t dim) : data_size_(dim * sizeof(float)), dim_(dim) {}
  size_t get_data_size() override { return data_size_; }
  DISTFUNC<float> get_dist_func() override { return fn; }
  void *get_dist_func_param() override { return &dim_; }
};

template <typename dist_t>
class AlgorithmInterface {
 public:
  virtual void addPoint(const void *datapoint, labeltype label, bool replace_deleted = false) = 0;
  virtual std::priority_queue<std::pair<dist_t, labeltype>> searchKnn(const void *, size_t,
                                                                     BaseFilterFunctor *isIdAllowed = nullptr) const = 0;
  virtual std::vector<std::pair<dist_t, labeltype>> searchKnnCloserFirst(const void *query_data, size_t k,
                                                                        BaseFilterFunctor *isIdAllowed = nullptr) const {
    std::vector<std::pair<dist_t, labeltype>> result;  // hnswlib.h:203-221
    auto ret = searchKnn(query_data, k, isIdAllowed);
    size_t sz = ret.size();
    result.resize(sz);
    while (!ret.empty()) {
      result[--sz] = ret.top();
      ret.pop();
    }
    return result;
  }
  virtual void saveIndex(const std::string &location) = 0;
  virtual ~AlgorithmInterface() {}
};

namespace detail {
inline void check(hs_status s) {
  if (s != HS_OK) throw std::runtime_error(hs_last_error());  // same exception type/messages as the reference
}
inline int metric_of(SpaceInterface<float> *s) { return dynamic_cast<InnerProductSpace *>(s) ? HS_METRIC_IP : HS_METRIC_L2; }
inline size_t dim_of(SpaceInterface<float> *s) { return s->get_data_size() / sizeof(float); }

// Common device-index holder.
class DeviceIndex {
 protected:
  hs_index *h_ = nullptr;
  std::string path_;
  int metric_ = HS_METRIC_L2;
  size_t dim_ = 0;
  int device_ = 0;
  // more than one device: the index is replicated and searchKnnBatch shards the batch (hs_search_batch_sharded);
  // replicas_[0] == h_.  Single-query searchKnn stays on the first device.
  std::vector<int> devices_;
  std::vector<hs_index *> replicas_;
  hs_comm *comm_ = nullptr;
  hs_row_format row_fmt_ = HS_ROWS_F32;   // what setRowFormat asked for: applied to every index this object loads
  bool f32_resident_ = true;              // what setF32Resident asked for: likewise
  void free_replicas() {
    for (size_t r = 1; r < replicas_.size(); r++) hs_index_free(replicas_[r]);
    replicas_.clear();
    hs_comm_free(comm_);
    comm_ = nullptr;
  }

 public:
  size_t ef_ = 10;
  ~DeviceIndex() {
    drop_filter_cache();
    free_replicas();
    hs_index_free(h_);
  }
  void setDevice(int device) { device_ = device; devices_.clear(); }
  // Call before loadIndex: replicate the index on these devices (e.g. {0,1,...,7} on one MI355X node).
  void setDevices(const std::vector<int> &devices) {
    devices_ = devices;
    if (!devices.empty()) device_ = devices[0];
  }
  void setEf(size_t ef) {
    ef_ = ef;
    if (h_) check(hs_set_ef(h_, ef));
    for (size_t r = 1; r < replicas_.size(); r++) check(hs_set_ef(replicas_[r], ef));
  }
  // Narrow rows (hs_index_set_row_format; no counterpart in the reference): the flat kernel reads a u8 / fp16 copy of the rows.
  // The data must be representable exactly (integers 0..255 / values already rounded to fp16), and then no answer changes;
  // otherwise std::runtime_error with the C ABI's message and the index stays as it was.  Holds for later loads of this object too
  // (an index that is built on first use gets it after that build).
  void setRowFormat(hs_row_format f) {
    if (h_) check(hs_index_set_row_format(h_, f));
    for (size_t r = 1; r < replicas_.size(); r++) check(hs_index_set_row_format(replicas_[r], f));
    row_fmt_ = f;
  }
  hs_row_format rowFormat() const { return h_ ? (hs_row_format)hs_index_row_format(h_) : row_fmt_; }
  // fp32-free index (hs_index_set_f32_resident; no counterpart in the reference): false frees the fp32 rows of an index in a narrow
  // row format, and every search kernel then reads the narrow copy -- a quarter / half of the row bytes in HBM, no answer changes;
  // true re-creates them.  std::runtime_error in HS_ROWS_F32 format.  Holds for later loads of this object too, after setRowFormat.
  void setF32Resident(bool on) {
    if (h_) check(hs_index_set_f32_resident(h_, on ? 1 : 0));
    for (size_t r = 1; r < replicas_.size(); r++) check(hs_index_set_f32_resident(replicas_[r], on ? 1 : 0));
    f32_resident_ = on;
  }
  bool f32Resident() const { return h_ ? hs_index_f32_resident(h_) != 0 : f32_resident_; }
  bool sharded() const { return comm_ != nullptr; }
  hs_index *handle() const { return h_; }
  const std::string &path() const { return path_; }
  // indexSize(): the bytes the reference reports for this index's graph structure in ITS layout (hnswalg.h:1533-1547,
  // hnswalg_slim.h:2435-2444, hnswalg_slimq.h:2047-2057), so that the strategies' "index size" lines keep their meaning
  // (hnsw_slim_strategy.h:83,99); deviceBytes() is what the index holds in HBM here.
  size_t indexSize() const {
    if (!h_) return 0;
    hs_info info;
    check(hs_index_info(h_, &info));
    return (size_t)info.index_size;
  }
  size_t deviceBytes() const {
    if (!h_) return 0;
    hs_info info;
    check(hs_index_info(h_, &info));
    return (size_t)info.device_bytes;
  }

 protected:
  void load(const std::string &location, int kind, SpaceInterface<float> *s, size_t max_elements) {
    drop_filter_cache();
    hs_index_free(h_);
    h_ = nullptr;
    metric_ = metric_of(s);
    dim_ = dim_of(s);
    path_ = location;
    free_replicas();
    check(hs_index_load(location.c_str(), kind, metric_, dim_, max_elements, device_, &h_));
    if (devices_.size() > 1) {
      replicas_.assign(1, h_);
      for (size_t r = 1; r < devices_.size(); r++) {
        hs_index *h = nullptr;
        check(hs_index_load(location.c_str(), kind, metric_, dim_, max_elements, devices_[r], &h));
        replicas_.push_back(h);
      }
      check(hs_comm_init((int)devices_.size(), devices_.data(), &comm_));
    }
    ef_ = 10;  // hnswalg.h:864, hnswalg_slim.h:793
    if (row_fmt_ != HS_ROWS_F32) setRowFormat(row_fmt_);
    if (!f32_resident_) setF32Resident(false);
  }
  // an index made resident without a file (hs_graph_convert_slimq): this object owns it from here on; path() stays empty
  void adopt(hs_index *h, SpaceInterface<float> *s) {
    drop_filter_cache();
    hs_index_free(h_);
    free_replicas();
    h_ = h;
    metric_ = metric_of(s);
    dim_ = dim_of(s);
    path_.clear();
    ef_ = 10;
  }
  // searchKnn(q, k, isIdAllowed): the functor's answers are cached as a ONE-ROW filter set on the device (hs_filter_set_*), so the
  // second and later calls with the same functor evaluate nothing and upload nothing.  The cache belongs to (functor, loaded index):
  // dropped when the index is reloaded, and when its element count is no longer the one the set was created for (hs_index_patch on
  // handle() added elements); rebuilt on the next filtered call.
  mutable BaseFilterFunctor *cached_filter_ = nullptr;
  mutable uint64_t cached_n_ = 0;
  mutable hs_filter_set *filter_set_ = nullptr;
  void drop_filter_cache() const {
    hs_filter_set_free(filter_set_);
    filter_set_ = nullptr;
    cached_filter_ = nullptr;
  }

 public:
  // device bytes of the cached filter set (0 when none): one bitmap row of the index
  size_t filterCacheBytes() const {
    uint64_t b = 0;
    if (filter_set_) check(hs_filter_set_info(filter_set_, nullptr, nullptr, nullptr, &b));
    return (size_t)b;
  }

 protected:
  // the cached one-row filter set of functor f, (re)built when the functor or the element count changed
  const hs_filter_set *filter_row_set(BaseFilterFunctor *f) const {
    hs_info info;
    check(hs_index_info(h_, &info));
    if (f != cached_filter_ || !filter_set_ || cached_n_ != info.n) {  // evaluate the functor once per element (hs_labels: label of each internal id)
      drop_filter_cache();
      std::vector<uint64_t> all(info.n);
      check(hs_labels(h_, all.data()));
      std::vector<uint8_t> allowed(info.n);
      for (size_t i = 0; i < info.n; i++) allowed[i] = (*f)((labeltype)all[i]) ? 1 : 0;
      check(hs_filter_set_create(h_, 1, &filter_set_));
      check(hs_filter_set_write(filter_set_, 0, 1, allowed.data()));
      cached_filter_ = f;
      cached_n_ = info.n;
    }
    return filter_set_;
  }
  std::priority_queue<std::pair<float, labeltype>> search_pq(const void *q, size_t k, BaseFilterFunctor *f = nullptr) const {
    std::priority_queue<std::pair<float, labeltype>> result;
    if (!h_) return result;
    std::vector<uint64_t> labels(k);
    std::vector<float> dists(k);
    uint32_t cnt = 0;
    if (f) {
      const hs_filter_set *fs = filter_row_set(f);
      const uint32_t row = 0;
      check(hs_search_batch_filter_set(h_, fs, (const float *)q, 1, k, &row, labels.data(), dists.data(), &cnt, nullptr));
    } else
    check(hs_search_batch(h_, (const float *)q, 1, k, HS_MODE_PQ, nullptr, labels.data(), dists.data(), &cnt, nullptr));
    for (uint32_t i = 0; i < cnt; i++) result.emplace(dists[i], (labeltype)labels[i]);
    return result;
  }
  // Exact k-NN over the rows the index holds (hs_index_exact_search; no counterpart in the reference's graph classes): the
  // min(k, #candidates) smallest (dist, label) pairs among the elements that are not marked deleted and that f, when given,
  // allows.  Exact under a filter too -- not the reference's BruteforceSearch filtered overload, whose answer depends on the scan
  // order (bruteforce.h:118-131).  setEf / setExactOrder do not apply.
  std::priority_queue<std::pair<float, labeltype>> exact_pq(const void *q, size_t k, BaseFilterFunctor *f) const {
    std::priority_queue<std::pair<float, labeltype>> result;
    if (!h_) return result;
    std::vector<uint64_t> labels(k);
    std::vector<float> dists(k);
    uint32_t cnt = 0;
    const uint32_t row = 0;
    const hs_filter_set *fs = f ? filter_row_set(f) : nullptr;
    check(hs_index_exact_search(h_, fs, (const float *)q, 1, k, f ? &row : nullptr, labels.data(), dists.data(), &cnt));
    for (uint32_t i = 0; i < cnt; i++) result.emplace(dists[i], (labeltype)labels[i]);
    return result;
  }
  // every row of `queries` in one launch; out_* nq x k ascending by (dist, label), UINT64_MAX / +inf beyond out_counts[q] (nullable)
  void exact_batch(const float *queries, size_t nq, size_t k, uint64_t *out_labels, float *out_dists, uint32_t *out_counts) const {
    if (!h_) throw std::runtime_error("hnswlib_amd: no index loaded");
    check(hs_index_exact_search(h_, nullptr, queries, nq, k, nullptr, out_labels, out_dists, out_counts));
  }
};
}  // namespace detail

template <typename dist_t>
class HierarchicalNSW;

template <>
class HierarchicalNSW<float> : public AlgorithmInterface<float>, public detail::DeviceIndex {
  // build-then-search callers (include/strategy/hnsw_strategy.h:24-40: ctor, addPoint loop, saveIndex, setEf, searchKnn):
  // points are collected on the host, the graph is built by the CPU harness (hs_build_hnsw_labeled: the reference's
  // addPoint loop, serial => the same bytes) the first time it is needed, written to `saveIndex`'s path (or a temporary
  // file) and loaded onto the device.
  SpaceInterface<float> *space_ = nullptr;
  size_t max_elements_ = 0, M_ = 16, efc_ = 200, seed_ = 100;
  std::string branching_ = "16";
  std::vector<float> rows_;
  std::vector<uint64_t> row_labels_;
  bool dirty_ = false;
  int build_threads_ = 1;
  int build_device_ = -1;                       // setBuildOnDevice: the device the deferred build runs on (-1: the host builder)
  size_t build_batch_max_ = 0;
  hs_batch_build_stats build_stats_{};
  bool allow_replace_ = false;                  // the constructors' allow_replace_deleted
  bool has_image_ = false;                      // the loaded index keeps its host image (loaded with room)
  bool marks_changed_ = false;                  // markDelete / unmarkDelete since the load
  std::unordered_set<uint64_t> collected_;      // labels collected before the build: a repeated one is an update
  // what every (re)load of this object's index is followed by: whether it can change, and the constructor's replacement flag
  void after_load() {
    hs_info info;
    detail::check(hs_index_info(h_, &info));
    has_image_ = hs_index_capacity(h_) > info.n;
    marks_changed_ = false;
    if (allow_replace_ && has_image_) each_replica([&](hs_index *h) { detail::check(hs_index_set_replace_deleted(h, 1)); });
  }
  std::string tmp_path_;   // index file of a graph that was built here and never saved by the caller
  void materialize(const std::string &location) {
    if (row_labels_.empty()) throw std::runtime_error("hnswlib_amd: nothing to build (no addPoint calls)");
    if (build_device_ >= 0) {   // setBuildOnDevice: batched addPoint on the device (hs_build_hnsw_batched)
      hs_batch_build_opts o{};
      o.device = build_device_; o.threads = build_threads_; o.batch_max = build_batch_max_;
      detail::check(hs_build_hnsw_batched(rows_.data(), row_labels_.data(), row_labels_.size(), detail::dim_of(space_), detail::metric_of(space_),
                                          M_, efc_, branching_.c_str(), seed_, &o, location.c_str(), &build_stats_));
    } else {
      detail::check(hs_build_hnsw_labeled(rows_.data(), row_labels_.data(), row_labels_.size(), detail::dim_of(space_), detail::metric_of(space_),
                                          M_, efc_, branching_.c_str(), seed_, build_threads_, location.c_str()));
    }
    const size_t ef_keep = ef_;
    load(location, HS_KIND_HNSW, space_, max_elements_);
    setEf(ef_keep);
    dirty_ = false;
    after_load();
    // a later addPoint continues this build: the level generator as the constructor's seed left it after these points
    if (hs_index_capacity(h_) > row_labels_.size())
      each_replica([&](hs_index *h) { detail::check(hs_index_seed_levels(h, seed_, row_labels_.size())); });
  }
  // every replica of setDevices (as setExactOrder), or the one index
  template <class F>
  void each_replica(F f) {
    if (replicas_.empty()) f(h_);
    else for (hs_index *h : replicas_) f(h);
  }
  bool resident() const { return h_ && !dirty_; }
  void ensure_built() const {
    if (!dirty_) return;
    char tmpl[] = "/tmp/hnswlib_amd_XXXXXX";
    const int fd = mkstemp(tmpl);
    if (fd < 0) throw std::runtime_error("Cannot open file");
    close(fd);
    auto *self = const_cast<HierarchicalNSW *>(this);
    if (!self->tmp_path_.empty()) unlink(self->tmp_path_.c_str());
    self->tmp_path_ = tmpl;
    self->materialize(tmpl);
  }

 public:
  ~HierarchicalNSW() { if (!tmp_path_.empty()) unlink(tmp_path_.c_str()); }
  void build() const { ensure_built(); }   // force the deferred build (convertFromHNSW calls it)
  size_t indexSize() const { ensure_built(); return detail::DeviceIndex::indexSize(); }
  explicit HierarchicalNSW(SpaceInterface<float> *s) : space_(s) {}
  HierarchicalNSW(SpaceInterface<float> *s, const std::string &location, bool /*nmslib*/ = false, size_t max_elements = 0,
                  bool allow_replace_deleted = false) : space_(s), allow_replace_(allow_replace_deleted) {
    loadIndex(location, s, max_elements);
  }
  // hnswalg.h:85-159
  HierarchicalNSW(SpaceInterface<float> *s, size_t max_elements, size_t M = 16, size_t ef_construction = 200,
                  std::string branching_factor = "16", size_t random_seed = 100, bool allow_replace_deleted = false)
      : space_(s), max_elements_(max_elements), M_(M), efc_(ef_construction), seed_(random_seed), branching_(branching_factor),
        allow_replace_(allow_replace_deleted) {
    rows_.reserve(max_elements * detail::dim_of(s));
    row_labels_.reserve(max_elements);
  }
  void setBuildThreads(int t) { build_threads_ = t < 1 ? 1 : t; }   // 1 = the reference's serial addPoint loop, byte for byte
  // The deferred build as batched addPoint on HIP device `device` (hs_build_hnsw_batched; batch_max 0: its default schedule,
  // 1: the reference's serial order, byte for byte).  A negative device goes back to the host builder.  Not called: nothing changes.
  void setBuildOnDevice(int device, size_t batch_max = 0) { build_device_ = device < 0 ? -1 : device; build_batch_max_ = batch_max; }
  const hs_batch_build_stats &buildStats() const { return build_stats_; }   // of the last build that went through setBuildOnDevice
  void loadIndex(const std::string &location, SpaceInterface<float> *s, size_t max_elements_i = 0) {
    space_ = s;
    rows_.clear(); row_labels_.clear(); collected_.clear(); dirty_ = false;
    load(location, HS_KIND_HNSW, s, max_elements_i);
    after_load();
  }
  // addPoint on a resident index -- loaded with room (loadIndex(path, space, max_elements)), or built here and already searched --
  // is incremental (hs_index_add_points): the reference's insertion on the host image, the changed rows written in place on the
  // device.  Before the first search of an index under construction the points are collected as before.
  // On a resident index the call is the reference's addPoint(data, label, replace_deleted) whole (hs_index_upsert_points): an
  // existing label is updated, a new one with replace_deleted takes a deleted slot while there is one, anything else is appended.
  // While points are still being collected, a repeated label or replace_deleted = true first forces the build.
  void addPoint(const void *datapoint, labeltype label, bool replace_deleted = false) override {
    if (replace_deleted && !allow_replace_) throw std::runtime_error("Replacement of deleted elements is disabled in constructor");  // hnswalg.h:1027-1030
    if (dirty_ && (replace_deleted || collected_.count(label))) ensure_built();
    if (resident()) {
      const uint64_t l = label;
      const uint8_t flag = replace_deleted ? 1 : 0;
      each_replica([&](hs_index *h) { detail::check(hs_index_upsert_points(h, (const float *)datapoint, &l, &flag, 1)); });
      drop_filter_cache();   // a cached functor row is per internal id: an update or a replacement may have changed a slot's label
      return;
    }
    if (!space_ || max_elements_ == 0)
      throw std::runtime_error("hnswlib_amd: addPoint needs the (space, max_elements, M, ef_construction, ..) constructor");
    if (row_labels_.size() >= max_elements_)
      throw std::runtime_error("The number of elements exceeds the specified limit");  // hnswalg.h:1289-1291
    const size_t d = detail::dim_of(space_);
    rows_.insert(rows_.end(), (const float *)datapoint, (const float *)datapoint + d);
    row_labels_.push_back(label);
    collected_.insert(label);
    dirty_ = true;
  }
  // addPoint for a block of n new labels.  On a resident index with setBuildOnDevice in force (and one device) it is the batched add
  // (hs_index_add_points_batched: the batched order of the deferred build continued on the graph the index holds, on the index's
  // own device, with setBuildOnDevice's batch_max; buildStats() then reports this call); all or nothing, and an index that holds
  // delete marks is refused.  Otherwise it is a loop of addPoint.
  void addPoints(const float *rows, const labeltype *labels, size_t n) {
    if (build_device_ >= 0 && dirty_) ensure_built();
    if (build_device_ >= 0 && resident() && replicas_.size() <= 1) {
      std::vector<uint64_t> l(labels, labels + n);
      hs_batch_build_opts o{};
      o.device = device_; o.threads = build_threads_; o.batch_max = build_batch_max_;
      detail::check(hs_index_add_points_batched(h_, rows, l.data(), n, &o, &build_stats_));
      drop_filter_cache();
      return;
    }
    const size_t d = detail::dim_of(space_);
    for (size_t i = 0; i < n; i++) addPoint(rows + i * d, labels[i]);
  }
  // resizeIndex (hnswalg.h:689-717).  A resident index that keeps its host image moves its device arrays (hs_index_resize).  One
  // that was loaded without room has no host image: its file is loaded again with the new capacity -- unless delete marks changed
  // since the load, which that file does not hold.
  void resizeIndex(size_t new_max_elements) {
    if (!resident()) {
      if (new_max_elements < row_labels_.size())
        throw std::runtime_error("Cannot resize, max element is less than the current number of elements");
      max_elements_ = new_max_elements;
      return;
    }
    if (has_image_) {
      each_replica([&](hs_index *h) { detail::check(hs_index_resize(h, new_max_elements)); });
      return;
    }
    if (new_max_elements < getCurrentElementCount())
      throw std::runtime_error("Cannot resize, max element is less than the current number of elements");
    if (marks_changed_)
      throw std::runtime_error("hnswlib_amd: resizeIndex of an index loaded without spare capacity reloads its file, which does not hold the "
                               "delete marks set since the load (load it with max_elements above its size)");
    const size_t ef_keep = ef_;
    const std::string file = path_;
    load(file, HS_KIND_HNSW, space_, new_max_elements);
    setEf(ef_keep);
    max_elements_ = new_max_elements;
    after_load();
    if (!row_labels_.empty() && has_image_)   // built here: the level generator as the constructor's seed left it
      each_replica([&](hs_index *h) { detail::check(hs_index_seed_levels(h, seed_, row_labels_.size())); });
  }
  // saveIndex of a resident index that keeps its host image (hs_index_save): marks and added points included
  void saveIndex(const std::string &location) override {
    if (resident() && hs_index_save(h_, location.c_str()) == HS_OK) return;
    if (row_labels_.empty()) throw std::runtime_error("hnswlib_amd: the device index is read-only; the file it was loaded from is unchanged");
    if (resident() && hs_index_deleted_count(h_) > 0)
      throw std::runtime_error("hnswlib_amd: delete marks of an index built without spare capacity cannot be saved (construct it with max_elements above its size)");
    materialize(location);
  }
  void markDelete(labeltype label) {   // hnswalg.h:923-936
    ensure_built();
    const uint64_t l = label;
    each_replica([&](hs_index *h) { detail::check(hs_index_mark_deleted(h, &l, 1, 1)); });
    marks_changed_ = true;
  }
  void unmarkDelete(labeltype label) {   // hnswalg.h:968-981
    ensure_built();
    const uint64_t l = label;
    each_replica([&](hs_index *h) { detail::check(hs_index_mark_deleted(h, &l, 1, 0)); });
    marks_changed_ = true;
  }
  size_t getDeletedCount() const { return h_ ? hs_index_deleted_count(h_) : 0; }
  size_t getMaxElements() const { return resident() ? hs_index_capacity(h_) : max_elements_; }
  size_t getCurrentElementCount() const {
    if (!resident()) return row_labels_.size();
    hs_info info;
    detail::check(hs_index_info(h_, &info));
    return (size_t)info.n;
  }
  template <typename data_t>
  std::vector<data_t> getDataByLabel(labeltype label) const {   // hnswalg.h:896-917
    ensure_built();
    if (!h_) throw std::runtime_error("Label not found");
    std::vector<float> row(dim_);
    detail::check(hs_index_get_row(h_, label, row.data()));
    return std::vector<data_t>(row.begin(), row.end());
  }
  std::priority_queue<std::pair<float, labeltype>> searchKnn(const void *query_data, size_t k,
                                                             BaseFilterFunctor *isIdAllowed = nullptr) const override {
    ensure_built();
    return search_pq(query_data, k, isIdAllowed);
  }
  // Exact answers over the same resident rows (detail::DeviceIndex::exact_pq / exact_batch): ground truth without a second copy.
  std::priority_queue<std::pair<float, labeltype>> searchKnnExact(const void *query_data, size_t k, BaseFilterFunctor *isIdAllowed = nullptr) const {
    ensure_built();
    return exact_pq(query_data, k, isIdAllowed);
  }
  void searchKnnExactBatch(const float *queries, size_t nq, size_t k, uint64_t *out_labels, float *out_dists, uint32_t *out_counts = nullptr) const {
    ensure_built();
    exact_batch(queries, nq, k, out_labels, out_dists, out_counts);
  }
  // Batched searchKnn: nq x dim queries; out_labels / out_dists nq x k (unused slots: UINT64_MAX / +inf).
  void searchKnnBatch(const float *queries, size_t nq, size_t k, uint64_t *out_labels, float *out_dists,
                      uint32_t *out_counts) const {
    ensure_built();
    if (comm_) detail::check(hs_search_batch_sharded(comm_, replicas_.data(), queries, nq, k, HS_MODE_PQ, nullptr, out_labels, out_dists, out_counts));
    else detail::check(hs_search_batch(h_, queries, nq, k, HS_MODE_PQ, nullptr, out_labels, out_dists, out_counts, nullptr));
  }
};

template <typename dist_t>
class HierarchicalNSWSlim;

template <>
class HierarchicalNSWSlim<float> : public AlgorithmInterface<float>, public detail::DeviceIndex {
  SpaceInterface<float> *space_ = nullptr;
  int thr_ = 0;
  float p0_ = 0.02f, p_ = 0.02f;
  size_t M0h_ = 32, m0l_ = 8, Mh_ = 16, ml_ = 4;
  std::string tmp_path_;
  hs_slim_diff *diff_ = nullptr;   // the last convertFromHNSWWithDiff: changed_old_nodes_ / changed_new_nodes_ and genPatch's cursors
  bool diffed_ = false;            // the host image has moved on from the file this object was loaded from

  void run_diff(HierarchicalNSW<float> *hnsw, int threads) {
    if (!h_ || !hnsw) throw std::runtime_error("hnswlib_amd: convertFromHNSWWithDiff needs a loaded Slim index and a vanilla index");
    if (replicas_.size() > 1) throw std::runtime_error("hnswlib_amd: convertFromHNSWWithDiff is not provided on a sharded index");
    hnsw->build();
    hs_slim_diff *d = nullptr;
    detail::check(hs_slim_convert_diff(h_, hnsw->handle(), p0_, p_, M0h_, m0l_, Mh_, ml_, threads, &d, nullptr, nullptr));
    if (diff_) hs_slim_diff_free(diff_);
    diff_ = d;
    diffed_ = true;
  }

 public:
  explicit HierarchicalNSWSlim(SpaceInterface<float> *s) : space_(s) {}
  HierarchicalNSWSlim(SpaceInterface<float> *s, const std::string &location, bool /*nmslib*/ = false,
                      size_t max_elements = 0, bool /*allow_replace_deleted*/ = false) : space_(s) {
    loadIndex(location, s, max_elements);
  }
  // hnswalg_slim.h:89-143: the pruning parameters live in the object, convertFromHNSW(hnsw) uses them
  HierarchicalNSWSlim(SpaceInterface<float> *s, size_t /*max_elements*/, size_t /*M*/ = 16, size_t /*ef_construction*/ = 200,
                      size_t threshold_level = 0, float top_degree_percent0 = 0.02f, float top_degree_percent = 0.02f,
                      size_t top_degree_M0 = 32, size_t low_degree_m0 = 8, size_t top_degree_M = 16, size_t low_degree_m = 4,
                      size_t /*random_seed*/ = 100, bool /*allow_replace_deleted*/ = false)
      : space_(s), thr_((int)threshold_level), p0_(top_degree_percent0), p_(top_degree_percent), M0h_(top_degree_M0),
        m0l_(low_degree_m0), Mh_(top_degree_M), ml_(low_degree_m) {}
  ~HierarchicalNSWSlim() {
    if (diff_) hs_slim_diff_free(diff_);
    if (!tmp_path_.empty()) unlink(tmp_path_.c_str());
  }
  // the pruning parameters of an object that was loaded from a file (the reference's loading constructor takes them too)
  void setPruning(float top_degree_percent0, float top_degree_percent, size_t top_degree_M0, size_t low_degree_m0, size_t top_degree_M,
                  size_t low_degree_m) {
    p0_ = top_degree_percent0; p_ = top_degree_percent; M0h_ = top_degree_M0; m0l_ = low_degree_m0; Mh_ = top_degree_M; ml_ = low_degree_m;
  }
  // convertFromHNSWWithDiff(hnsw, output, to_add_data) (hnswalg_slim.h:1110-1424) on two resident indexes, both loaded with
  // max_elements > their element count: re-derives this index from `hnsw` with the object's pruning parameters, in place on the
  // device, and writes the whole stream -- count, the two list lengths, the old records, the new records without rows: what
  // patchFromStream(in, false) takes.  Returns the new ids when to_add_data (the rows the caller ships beside the stream).
  // The changed lists are ascending (the reference fills them in thread order); see INTEGRATION.md 9 for the other decisions.
  std::vector<tableint> convertFromHNSWWithDiff(HierarchicalNSW<float> *hnsw, std::ostream &output, bool to_add_data = false, int threads = 8) {
    run_diff(hnsw, threads);
    size_t len = 0;
    (void)hs_slim_diff_stream(diff_, h_, nullptr, 0, &len);
    std::string buf(len, '\0');
    detail::check(hs_slim_diff_stream(diff_, h_, &buf[0], buf.size(), &len));
    output.write(buf.data(), (std::streamsize)len);
    std::vector<tableint> ids;
    if (to_add_data) {
      size_t n_new = 0;
      detail::check(hs_slim_diff_info(diff_, nullptr, nullptr, &n_new, nullptr));
      ids.resize(n_new);
      detail::check(hs_slim_diff_ids(diff_, nullptr, ids.data()));
    }
    return ids;
  }
  // convertFromHNSWWithDiff(hnsw, changed_old_cnt, changed_new_cnt) (hnswalg_slim.h:1478-1751): the same conversion, the changed
  // lists kept in the object for genPatch, whose cursors start at the head of the new lists.
  void convertFromHNSWWithDiff(HierarchicalNSW<float> *hnsw, size_t &changed_old_cnt, size_t &changed_new_cnt, int threads = 8) {
    run_diff(hnsw, threads);
    detail::check(hs_slim_diff_info(diff_, nullptr, &changed_old_cnt, &changed_new_cnt, nullptr));
  }
  // genPatch (hnswalg_slim.h:1427-1476): the bare records, up to `limit` bytes of them; old_written / new_written are incremented
  // per record as the reference increments them.  As written there, the record that reaches `limit` is sent and its cursor is not
  // advanced: the next call sends that node again.  Returns `finished`.
  uint32_t genPatch(std::ostream &output, size_t &old_written, size_t &new_written, size_t limit, bool to_add = false) {
    if (!diff_) return 1;   // old_nodes_cnt_ == new_nodes_cnt_ == 0: both loops are empty
    size_t len = 0, ow = 0, nw = 0;
    int finished = 0;
    std::string buf(1 << 16, '\0');
    hs_status st = hs_slim_diff_next(diff_, h_, limit, to_add ? 1 : 0, &buf[0], buf.size(), &len, &ow, &nw, &finished);
    if (st == HS_ERR_CAPACITY) {   // the cursors have not moved: once more with the size it asked for
      buf.resize(len);
      st = hs_slim_diff_next(diff_, h_, limit, to_add ? 1 : 0, &buf[0], buf.size(), &len, &ow, &nw, &finished);
    }
    detail::check(st);
    output.write(buf.data() + 24, (std::streamsize)(len - 24));
    old_written += ow;
    new_written += nw;
    return (uint32_t)finished;
  }
  void loadIndex(const std::string &location, SpaceInterface<float> *s, size_t max_elements_i = 0) {
    space_ = s;
    load(location, HS_KIND_SLIM, s, max_elements_i);
  }
  // convertFromHNSW(hnsw) (hnswalg_slim.h:867-1108) with the object's parameters; the Slim file goes to a temporary
  // path until saveIndex names one
  void convertFromHNSW(HierarchicalNSW<float> *hnsw, int threads = 1) {
    hnsw->build();
    char tmpl[] = "/tmp/hnswlib_amd_slim_XXXXXX";
    const int fd = mkstemp(tmpl);
    if (fd < 0) throw std::runtime_error("Cannot open file");
    close(fd);
    if (!tmp_path_.empty()) unlink(tmp_path_.c_str());
    tmp_path_ = tmpl;
    convertFromHNSW(hnsw, space_, tmp_path_, thr_, p0_, p_, M0h_, m0l_, Mh_, ml_, threads);
  }
  // convertFromHNSW + saveIndex to `slim_location`, then load it on the device.
  void convertFromHNSW(HierarchicalNSW<float> *hnsw, SpaceInterface<float> *s, const std::string &slim_location,
                       int threshold_level = 0, float top_degree_percent0 = 0.02f, float top_degree_percent = 0.02f,
                       size_t top_degree_M0 = 32, size_t low_degree_m0 = 8, size_t top_degree_M = 16,
                       size_t low_degree_m = 4, int threads = 1) {
    hnsw->build();
    detail::check(hs_convert_slim(hnsw->path().c_str(), detail::metric_of(s), detail::dim_of(s), threshold_level,
                                  top_degree_percent0, top_degree_percent, top_degree_M0, low_degree_m0, top_degree_M,
                                  low_degree_m, threads, slim_location.c_str()));
    const size_t ef_keep = ef_;
    loadIndex(slim_location, s);
    setEf(ef_keep);
  }
  void addPoint(const void *, labeltype, bool = false) override {
    throw std::runtime_error("HierarchicalNSWSlim does not support addPoint");  // hnswalg_slim.h:149-152
  }
  // saveIndex (hnswalg_slim.h:717-751): the Slim file this object holds (written by convertFromHNSW or loaded), copied
  void saveIndex(const std::string &location) override {
    if (diffed_) { detail::check(hs_slim_index_save(h_, location.c_str())); return; }   // after convertFromHNSWWithDiff: the host image
    if (path_.empty()) throw std::runtime_error("hnswlib_amd: nothing to save");
    if (location == path_) return;
    std::ifstream in(path_, std::ios::binary);
    std::ofstream out(location, std::ios::binary);
    if (!in.is_open() || !out.is_open()) throw std::runtime_error("Cannot open file");
    out << in.rdbuf();
  }
  // searchKnn(q, k, filter) / searchKnn(q, k): hnswalg_slim.h:1783-1905 / 1907-2028
  std::priority_queue<std::pair<float, labeltype>> searchKnn(const void *query_data, size_t k,
                                                             BaseFilterFunctor *isIdAllowed = nullptr) const override {
    return search_pq(query_data, k, isIdAllowed);
  }
  // Exact answers over the same resident rows (detail::DeviceIndex::exact_pq / exact_batch): ground truth without a second copy.
  std::priority_queue<std::pair<float, labeltype>> searchKnnExact(const void *query_data, size_t k, BaseFilterFunctor *isIdAllowed = nullptr) const {
    return exact_pq(query_data, k, isIdAllowed);
  }
  void searchKnnExactBatch(const float *queries, size_t nq, size_t k, uint64_t *out_labels, float *out_dists, uint32_t *out_counts = nullptr) const {
    exact_batch(queries, nq, k, out_labels, out_dists, out_counts);
  }
  // searchKnn(q, k, tableint* result): hnswalg_slim.h:2030-2131.  k labels; same k-subset as the reference,
  // sorted by distance (call setExactOrder(true) to also reproduce the reference's array order).
  void searchKnn(const void *query_data, size_t k, tableint *result) const {
    if (!h_) return;  // cur_element_count_ == 0 (hnswalg_slim.h:2031-2032)
    detail::check(hs_search_batch(h_, (const float *)query_data, 1, k, HS_MODE_SLIM_IDS, result, nullptr, nullptr, nullptr, nullptr));
  }
  // The fast entry: every row of `queries` in one launch.
  // With setDevices({...}) before loadIndex the batch is sharded over the devices and gathered (RCCL over xGMI).
  void searchKnnBatch(const float *queries, size_t nq, size_t k, tableint *results) const {
    if (comm_) detail::check(hs_search_batch_sharded(comm_, replicas_.data(), queries, nq, k, HS_MODE_SLIM_IDS, results, nullptr, nullptr, nullptr));
    else detail::check(hs_search_batch(h_, queries, nq, k, HS_MODE_SLIM_IDS, results, nullptr, nullptr, nullptr, nullptr));
  }
  void setExactOrder(bool on) {
    detail::check(hs_set_exact_order(h_, on ? 1 : 0));
    for (size_t r = 1; r < replicas_.size(); r++) detail::check(hs_set_exact_order(replicas_[r], on ? 1 : 0));
  }
};

// BruteforceSearch (bruteforce.h): exhaustive scan.  addPoint keeps the rows on the host; searchKnn / searchKnnBatch
// run the exhaustive-scan kernel over them (hs_brute_force: same distances, same (dist, label) tie order).
template <typename dist_t>
class BruteforceSearch;

template <>
class BruteforceSearch<float> : public AlgorithmInterface<float> {
  std::vector<float> rows_;
  std::vector<uint64_t> labels_;
  size_t dim_ = 0, max_ = 0;
  int metric_ = HS_METRIC_L2;
 public:
  BruteforceSearch(SpaceInterface<float> *s, size_t maxElements) : dim_(detail::dim_of(s)), max_(maxElements), metric_(detail::metric_of(s)) {
    rows_.reserve(maxElements * dim_);
    labels_.reserve(maxElements);
  }
  void addPoint(const void *datapoint, labeltype label, bool = false) override {
    for (size_t i = 0; i < labels_.size(); i++)
      if (labels_[i] == label) {  // bruteforce.h:66-70: an existing label is overwritten in place
        std::copy((const float *)datapoint, (const float *)datapoint + dim_, rows_.begin() + i * dim_);
        return;
      }
    if (labels_.size() >= max_) throw std::runtime_error("The number of elements exceeds the specified limit\n");  // :72-74
    rows_.insert(rows_.end(), (const float *)datapoint, (const float *)datapoint + dim_);
    labels_.push_back(label);
  }
  void saveIndex(const std::string &) override { throw std::runtime_error("hnswlib_amd: BruteforceSearch::saveIndex is not provided"); }
  std::priority_queue<std::pair<float, labeltype>> searchKnn(const void *query_data, size_t k, BaseFilterFunctor *f = nullptr) const override {
    if (f) throw std::runtime_error("hnswlib_amd: BruteforceSearch with a filter is not provided");
    std::priority_queue<std::pair<float, labeltype>> r;
    if (labels_.empty()) return r;
    std::vector<uint64_t> lab(k);
    std::vector<float> d(k);
    uint32_t cnt = 0;
    detail::check(hs_brute_force(rows_.data(), labels_.size(), dim_, metric_, labels_.data(), (const float *)query_data, 1, k, 0, lab.data(),
                                 d.data(), &cnt));
    for (uint32_t i = 0; i < cnt; i++) r.emplace(d[i], (labeltype)lab[i]);
    return r;
  }
  // every row of `queries` in one launch; out_* are nq x k, ascending by (dist, label)
  void searchKnnBatch(const float *queries, size_t nq, size_t k, uint64_t *out_labels, float *out_dists, uint32_t *out_counts = nullptr) const {
    detail::check(hs_brute_force(rows_.data(), labels_.size(), dim_, metric_, labels_.data(), queries, nq, k, 0, out_labels, out_dists, out_counts));
  }
};

}  // namespace hnswlib

// rabitqlib::hnsw::HierarchicalNSW (third_party/rabitqlib/index/hnsw/hnsw.hpp) as the reference's SlimQ strategy uses it
// (include/strategy/hnsw_slimq_strategy.h:106-127): the constructor, construct() and save().  construct() builds the EDGES, from
// the raw rows, and keeps the centroid and cluster arguments for HierarchicalNSWSlimQ::convertFromHNSW, which writes the RaBitQ
// records; total_bits and faster_quant are accepted and not used.  save() writes the graph in hnswlib's saveIndex layout, the file
// the converters read.  setBuildOnDevice(device, batch_max) (no counterpart in the reference) moves construct() to the batched
// build on that HIP device (hs_build_rabitq_hnsw_batched_mem) and keeps the graph in memory (an hs_graph): save()
// writes it, and a file exists only once someone asks for graphPath(); without it construct() is hs_build_rabitq_hnsw on
// num_threads host threads (0: all of them; 1: the reference's serial construct(), edge for edge) into a temporary file.
namespace rabitqlib {
enum MetricType : std::uint8_t { METRIC_L2, METRIC_IP };
using PID = uint32_t;
namespace hnsw {
class HierarchicalNSW {
  size_t n_, dim_, M_, efc_, seed_;
  int metric_;
  int build_device_ = -1;
  size_t build_batch_max_ = 0;
  hs_batch_build_stats build_stats_{};
  mutable std::string tmp_path_;        // the graph construct() built, where it lies in a file
  hs_graph *graph_ = nullptr;           // ... and where it lies in memory (setBuildOnDevice)
  std::vector<float> centroids_;
  std::vector<PID> cluster_ids_;
  size_t num_clusters_ = 0;

 public:
  HierarchicalNSW(size_t num_points, size_t dim, size_t /*total_bits*/, size_t M, size_t ef_construction, size_t random_seed = 100,
                  MetricType metric_type = METRIC_L2)
      : n_(num_points), dim_(dim), M_(M), efc_(ef_construction), seed_(random_seed), metric_(metric_type == METRIC_IP ? HS_METRIC_IP : HS_METRIC_L2) {}
  HierarchicalNSW(const HierarchicalNSW &) = delete;
  HierarchicalNSW &operator=(const HierarchicalNSW &) = delete;
  ~HierarchicalNSW() {
    if (!tmp_path_.empty()) unlink(tmp_path_.c_str());
    hs_graph_free(graph_);
  }
  void setBuildOnDevice(int device, size_t batch_max = 0) { build_device_ = device < 0 ? -1 : device; build_batch_max_ = batch_max; }
  const hs_batch_build_stats &buildStats() const { return build_stats_; }   // of the last construct() that went through setBuildOnDevice
  void construct(size_t num_clusters, const float *centroids, size_t num_points, const float *data, const PID *cluster_ids, size_t num_threads = 0,
                 bool /*faster_quant*/ = false) {
    if (num_points != n_) throw std::runtime_error("hnswlib_amd: construct() with another number of points than the constructor's");
    if (!data) throw std::runtime_error("hnswlib_amd: construct() without rows");
    if (!tmp_path_.empty()) unlink(tmp_path_.c_str());
    tmp_path_.clear();
    hs_graph_free(graph_);
    graph_ = nullptr;
    const int threads = num_threads ? (int)num_threads : (int)std::max(1u, std::thread::hardware_concurrency());
    build_stats_ = hs_batch_build_stats{};
    if (build_device_ >= 0) {
      hs_batch_build_opts o{};
      o.device = build_device_;
      o.threads = threads;
      o.batch_max = build_batch_max_;
      hnswlib::detail::check(hs_build_rabitq_hnsw_batched_mem(data, n_, dim_, metric_, M_, efc_, seed_, &o, &graph_, &build_stats_));
    } else {
      const std::string tmpl = temp_file();
      tmp_path_ = tmpl;
      hnswlib::detail::check(hs_build_rabitq_hnsw(data, n_, dim_, metric_, M_, efc_, seed_, threads, tmpl.c_str()));
    }
    num_clusters_ = num_clusters;
    centroids_.assign(centroids, centroids + (centroids ? num_clusters * dim_ : 0));
    cluster_ids_.assign(cluster_ids, cluster_ids + (cluster_ids ? n_ : 0));
  }
  // save (hnsw.hpp:506-560 writes rabitqlib's own layout; here: the saveIndex layout every converter of this library reads)
  void save(const char *path) const {
    if (graph_) { hnswlib::detail::check(hs_graph_save(graph_, path)); return; }
    if (tmp_path_.empty()) throw std::runtime_error("hnswlib_amd: save() before construct()");
    std::ifstream in(tmp_path_, std::ios::binary);
    std::ofstream out(path, std::ios::binary);
    out << in.rdbuf();
    if (!in || !out) throw std::runtime_error("Cannot open file");
  }
  bool constructed() const { return graph_ || !tmp_path_.empty(); }
  const hs_graph *graph() const { return graph_; }              // the graph in memory (null unless setBuildOnDevice built it)
  const std::string &tempFile() const { return tmp_path_; }     // the temporary file this object holds, "" when it holds none
  // the graph as a file, for the converters that read one: a graph held in memory is written to a temporary file on first demand
  const std::string &graphPath() const {
    if (tmp_path_.empty() && graph_) {
      const std::string tmpl = temp_file();
      tmp_path_ = tmpl;
      hnswlib::detail::check(hs_graph_save(graph_, tmpl.c_str()));
    }
    return tmp_path_;
  }
  size_t dim() const { return dim_; }
  int metric() const { return metric_; }
  size_t numClusters() const { return num_clusters_; }
  const float *centroids() const { return centroids_.empty() ? nullptr : centroids_.data(); }
  const PID *clusterIds() const { return cluster_ids_.empty() ? nullptr : cluster_ids_.data(); }

 private:
  static std::string temp_file() {
    char tmpl[] = "/tmp/hnswlib_amd_rq_XXXXXX";
    const int fd = mkstemp(tmpl);
    if (fd < 0) throw std::runtime_error("hnswlib_amd: cannot create a temporary index file");
    close(fd);
    return tmpl;
  }
};
}  // namespace hnsw
}  // namespace rabitqlib

namespace hnswlib {

// HierarchicalNSWSlimQ (hnswalg_slimq.h): the RaBitQ-quantised variant.  Same call sequence as the reference's
// strategy (include/strategy/hnsw_slimq_strategy.h:72,142-156): loadIndex, setDataset, setEf, searchKnn(q, K, result); and its
// build side (:53-57, 106-141): the constructor with the pruning parameters, convertFromHNSW(rabitqlib's index), saveIndex.
template <typename dist_t>
class HierarchicalNSWSlimQ;

template <>
class HierarchicalNSWSlimQ<float> : public AlgorithmInterface<float>, public detail::DeviceIndex {
  SpaceInterface<float> *space_ = nullptr;
  int thr_ = 0;                          // hnswalg_slimq.h's constructor defaults
  float p0_ = 0.02f, p_ = 0.02f;
  size_t M0h_ = 32, m0l_ = 8, Mh_ = 16, ml_ = 4;
  std::string tmp_path_;                 // the SlimQ file convertFromHNSW wrote (host path)
  bool from_graph_ = false;              // convertFromHNSW made the index resident without a file (setBuildOnDevice)
  int convert_device_ = -1;
  hs_slimq_convert_stats convert_stats_{};

 public:
  explicit HierarchicalNSWSlimQ(SpaceInterface<float> *s) : space_(s) {}
  // (no counterpart in the reference) convertFromHNSW on that HIP device: both steps and the index's tiles there, no file written
  // or read (hs_graph_convert_slimq); the index it leaves is word for word the one the two host calls and a
  // load leave, and saveIndex writes their file from the index's host image.
  void setBuildOnDevice(int device) { convert_device_ = device < 0 ? -1 : device; }
  const hs_slimq_convert_stats &convertStats() const { return convert_stats_; }   // of the last convertFromHNSW that went through setBuildOnDevice
  const std::string &tempFile() const { return tmp_path_; }   // the temporary file this object holds, "" when it holds none
  HierarchicalNSWSlimQ(SpaceInterface<float> *s, size_t /*max_elements*/, size_t /*M*/ = 16, size_t /*ef_construction*/ = 200, int threshold_level = 0,
                       float top_degree_percent0 = 0.02f, float top_degree_percent = 0.02f, size_t top_degree_M0 = 32, size_t low_degree_m0 = 8,
                       size_t top_degree_M = 16, size_t low_degree_m = 4)
      : space_(s), thr_(threshold_level), p0_(top_degree_percent0), p_(top_degree_percent), M0h_(top_degree_M0), m0l_(low_degree_m0),
        Mh_(top_degree_M), ml_(low_degree_m) {}
  ~HierarchicalNSWSlimQ() { if (!tmp_path_.empty()) unlink(tmp_path_.c_str()); }
  // convertFromHNSW(hnsw) (hnswalg_slimq.h:1471-1790) on the graph construct() built: the graph passes (hs_convert_slimq_graph), the
  // RaBitQ records with the centroids and cluster ids construct() was given (hs_convert_slimq), then the result is loaded.  After
  // setBuildOnDevice: the same two steps on that device, chained in memory.
  void convertFromHNSW(rabitqlib::hnsw::HierarchicalNSW *hnsw, int threads = 8, uint64_t flip_seed = 1) {
    if (!hnsw || !hnsw->constructed()) throw std::runtime_error("hnswlib_amd: convertFromHNSW needs a constructed rabitqlib index");
    if (!space_) throw std::runtime_error("hnswlib_amd: convertFromHNSW needs the space the index was constructed with");
    if (!hnsw->centroids()) throw std::runtime_error("hnswlib_amd: convertFromHNSW needs the centroids construct() was given");
    if (!tmp_path_.empty()) unlink(tmp_path_.c_str());
    tmp_path_.clear();
    convert_stats_ = hs_slimq_convert_stats{};
    if (convert_device_ >= 0) {   // in memory all the way: the graph handle (read from the file of a host-built graph), a resident index
      hs_graph *loaded = nullptr;
      if (!hnsw->graph()) detail::check(hs_graph_load(hnsw->graphPath().c_str(), hnsw->metric(), hnsw->dim(), &loaded));
      hs_slimq_params p{};
      p.threshold_level = thr_; p.top_degree_percent0 = p0_; p.top_degree_percent = p_;
      p.top_degree_M0 = M0h_; p.low_degree_m0 = m0l_; p.top_degree_M = Mh_; p.low_degree_m = ml_;
      p.centroids = hnsw->centroids(); p.num_cluster = hnsw->numClusters(); p.cluster_ids = hnsw->clusterIds(); p.flip_seed = flip_seed;
      hs_index *ix = nullptr;
      const hs_status s = hs_graph_convert_slimq(loaded ? loaded : hnsw->graph(), &p, convert_device_, threads, nullptr, device_, 0, &ix, &convert_stats_);
      hs_graph_free(loaded);
      detail::check(s);
      adopt(ix, space_);
      from_graph_ = true;
      return;
    }
    from_graph_ = false;
    char slim[] = "/tmp/hnswlib_amd_rqslim_XXXXXX", slimq[] = "/tmp/hnswlib_amd_slimq_XXXXXX";
    const int fd = mkstemp(slim), fq = mkstemp(slimq);
    if (fd >= 0) close(fd);
    if (fq >= 0) close(fq);
    if (fd < 0 || fq < 0) throw std::runtime_error("hnswlib_amd: cannot create a temporary index file");
    tmp_path_ = slimq;
    hs_status s = hs_convert_slimq_graph(hnsw->graphPath().c_str(), hnsw->metric(), hnsw->dim(), thr_, p0_, p_, M0h_, m0l_, Mh_, ml_, threads, slim);
    if (s == HS_OK)
      s = hs_convert_slimq(slim, hnsw->metric(), hnsw->dim(), hnsw->centroids(), hnsw->numClusters(), hnsw->clusterIds(), flip_seed, threads, slimq);
    unlink(slim);
    detail::check(s);
    loadIndex(slimq, space_);
  }
  HierarchicalNSWSlimQ(SpaceInterface<float> *s, const std::string &location, bool /*nmslib*/ = false,
                       size_t max_elements = 0, bool /*allow_replace_deleted*/ = false) {
    loadIndex(location, s, max_elements);
  }
  void loadIndex(const std::string &location, SpaceInterface<float> *s, size_t max_elements_i = 0) {
    space_ = s;
    from_graph_ = false;
    load(location, HS_KIND_SLIMQ, s, max_elements_i);
  }
  // setDataset (hnswalg_slimq.h:303-305): the raw rows, indexed by internal id, for the exact re-rank
  void setDataset(std::vector<std::vector<float>> *data_set) {
    if (!h_ || !data_set || data_set->empty()) return;
    const size_t n = data_set->size(), d = (*data_set)[0].size();
    std::vector<float> flat(n * d);
    for (size_t i = 0; i < n; i++) std::copy((*data_set)[i].begin(), (*data_set)[i].end(), flat.begin() + i * d);
    detail::check(hs_slimq_set_dataset(h_, flat.data(), n, d));
  }
  void setDataset(const float *rows, size_t n, size_t d) { detail::check(hs_slimq_set_dataset(h_, rows, n, d)); }
  void setTConst(double t) { detail::check(hs_slimq_set_tconst(h_, t)); }
  void setRowFormat(hs_row_format) { throw std::runtime_error("narrow rows: a SlimQ index has no flat-kernel rows"); }
  void setF32Resident(bool) { throw std::runtime_error("narrow rows: a SlimQ index has no flat-kernel rows"); }
  void addPoint(const void *, labeltype, bool = false) override {
    throw std::runtime_error("HierarchicalNSWSlimQ does not support addPoint");  // hnswalg_slimq.h:298-301
  }
  // saveIndex (hnswalg_slimq.h:1161-1216) after convertFromHNSW: the file it wrote, copied
  void saveIndex(const std::string &location) override {
    if (from_graph_ && h_) { detail::check(hs_slimq_index_save(h_, location.c_str())); return; }   // the index's host image
    if (tmp_path_.empty() || path_ != tmp_path_)
      throw std::runtime_error("hnswlib_amd: the device index is read-only; the file it was loaded from is unchanged");
    std::ifstream in(tmp_path_, std::ios::binary);
    std::ofstream out(location, std::ios::binary);
    out << in.rdbuf();
    if (!in || !out) throw std::runtime_error("Cannot open file");
  }
  // the priority_queue overloads of the reference print "todo: searchKnn()" and return nothing (:1795-1808)
  std::priority_queue<std::pair<float, labeltype>> searchKnn(const void *, size_t, BaseFilterFunctor * = nullptr) const override {
    return {};
  }
  // searchKnn(q, k, tableint* result): hnswalg_slimq.h:1810-1924 -- k labels in the reference's heap-array order
  void searchKnn(const void *query_data, size_t k, tableint *result) const {
    if (!h_) return;
    std::vector<uint64_t> lab(k);
    detail::check(hs_slimq_search_batch(h_, (const float *)query_data, 1, k, lab.data(), nullptr, nullptr, nullptr));
    for (size_t i = 0; i < k; i++) result[i] = (tableint)lab[i];
  }
  // The fast entry: every row of `queries` in one launch; results nq x k.
  void searchKnnBatch(const float *queries, size_t nq, size_t k, tableint *results) const {
    std::vector<uint64_t> lab(nq * k);
    detail::check(hs_slimq_search_batch(h_, queries, nq, k, lab.data(), nullptr, nullptr, nullptr));
    for (size_t i = 0; i < nq * k; i++) results[i] = (tableint)lab[i];
  }
};

// A search queue on a loaded HierarchicalNSW<float> / HierarchicalNSWSlim<float> (hs_queue_*; no counterpart in the reference): a
// server's worker threads each call searchKnn(q, k) -- or submit / wait with their own small batches -- on ONE queue object, and
// whatever is pending when a thread starts to wait leaves as one search launch.  Every answer is bit for bit the index's own
// searchKnn(q, k) / searchKnnBatch.  k is fixed per queue; ef is the index's at the moment of a flush.  Every method is safe from
// any thread (drain() releases the tickets it completes: a wait() that loses that race throws "unknown ticket" with its results
// already in place -- stop the workers before draining).  Changing the index in place (addPoint, markDelete, resizeIndex on an
// index loaded with room, setRowFormat, ...) wants drain() first.  Calls that free and reload the index's device handle --
// loadIndex, setDevices, resizeIndex on an index loaded without room, and the destructor -- want the queue DESTROYED first: it
// holds that handle.
template <typename dist_t>
class SearchQueue;

template <>
class SearchQueue<float> {
  hs_queue *q_ = nullptr;
  size_t k_ = 0;

  void open(hs_index *h, size_t max_queries, int slots) {
    if (!h) throw std::runtime_error("hnswlib_amd: no index loaded");
    detail::check(hs_queue_create(h, k_, HS_MODE_PQ, max_queries, slots, nullptr, &q_));
  }

 public:
  typedef uint64_t ticket_t;
  SearchQueue(HierarchicalNSW<float> &index, size_t k, size_t max_queries = 8192, int slots = 2) : k_(k) {
    index.build();   // (an index still being filled by addPoint is built and uploaded here)
    open(index.handle(), max_queries, slots);
  }
  SearchQueue(HierarchicalNSWSlim<float> &index, size_t k, size_t max_queries = 8192, int slots = 2) : k_(k) {
    open(index.handle(), max_queries, slots);
  }
  SearchQueue(const SearchQueue &) = delete;
  SearchQueue &operator=(const SearchQueue &) = delete;
  ~SearchQueue() { hs_queue_free(q_); }   // drains first

  size_t k() const { return k_; }
  // nq x dim rows (copied before this returns -- unless they lie in page-locked, device-mapped memory: those are read in place and
  // stay unchanged until wait); out_labels / out_dists nq x k and out_counts nq as searchKnnBatch writes them, valid after wait(ticket)
  ticket_t submit(const float *queries, size_t nq, uint64_t *out_labels, float *out_dists, uint32_t *out_counts) {
    ticket_t t = 0;
    detail::check(hs_queue_submit(q_, queries, nq, nullptr, nullptr, out_labels, out_dists, out_counts, nullptr, &t));
    return t;
  }
  void flush() { detail::check(hs_queue_flush(q_)); }
  void wait(ticket_t t) { detail::check(hs_queue_wait(q_, t)); }
  void drain() { detail::check(hs_queue_drain(q_)); }
  struct hs_queue_info info() const {
    struct hs_queue_info i;
    detail::check(hs_queue_info(q_, &i));
    return i;
  }
  // searchKnn(q, k) of the index, thread-safe, by submit + wait: queries of threads that arrive together share a launch.
  std::priority_queue<std::pair<float, labeltype>> searchKnn(const void *query_data, size_t k) {
    if (k != k_) throw std::runtime_error("hnswlib_amd: this SearchQueue answers k = " + std::to_string(k_));
    uint64_t labels[64];
    float dists[64];
    std::vector<uint64_t> lv;
    std::vector<float> dv;
    uint64_t *lp = labels;
    float *dp = dists;
    if (k > 64) { lv.resize(k); dv.resize(k); lp = lv.data(); dp = dv.data(); }
    uint32_t cnt = 0;
    wait(submit((const float *)query_data, 1, lp, dp, &cnt));
    std::priority_queue<std::pair<float, labeltype>> result;
    for (uint32_t i = 0; i < cnt; i++) result.emplace(dp[i], (labeltype)lp[i]);
    return result;
  }
};

}  // namespace hnswlib
