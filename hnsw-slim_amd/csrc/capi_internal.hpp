// capi_internal.hpp -- what the C ABI's translation units (capi_*.cpp) share: error reporting and the guard (capi_guard.hpp), the
// device buffer, the index and filter-set objects behind the opaque handles, the shared refusals, and the few functions that cross
// files.  No CPU search path exists in this library: without a HIP device every search call returns HS_ERR_DEVICE.
// The rule for an exported entry: if its body can throw -- it allocates, builds a string, touches a container or calls into host_*.hpp --
// it runs inside one guarded(...) at the entry itself (capi_guard.hpp), and the functions below it let exceptions pass; a refusal
// that more than one entry reports is a function here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/hnsw_slim_amd.h"
#include "capi_guard.hpp"
#include "engine.hpp"
#include "narrow_rows.hpp"
#include "host_graph.hpp"
#include "packed_index.hpp"
#include "host_tiles.hpp"
#include "rabitq_host.hpp"
#include "search_plan.hpp"
#include "slim_diff.hpp"
#include "slimq_engine.hpp"

using namespace hs;

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) return fail(HS_ERR_DEVICE, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  hipError_t alloc(size_t count) {
    release();
    if (count == 0) return hipSuccess;
    const hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
    if (e == hipSuccess) n = count;   // (a failed allocation leaves the buffer empty: the next ensure() tries again)
    else p = nullptr;
    return e;
  }
  hipError_t ensure(size_t count) { return count <= n ? hipSuccess : alloc(count); }
  hipError_t upload(const std::vector<T> &v) {
    hipError_t e = alloc(std::max<size_t>(v.size(), 1));
    if (e != hipSuccess) return e;
    return v.empty() ? hipSuccess : hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { release(); }
};

struct hs_index {
  int device = 0;
  hs_info info{};
  size_t ef = 10;  // hnswalg.h:864, hnswalg_slim.h:793
  uint32_t user_cand_cap = 0, user_hash_slots = 0;
  uint32_t grow_cand = 0, grow_hash = 0;  // adaptive: doublings learnt from earlier batches' overflow counts
  bool exact_order = false;               // always use the strict kernel (reference output order)
  const char *last_kernel = "";           // the kernel that served pass 0 of the most recent search call (hs_last_kernel)
  // patching (hs_index_patch): a Slim index loaded with max_elements > count keeps its host image and has row capacity
  std::unique_ptr<SlimGraph> host_slim;
  size_t cap_rows = 0;
  // hs_slim_convert_diff: the Slim index's label_lookup_ (hnswalg_slim.h:61), built from the host image by the first call
  // (buildLabelLookup :216-220) and merged into by every call (:1121)
  SlimLookup slim_lookup;
  bool slim_lookup_built = false;
  uint64_t slim_gen = 0;   // counts the calls that re-derived the host image: a diff object belongs to one of them
  // live updates (capi_update.cpp): a vanilla index loaded with max_elements > count keeps its host image too (addPoint continues
  // on it, hs_index_save writes it); the label -> internal id map (the reference's label_lookup_) and the number of delete marks
  // is built from host_labels the first time a call needs it; the number of delete marks (num_deleted_) follows every upload
  std::unique_ptr<VanillaGraph> host_vanilla;
  std::unordered_map<uint64_t, uint32_t> label_to_id;
  bool label_map_built = false;
  size_t num_deleted = 0;
  bool has_dup0 = false;         // some level-0 list names an id twice (PackedIndex::repeats_id0, refreshed by upload_small)
  DevBuf<uint32_t> upd_stage;    // the records of the update call being applied (grow-only)
  std::vector<uint32_t> last_add_changed;   // hs_debug_batched_add_changed: old nodes whose lists the last device-side batched add changed
  size_t last_add_downloaded = 0;           // ... and the old lists it downloaded (those that received an id)
  DevIndex dev{};
  DevBuf<float> vec;
  DevBuf<uint32_t> row_ptr0, cols, up_base, up_ptr, tile0, uptile;
  DevBuf<uint64_t> labels;
  DevBuf<uint8_t> deleted;
  // narrow rows (hs_index_set_row_format): a u8 / fp16 copy of `vec` in the flat kernel's lane-major layout (narrow_rows.hip), sized
  // like `vec` (row capacity x dim values).  While `vec` is resident every kernel but the flat one reads it; once it has been dropped
  // (hs_index_set_f32_resident(ix, 0), hs_index_load_narrow: f32_resident = false, vec.p = dev.vec = null) every search launch goes to
  // the narrow twin of the chosen kernel and nothing on the device holds fp32 rows
  int row_fmt = ROWS_F32;
  bool f32_resident = true;
  DevBuf<uint8_t> narrow;
  DevBuf<uint32_t> narrow_bad;   // the conversion kernel's "first row that does not fit" word
  size_t base_bytes = 0;         // info.device_bytes without the narrow copy, fp32 rows counted (refresh_device_bytes)
  // per-stream scratch (grow-only): calls on different HIP streams may be in flight together
  struct StreamWs {
    DevBuf<uint32_t> spill;             // visited-set tier 2, nq x kSpillSlots
    DevBuf<uint32_t> prep;              // SlimQ: per-query preparation records
    DevBuf<uint32_t> status, counters;  // counters: 3 passes x 4 {visited overflow, candidate overflow, tie hazard, tier-2 spills}
    DevBuf<uint32_t> entry, order;      // two-launch fast pass: level-0 entries (nq x 4 words) and the start order
    DevBuf<uint32_t> fb;                // last-resort pass: kFbGrid x (candidate heap + tier-2 visited set)
    uint32_t oflip = 0;
    size_t last_nq = 0;
    // hs_search_batch_async: device staging of the queries and outputs of the call in flight on this stream
    DevBuf<float> aq, adist;
    DevBuf<uint32_t> al32, acnt, astats;
    DevBuf<uint64_t> al64;
    DevBuf<uint32_t> afoq;              // hs_search_batch_filter_set: the per-query filter indices of the call in flight
    DevBuf<uint8_t> xruns;              // hs_index_exact_search: the sorted runs between the scan and the merge
    DevBuf<uint32_t> xorder;            // hs_index_exact_search (host entry): the queries grouped by filter
  };
  std::map<hipStream_t, std::unique_ptr<StreamWs>> ws;
  std::mutex ws_mu;
  StreamWs *stream_ws(hipStream_t st) {
    std::lock_guard<std::mutex> g(ws_mu);
    auto &p = ws[st];
    if (!p) p.reset(new StreamWs());
    return p.get();
  }
  // host-pointer API staging (default stream)
  DevBuf<float> wq, wdist;
  DevBuf<uint32_t> wl32, wcnt, wstats, wrawsz;
  DevBuf<uint64_t> wl64;
  DevBuf<Pair> wraw;
  std::vector<uint64_t> host_labels;   // external labels by internal id
  std::vector<uint8_t> host_deleted;   // delete marks by internal id
  DevBuf<uint8_t> wexcl;               // deleted | !allowed of the current filtered call
  // HNSW-SlimQ (kind == HS_KIND_SLIMQ): RaBitQ records, rotated centroids, rotator flips; `vec` then holds the
  // dataset rows of hs_slimq_set_dataset()
  DevBuf<uint32_t> q_rec, q_ftile, q_uptile;
  DevBuf<float> q_cent;
  DevBuf<uint8_t> q_flips;
  DevSlimQ sq{};
  bool has_dataset = false;
  uint32_t *trace_ptr = nullptr;   // hs_slimq_trace only
  // the file image a SlimQ index was made resident from (codes, factors, blobs, labels; no fp32 rows): hs_slimq_index_save writes it
  std::unique_ptr<SlimQGraph> host_slimq;
  double resident_ms = 0.0, tile_kernel_ms = 0.0;   // slimq_make_resident: the whole call; its three tile kernels
  uint32_t trace_cap = 0;
};

// A filter set (hs_filter_set_*): nf bitmap rows over the n internal ids the index had when the set was created (filter_set.hip).
struct hs_filter_set {
  int device = 0;
  size_t n = 0, nf = 0, row_words = 0;
  DevBuf<uint32_t> bits;     // nf x row_words
  DevBuf<uint8_t> stage;     // hs_filter_set_write: bounded staging of the host bytes
  DevBuf<uint8_t> unpacked;  // hs_filter_set_read: one row as bytes
};
// What a search under a filter set hands down to the launch plan (null = no filter set).
struct FilterUse {
  const hs_filter_set *fs;
  const uint32_t *d_of_query;   // nq filter indices (device)
};

// The batched add takes no index with delete marks, on the device or on the host twin.
static constexpr const char *kBatchedAddMarksRefusal =
    "batched add refused: the index holds delete marks (the batched insertion has no deleted-element branches); use hs_index_add_points";

// ---- the refusals and small helpers more than one entry uses: one text, one definition (error reporting: capi_guard.hpp) ----------
#pragma GCC visibility push(hidden)
inline hs_status metric_ok(int metric) {
  return metric == HS_METRIC_L2 || metric == HS_METRIC_IP ? HS_OK : fail(HS_ERR_INVALID, "bad metric");
}
// search_path: the text of the entries that would search on the device (an index, brute force); the builders and converters use the short one
inline hs_status device_ok(int device, bool search_path) {
  if (hs_device_count() > device) return HS_OK;
  return fail(HS_ERR_DEVICE, search_path ? "no HIP device (this library has no CPU search path)" : "no HIP device");
}
// addPoint's label refusals for new points, on a file (hs_hnsw_resume*) and on a resident index (hs_index_add_points*): a label the
// graph holds (has_label), a label twice in the call
template <class HasLabel>
hs_status labels_new_ok(HasLabel &&has_label, const uint64_t *labels, size_t count) {
  std::unordered_map<uint64_t, size_t> seen;
  seen.reserve(count);
  for (size_t i = 0; i < count; i++) {
    if (has_label(labels[i]))
      return fail(HS_ERR_UNSUPPORTED, "label " + std::to_string(labels[i]) + " (row " + std::to_string(i) + ") already exists: updatePoint is not supported");
    auto ins = seen.emplace(labels[i], i);
    if (!ins.second)
      return fail(HS_ERR_INVALID, "label " + std::to_string(labels[i]) + " appears twice in the call (rows " + std::to_string(ins.first->second) + " and " + std::to_string(i) + ")");
  }
  return HS_OK;
}
inline SlimParams slim_params(int threshold_level, float top_degree_percent0, float top_degree_percent, size_t top_degree_M0, size_t low_degree_m0,
                              size_t top_degree_M, size_t low_degree_m) {
  SlimParams p;
  p.threshold_level = threshold_level;
  p.top_pct0 = top_degree_percent0; p.top_pct = top_degree_percent;
  p.top_M0 = top_degree_M0; p.low_m0 = low_degree_m0; p.top_M = top_degree_M; p.low_m = low_degree_m;
  return p;
}
inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The functions that cross files (shared between the library's own objects, not exported).
// capi_index.cpp
hs_status upload(hs_index *ix, const PackedIndex &p);
hs_status upload_small(hs_index *ix, const PackedIndex &p);
hs_status build_narrow(hs_index *ix, int fmt, DevBuf<uint8_t> &out);
// capi_resident.cpp
// The device side of a call that changed the host image (packed as `p`, without rows; row_of(i) reads row i of the image): `changed`
// are the nodes whose level-0 list, label or mark changed, `row_ids` those that also carry a row -- in any order, repeats allowed.
// One staging copy and one kernel, then the small structure arrays (upload_small); a list that outgrew the tile stride re-uploads
// the whole index.  src_vec (nullable): fp32 rows on the same device, indexed like the image -- the kernel copies the rows from
// there and none is uploaded.
hs_status write_changed(hs_index *ix, PackedIndex &p, const std::function<const float *(uint32_t)> &row_of, const std::vector<uint32_t> &changed,
                        const std::vector<uint32_t> &row_ids, const float *src_vec = nullptr);
// hs_info.device_bytes from the index's state: base_bytes, plus the narrow copy and less the absent fp32 array, both by row capacity
void refresh_device_bytes(hs_index *ix);
void set_delete_marks(hs_index *ix, size_t num_deleted, bool has_deleted);   // num_deleted_ and the flag the kernels and hs_info carry
size_t first_unfit(const float *x, size_t count, int fmt);   // first value not representable in the row format, `count` when none
std::string unfit_message(size_t row, size_t comp, float v, int fmt);
// capi_build.cpp: what every batched entry refuses in its options (null, a device below -1, scratch_ids, grow_div / batch_max)
hs_status batch_opts_ok(const hs_batch_build_opts *opts);
// capi_slimq.cpp
hs_status load_slimq(const BinSource &src, int metric, size_t dim, int device, hs_index **out);
// The one way a SlimQ index becomes resident: the packed graph uploaded, the record fields uploaded as they lie in `q`, records and
// fused tiles gathered by slimq_tiles.hip; the index keeps `q` as its host image.  hs_index_load of a SlimQ file ends here too.
hs_status slimq_make_resident(std::unique_ptr<SlimQGraph> q, int device, hs_index **out);
// hs_slimq_set_dataset with the rows `pitch` bytes apart (the rows of a graph image lie inside its elements)
hs_status slimq_set_dataset_pitched(hs_index *ix, const void *rows, size_t pitch, size_t n, size_t dim);
// capi_search.cpp
hs_status search_dev(hs_index *ix, const float *d_q, size_t nq, size_t k, int mode, uint32_t *l32, uint64_t *l64, float *dd,
                     uint32_t *cnt, uint32_t *stats, Pair *raw, uint32_t *rawsz, hipStream_t stream, const FilterUse *fu = nullptr);
hs_status search_async(hs_index *ix, const float *queries, size_t nq, size_t k, int mode, uint32_t *l32, uint64_t *l64, float *dd,
                       uint32_t *cnt, uint32_t *stats, hipStream_t st, const FilterUse *fu = nullptr);
#pragma GCC visibility pop
