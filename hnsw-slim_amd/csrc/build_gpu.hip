// build_gpu.hip -- batched addPoint on gfx950, for two builders: hnswlib's (the host twin is host_batch_build.hpp) and
// rabitqlib's, the graph HNSW-SlimQ converts from (host_rq_batch_build.hpp, GpuBuildInput::rq).  Device and twin write
// the same bytes.  Per batch, on one stream:
//   bg_search_kernel   one wavefront per new row: the upper-level descent, then per level the builder's beam (searchBaseLayer,
//                      hnswalg.h:229-322 / search_base_layer, hnsw.hpp:827-905: a candidate and a result heap maintained on one
//                      lane, heap_emul.hpp; an exact visited set; neighbours in adjacency order) and its selection heuristic.  It
//                      writes the row's own lists: no search of the batch can reach them, since no older node links to a row of
//                      the batch yet.  The visited set (a hash) and the candidate heap live in LDS; a row that outgrows its share
//                      is flagged, and the same kernel runs again over the flagged rows with a bitmap and a heap in device memory.
//   bg_rev_count / bg_scan / bg_rev_fill   the new edges grouped by (target, level), as cv_rev_* and cd_scan_kernel do.
//   bg_link_kernel     one wavefront per target list with incoming ids: the reverse-link step (mutuallyConnectNewElement,
//                      hnswalg.h:618-683 / hnsw.hpp:973-1010) for its incoming ids in ascending order -- append while there is
//                      room, otherwise the heuristic over {new id} + the list at maxM / maxM0, stored in pop order (what it does
//                      not overwrite stays, as in the builder's memory).
// The two kernels are one text each.  What the builders do differently is a compile-time flavour, BgHnswlib or BgRabitq (below):
// the distance function, the order of the two heaps, the selection heuristic's candidate order and what it leaves behind, the
// capacity of the link kernel's candidate arrays and whether a list that already names the new id is left alone.  Rows, levels,
// task decoding, the visited set, the flag-and-re-run protocol, the sort of the incoming ids and the keep loop (cv_prune,
// convert_common.hpp) are shared; so are bg_rev / bg_scan and each kernel's LDS layout, which kernel and host read from one struct.
// Every store is a vector store; nothing is read back between batches.
// The same batches continued on a resident index (gpu_batch_add): the rows are the index's own array, the lists are
// seeded from its host image, and between bg_scan and bg_link of every batch
//   bga_mark_kernel    marks the lists of the old nodes that have incoming ids; after the last batch bga_count / bga_scan /
//                      bga_scatter compact the marked lists in ascending order and bga_gather_kernel packs their slots and the
//                      new nodes' slots into one dense buffer: what changed comes back, not everything.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "build_engine.hpp"
#include "convert_common.hpp"
#include "diff_prune.hpp"
#include "rq_dist.hpp"

namespace hs {

static constexpr uint32_t kBgPad = 0xFFFFFFFFu;    // id of a padding entry of the bitonic sort; the empty slot of the visited hash
static constexpr uint32_t kBgRerunGrid = 128;      // workgroups (and scratch areas) of the re-run pass
static constexpr uint32_t kBgLdsLimit = 160 * 1024;

struct BgDev {
  const float *vec;
  uint32_t *l0, *lu;             // level-0 lists (s0 words each), upper lists (su words each)
  const uint32_t *upb, *lev;     // per node: first upper slot, level
  uint32_t n, dim, dpad, M, maxM, maxM0, s0, su, efc, topcap;
};

__device__ __forceinline__ uint32_t *bg_list(const BgDev &g, uint32_t u, uint32_t level) {
  return level == 0 ? g.l0 + (size_t)u * g.s0 : g.lu + ((size_t)g.upb[u] + level - 1) * g.su;
}
__device__ __forceinline__ uint32_t bg_task(const BgDev &g, uint32_t u, uint32_t level) { return cv_task_of(u, level, g.n, g.upb); }

// ascending sort of arr[0..N) (N a power of two, padding entries behind every candidate); BEFORE()(a, b): a comes before b
template <class BEFORE>
__device__ __forceinline__ void bg_sort_pairs(Pair *arr, uint32_t N, int lane) {
  for (uint32_t k = 2; k <= N; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = lane; i < N; i += 64) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const Pair a = arr[i], b = arr[p];
          const bool a_after_b = b.id != kBgPad && (a.id == kBgPad || BEFORE()(b, a));
          const bool up = (i & k) == 0;
          if (a_after_b == up) { arr[i] = b; arr[p] = a; }
        }
      }
      wave_sync();
    }
}
// the result heap topq[0..topn) as the heuristic's candidates: padded to a power of two, sorted
template <class BEFORE>
__device__ __forceinline__ void bg_sort_top(Pair *topq, uint32_t topn, int lane) {
  uint32_t N = 64;
  while (N < topn) N <<= 1;
  for (uint32_t i = topn + lane; i < N; i += 64) topq[i] = Pair{0.f, kBgPad};
  wave_sync();
  bg_sort_pairs<BEFORE>(topq, N, lane);
}

// ---- the two flavours ------------------------------------------------------------------------------------------------------------------
// A flavour is a type of static members, resolved when a kernel is instantiated:
//   dists              the builder's distance: query row (LDS) -> rows nid[0..cnt) into nd[0..cnt); also cv_prune's
//   TopCmp, CandCmp    the orders of the result heap and the candidate heap; cand_key(d): what the candidate heap stores for a
//                      distance d, and the distance for what it stores
//   select             the selection heuristic over the result heap topq[0..topn) -> how many it selected
//   rank_sort          the link kernel's candidates (nd[j], nid[j]), j < sz, into arr[] in the heuristic's candidate order
//   pop_order          after the keep loop (kept / keptd[0..kc) in kept order): whatever it takes before selected() can be read
//   selected, entry    selected(arr, kept, i): the selected ids in the reverse of the builder's pop order, i = kc - 1 the first one
//                      popped; entry: the last one popped, the next level's entry point
//   kKeptD             the keep loop records the kept distances (an LDS array of its own)
//   kLinkCap           entries of the link kernel's arr / nid / nd: {new id} + a full list
//   kSkipNamed         the link step leaves a list alone that already names the new id
struct H2Before { __device__ __forceinline__ bool operator()(const Pair &a, const Pair &b) const { return h2_before(a, b); } };

// hnswlib (hnswalg.h): both heaps compare distances only (CompareByFirst), so libstdc++'s push / pop mechanics decide among equal
// distances; the candidate heap holds negated distances.  getNeighborsByHeuristic2 (:481-523) does nothing below M entries;
// otherwise the candidates by (distance ascending, id descending), the keep loop, the kept entries re-emplaced and popped
// (diff_prune.hpp).  sz <= 63 link candidates (kBgMaxM), one per lane.
struct BgHnswlib {
  static constexpr bool kKeptD = true, kSkipNamed = false;
  static constexpr uint32_t kLinkCap = 64;
  using TopCmp = LessD;
  using CandCmp = LessD;
  static __device__ __forceinline__ float cand_key(float d) { return -d; }
  template <int METRIC>
  static __device__ __forceinline__ void dists(const float *vec, uint32_t dim, const float *qv, const uint32_t *nid, float *nd, uint32_t cnt, int lane) {
    cv_dists<METRIC>(vec, dim, qv, nid, nd, cnt, lane);
  }
  static __device__ __forceinline__ void pop_order(Pair *arr, const uint32_t *kept, const float *keptd, uint32_t kc, int lane) {
    wave_sync();
    if ((uint32_t)lane < kc) arr[lane] = Pair{keptd[lane], kept[lane]};
    wave_sync();
    if (lane == 0) h2_pop_order(arr, (long)kc);
  }
  static __device__ __forceinline__ uint32_t selected(const Pair *arr, const uint32_t *kept, uint32_t i) { return arr[i].id; }
  static __device__ __forceinline__ uint32_t entry(const Pair *arr, const uint32_t *kept) { return arr[0].id; }   // sel.back()
  template <int METRIC>
  static __device__ __forceinline__ uint32_t select(const BgDev &g, Pair *topq, uint32_t topn, float *qc, uint32_t *kept, float *keptd, float *kd, int lane) {
    if (topn < g.M) {   // the pop order connect() reads, nothing else
      if (lane == 0)
        for (long m = topn; m > 1; m--) pop_heap(topq, m, LessD());
      return topn;
    }
    bg_sort_top<H2Before>(topq, topn, lane);
    const uint32_t kc = cv_prune<METRIC, BgHnswlib>(g.vec, g.dim, topq, topn, g.M, qc, kept, kd, lane, keptd);
    pop_order(topq, kept, keptd, kc, lane);
    return kc;
  }
  static __device__ __forceinline__ void rank_sort(const uint32_t *nid, const float *nd, uint32_t sz, Pair *arr, int lane) {
    const bool act = (uint32_t)lane < sz;
    const Pair mine{act ? nd[lane] : 0.f, act ? nid[lane] : 0u};
    uint32_t rank = 0;
    for (uint32_t j = 0; j < sz; j++) rank += h2_before(Pair{nd[j], nid[j]}, mine) ? 1u : 0u;
    if (act) arr[rank] = mine;
  }
};

// rabitqlib (hnsw.hpp; RqGraph, host_rq_graph.hpp), at M up to 32: every distance is rq_dists (rq_dist.hpp); both heaps order
// (distance, id) pairs (:33-36) -- a total order, so libstdc++'s heap mechanics decide nothing and any correct heap or sort serves.
// get_neighbors_by_heuristic2 (:1016-1054) takes its candidates by ascending pair, keeps everything below M entries, and what it
// keeps leaves the max-heap in descending pair order (:917-922), i.e. kept[] reversed.  A full level-0 list at M = 32 plus the new
// id is 65 link candidates: the rank sort takes two per lane; the keep loop keeps at most 64, one lane per kept entry.
__device__ __forceinline__ bool rq_less(const Pair &a, const Pair &b) { return a.d < b.d || (a.d == b.d && a.id < b.id); }
struct RqLess { __device__ __forceinline__ bool operator()(const Pair &a, const Pair &b) const { return rq_less(a, b); } };      // maxheap
struct RqGreater { __device__ __forceinline__ bool operator()(const Pair &a, const Pair &b) const { return rq_less(b, a); } };   // minheap
struct BgRabitq {
  static constexpr bool kKeptD = false, kSkipNamed = true;   // (hnsw.hpp:973-980)
  static constexpr uint32_t kLinkCap = 128;
  using TopCmp = RqLess;
  using CandCmp = RqGreater;
  static __device__ __forceinline__ float cand_key(float d) { return d; }
  template <int METRIC>
  static __device__ __forceinline__ void dists(const float *vec, uint32_t dim, const float *qv, const uint32_t *nid, float *nd, uint32_t cnt, int lane) {
    rq_dists<METRIC>(vec, dim, qv, nid, nd, cnt, lane);
  }
  static __device__ __forceinline__ void pop_order(Pair *, const uint32_t *, const float *, uint32_t, int) {}
  static __device__ __forceinline__ uint32_t selected(const Pair *arr, const uint32_t *kept, uint32_t i) { return kept[i]; }
  static __device__ __forceinline__ uint32_t entry(const Pair *arr, const uint32_t *kept) { return uni(kept[0]); }   // sel.back()
  template <int METRIC>
  static __device__ __forceinline__ uint32_t select(const BgDev &g, Pair *topq, uint32_t topn, float *qc, uint32_t *kept, float *keptd, float *kd, int lane) {
    bg_sort_top<RqLess>(topq, topn, lane);
    if (topn >= g.M) return cv_prune<METRIC, BgRabitq>(g.vec, g.dim, topq, topn, g.M, qc, kept, kd, lane);
    if ((uint32_t)lane < topn) kept[lane] = topq[lane].id;
    return topn;
  }
  static __device__ __forceinline__ void rank_sort(const uint32_t *nid, const float *nd, uint32_t sz, Pair *arr, int lane) {
    for (uint32_t x = lane; x < sz; x += 64) {   // equal pairs (a damaged list) by their place
      const Pair mine{nd[x], nid[x]};
      uint32_t rank = 0;
      for (uint32_t j = 0; j < sz; j++) {
        const Pair o{nd[j], nid[j]};
        rank += (rq_less(o, mine) || (!rq_less(mine, o) && j < x)) ? 1u : 0u;
      }
      arr[rank] = mine;
    }
  }
};

// ---- LDS layouts: where every array of a kernel starts, in order; the kernel takes its pointers and the host its byte count from
//      the same object.  A, the address type: unsigned char * in a kernel (base: the start of its LDS, so the members are the arrays
//      themselves), size_t on the host (base 0: byte offsets) -------------------------------------------------------------------------
__host__ __device__ constexpr uint32_t bg_topcap(uint32_t efc) {
  uint32_t c = 64;
  while (c < efc + 1) c <<= 1;
  return c;
}
// the search kernel: two rows, the result heap, 64 entries each of nid / nd / kept / (keptd) / kd; ONCHIP (scratch_ids != 0) the
// visited hash of 2 * scratch_ids slots and scratch_ids / 2 candidate pairs
template <class F, class A>
struct BgSearchLds {
  A qv, qc, topq, nid, nd, kept, keptd, kd, hash, cand, end;
  __host__ __device__ constexpr BgSearchLds(A base, uint32_t dpad, uint32_t topcap, uint32_t scratch_ids)
      : qv(base), qc(qv + (size_t)dpad * sizeof(float)), topq(qc + (size_t)dpad * sizeof(float)), nid(topq + (size_t)topcap * sizeof(Pair)),
        nd(nid + 64 * sizeof(uint32_t)), kept(nd + 64 * sizeof(float)), keptd(kept + 64 * sizeof(uint32_t)),
        kd(keptd + (F::kKeptD ? 64 * sizeof(float) : 0)), hash(kd + 64 * sizeof(float)), cand(hash + 2 * (size_t)scratch_ids * sizeof(uint32_t)),
        end(cand + (size_t)scratch_ids / 2 * sizeof(Pair)) {}
};
// the link kernel: two rows, kLinkCap entries each of arr / nid / nd, 64 each of kept / (keptd) / kd / curl / inc
template <class F, class A>
struct BgLinkLds {
  A qv, qc, arr, nid, nd, kept, keptd, kd, curl, inc, end;
  __host__ __device__ constexpr BgLinkLds(A base, uint32_t dpad)
      : qv(base), qc(qv + (size_t)dpad * sizeof(float)), arr(qc + (size_t)dpad * sizeof(float)), nid(arr + F::kLinkCap * sizeof(Pair)),
        nd(nid + F::kLinkCap * sizeof(uint32_t)), kept(nd + F::kLinkCap * sizeof(float)), keptd(kept + 64 * sizeof(uint32_t)),
        kd(keptd + (F::kKeptD ? 64 * sizeof(float) : 0)), curl(kd + 64 * sizeof(float)), inc(curl + 64 * sizeof(uint32_t)),
        end(inc + 64 * sizeof(uint32_t)) {}
};
template <class F>
constexpr size_t bg_search_lds(uint32_t dpad, uint32_t efc, uint32_t scratch_ids) { return BgSearchLds<F, size_t>(0, dpad, bg_topcap(efc), scratch_ids).end; }
template <class F>
constexpr size_t bg_link_lds(uint32_t dpad) { return BgLinkLds<F, size_t>(0, dpad).end; }
template <class T>
__device__ __forceinline__ T *bg_lds(unsigned char *at) { return reinterpret_cast<T *>(at); }

// The byte counts at four (dim, ef_construction, scratch_ids) points, as the numbers the hand-written sums gave before the layouts
// existed (gpu_build_supported / gpu_rq_build_supported decide by them).
template <class F>
constexpr bool bg_lds_is(uint32_t dim, uint32_t efc, uint32_t scratch_ids, size_t search, size_t link) {
  return bg_search_lds<F>(dim, efc, scratch_ids) == search && bg_link_lds<F>(dim) == link;
}
static_assert(bg_lds_is<BgHnswlib>(16, 10, 64, 2688, 2432) && bg_lds_is<BgRabitq>(16, 10, 64, 2432, 3200), "LDS layout");
static_assert(bg_lds_is<BgHnswlib>(128, 200, 4096, 53504, 3328) && bg_lds_is<BgRabitq>(128, 200, 4096, 53248, 4096), "LDS layout");
static_assert(bg_lds_is<BgHnswlib>(768, 128, 4096, 58624, 8448) && bg_lds_is<BgRabitq>(768, 128, 4096, 58368, 9216), "LDS layout");
static_assert(bg_lds_is<BgHnswlib>(960, 512, 8192, 115456, 9984) && bg_lds_is<BgRabitq>(960, 512, 8192, 115200, 10752), "LDS layout");

// ---- phase A ------------------------------------------------------------------------------------------------------------------------
// ONCHIP: grid = the rows of the batch.  Otherwise: the flagged rows, kBgRerunGrid workgroups, scratch area `blockIdx.x` of gscratch
// ((n + 31) / 32 bitmap words, then n candidate pairs).  ctr[0]: flagged rows of this batch, ctr[1]: of the build.
template <class F, int METRIC, bool ONCHIP>
__global__ void __launch_bounds__(64) bg_search_kernel(BgDev g, uint32_t begin, uint32_t count, uint32_t ep, int32_t top, uint32_t scratch_ids,
                                                       uint32_t *flagged, uint32_t *ctr, uint32_t *gscratch, size_t gstride) {
  extern __shared__ __align__(16) unsigned char smem[];
  const BgSearchLds<F, unsigned char *> lds(smem, g.dpad, g.topcap, scratch_ids);
  float *qv = bg_lds<float>(lds.qv);
  float *qc = bg_lds<float>(lds.qc);
  Pair *topq = bg_lds<Pair>(lds.topq);
  uint32_t *nid = bg_lds<uint32_t>(lds.nid);
  float *nd = bg_lds<float>(lds.nd);
  uint32_t *kept = bg_lds<uint32_t>(lds.kept);
  float *keptd = F::kKeptD ? bg_lds<float>(lds.keptd) : nullptr;
  float *kd = bg_lds<float>(lds.kd);
  uint32_t *hash = bg_lds<uint32_t>(lds.hash);                            // ONCHIP
  const uint32_t hmask = 2 * scratch_ids - 1;
  uint32_t *bitmap = gscratch + (size_t)blockIdx.x * gstride;                   // !ONCHIP
  Pair *cand = ONCHIP ? bg_lds<Pair>(lds.cand) : reinterpret_cast<Pair *>(bitmap + (((size_t)g.n + 31) / 32 + 1) / 2 * 2);
  const uint32_t candcap = ONCHIP ? scratch_ids / 2 : g.n;
  const int lane = threadIdx.x;
  const uint32_t nrows = ONCHIP ? count : min(ctr[0], count);
  for (uint32_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    const uint32_t p = ONCHIP ? begin + r : flagged[r];
    if (p < begin || p >= begin + count) continue;
    const uint32_t lp = g.lev[p];
    wave_sync();
    for (uint32_t i = lane; i < g.dim; i += 64) qv[i] = g.vec[(size_t)p * g.dim + i];
    uint32_t cur = ep;
    wave_sync();
    if ((int32_t)lp < top) {   // the greedy walk of the upper levels (hnswalg.h:1300-1326 / hnsw.hpp:733-760)
      if (lane == 0) nid[0] = cur;
      wave_sync();
      F::template dists<METRIC>(g.vec, g.dim, qv, nid, nd, 1, lane);
      wave_sync();
      float curdist = nd[0];
      for (int32_t level = top; level > (int32_t)lp; level--) {
        bool changed = true;
        while (changed) {
          changed = false;
          const uint32_t *l = bg_list(g, cur, (uint32_t)level);
          const uint32_t cnt = min(uni(l[0]) & 0xFFFFu, g.maxM);
          wave_sync();
          if ((uint32_t)lane < cnt) nid[lane] = min(l[1 + lane], begin - 1);
          wave_sync();
          F::template dists<METRIC>(g.vec, g.dim, qv, nid, nd, cnt, lane);
          wave_sync();
          for (uint32_t i = 0; i < cnt; i++) {   // every lane the same walk over LDS
            const float d = nd[i];
            if (d < curdist) { curdist = d; cur = nid[i]; changed = true; }
          }
          cur = uni(cur);
          curdist = unif(curdist);
          changed = hs_ballot(changed) != 0;
        }
      }
    }
    bool ok = true;
    for (int32_t level = min((int32_t)lp, top); level >= 0 && ok; level--) {
      // ---- the beam ---------------------------------------------------------------------------------------------------------
      wave_sync();
      if (ONCHIP) for (uint32_t i = lane; i <= hmask; i += 64) hash[i] = kBgPad;
      else for (uint32_t i = lane; i < (begin + 31) / 32; i += 64) bitmap[i] = 0;
      if (lane == 0) nid[0] = cur;
      if (!ONCHIP) __syncthreads();   // (one wavefront per workgroup: orders the bitmap's plain stores before its atomics)
      wave_sync();
      F::template dists<METRIC>(g.vec, g.dim, qv, nid, nd, 1, lane);
      wave_sync();
      uint32_t topn = 1, candn = 1, nvis = 1;
      float lower = nd[0];
      if (lane == 0) {
        topq[0] = Pair{lower, cur};
        cand[0] = Pair{F::cand_key(lower), cur};
        if (ONCHIP) hash[(cur * 2654435761u) & hmask] = cur;
        else bitmap[cur >> 5] = 1u << (cur & 31);
      }
      if (!ONCHIP) __syncthreads();
      wave_sync();
      while (candn > 0) {
        Pair c{0.f, 0u};
        if (lane == 0) c = cand[0];   // (the lane that maintains the heap reads it: program order, whichever memory holds it)
        const uint32_t node = uni(c.id);
        if (F::cand_key(unif(c.d)) > lower && topn == g.efc) break;
        if (lane == 0) pop_heap(cand, (long)candn, typename F::CandCmp());
        candn--;
        const uint32_t lim = level ? g.maxM : g.maxM0;
        const uint32_t *l = bg_list(g, node, (uint32_t)level);
        const uint32_t cnt = min(uni(l[0]) & 0xFFFFu, lim);
        const uint32_t id = (uint32_t)lane < cnt ? l[1 + lane] : kBgPad;
        bool isnew = false;
        if (id < begin) {   // (every id of the graph so far is; the test keeps a damaged list inside the arrays)
          if (ONCHIP) {
            uint32_t slot = (id * 2654435761u) & hmask;
            while (true) {   // at most scratch_ids + 64 <= 2 * scratch_ids - 1 ids are ever in the table: an empty slot exists
              const uint32_t old = lds_cas(&hash[slot], kBgPad, id);
              if (old == kBgPad) { isnew = true; break; }
              if (old == id) break;
              slot = (slot + 1) & hmask;
            }
          } else {
            const uint32_t bit = 1u << (id & 31);
            isnew = (atomicOr(&bitmap[id >> 5], bit) & bit) == 0;
          }
        }
        const unsigned long long nm = hs_ballot(isnew);
        const uint32_t nnew = __popcll(nm);
        wave_sync();
        if (isnew) nid[__popcll(nm & ((1ull << lane) - 1ull))] = id;   // adjacency order
        nvis += nnew;
        if (ONCHIP && nvis > scratch_ids) { ok = false; break; }
        wave_sync();
        F::template dists<METRIC>(g.vec, g.dim, qv, nid, nd, nnew, lane);
        wave_sync();
        uint32_t ovf = 0;
        if (lane == 0) {
          for (uint32_t j = 0; j < nnew; j++) {
            const float d = nd[j];
            if (topn < g.efc || lower > d) {
              if (candn >= candcap) { ovf = 1; break; }
              cand[candn++] = Pair{F::cand_key(d), nid[j]};
              push_heap(cand, (long)candn, typename F::CandCmp());
              topq[topn++] = Pair{d, nid[j]};
              push_heap(topq, (long)topn, typename F::TopCmp());
              if (topn > g.efc) { pop_heap(topq, (long)topn, typename F::TopCmp()); topn--; }
              lower = topq[0].d;
            }
          }
        }
        topn = uni(topn); candn = uni(candn); lower = unif(lower); ovf = uni(ovf);
        wave_sync();
        if (ovf) { ok = false; break; }
      }
      if (!ok) break;
      // ---- the heuristic over the result heap at M, then the row's list in the builder's pop order ----------------------------------
      const uint32_t kc = F::template select<METRIC>(g, topq, topn, qc, kept, keptd, kd, lane);
      wave_sync();
      uint32_t *own = bg_list(g, p, (uint32_t)level);
      if ((uint32_t)lane < kc) own[1 + lane] = F::selected(topq, kept, kc - 1 - lane);
      if (lane == 0) own[0] = kc;
      cur = F::entry(topq, kept);
    }
    if (!ok && ONCHIP && lane == 0) {
      flagged[atomicAdd(&ctr[0], 1u)] = p;
      atomicAdd(&ctr[1], 1u);
    }
  }
}

// ---- reverse edges by (target, level) ----------------------------------------------------------------------------------------------
// one wavefront per row of the batch; FILL: rev[roff[task] + rank] = the row, any rank (the link kernel sorts its segment)
template <bool FILL>
__global__ void __launch_bounds__(256) bg_rev_kernel(BgDev g, uint32_t begin, uint32_t count, int32_t top, uint32_t *rcnt, const uint32_t *roff,
                                                     uint32_t *rcur, uint32_t *rev, uint32_t rev_cap) {
  const uint32_t lane = threadIdx.x & 63u, r = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (r >= count) return;
  const uint32_t p = begin + r;
  const int32_t l0 = min((int32_t)g.lev[p], top);
  for (int32_t level = 0; level <= l0; level++) {
    const uint32_t *own = bg_list(g, p, (uint32_t)level);
    const uint32_t cnt = min(own[0] & 0xFFFFu, g.M);
    if (lane < cnt) {
      const uint32_t t = own[1 + lane];
      if (t < begin && g.lev[t] >= (uint32_t)level) {
        const uint32_t task = bg_task(g, t, (uint32_t)level);
        if (!FILL) atomicAdd(&rcnt[task], 1u);
        else {
          const uint32_t at = roff[task] + atomicAdd(&rcur[task], 1u);
          if (at < rev_cap) rev[at] = p;
        }
      }
    }
  }
}

// active task i -> task: the level-0 lists of the nodes below `begin`, then their upper lists
__device__ __forceinline__ uint32_t bg_active(uint32_t i, uint32_t begin, uint32_t n) { return i < begin ? i : n + (i - begin); }

// exclusive scan over the 256 threads of the workgroup: the sum of the threads before this one; thread 0 hands the sum of all to `total`
template <class TOTAL>
__device__ __forceinline__ uint32_t bg_scan256(uint32_t sum, TOTAL total) {
  __shared__ uint32_t part[256];
  const uint32_t t = threadIdx.x;
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (uint32_t j = 0; j < 256; j++) { const uint32_t c = part[j]; part[j] = run; run += c; }
    total(run);
  }
  __syncthreads();
  return part[t];
}

// exclusive prefix sums of rcnt over the active tasks (one workgroup, as cd_scan_kernel)
__global__ void __launch_bounds__(256) bg_scan_kernel(const uint32_t *rcnt, uint32_t *roff, uint32_t begin, uint32_t n, uint32_t nact) {
  const uint32_t t = threadIdx.x, per = (nact + 255u) / 256u, lo = min(nact, t * per), hi = min(nact, lo + per);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; i++) sum += rcnt[bg_active(i, begin, n)];
  sum = bg_scan256(sum, [](uint32_t) {});
  for (uint32_t i = lo; i < hi; i++) { const uint32_t a = bg_active(i, begin, n); roff[a] = sum; sum += rcnt[a]; }
}

// ---- phase B: the reverse links ------------------------------------------------------------------------------------------------------
// up_node / up_level: node and level of upper slot j (task n + j)
template <class F, int METRIC>
__global__ void __launch_bounds__(64) bg_link_kernel(BgDev g, uint32_t begin, uint32_t nact, const uint32_t *up_node, const uint32_t *up_level,
                                                     uint32_t *rcnt, const uint32_t *roff, uint32_t *rcur, uint32_t *rev, uint32_t rev_cap) {
  extern __shared__ __align__(16) unsigned char smem[];
  const BgLinkLds<F, unsigned char *> lds(smem, g.dpad);
  float *qv = bg_lds<float>(lds.qv);
  float *qc = bg_lds<float>(lds.qc);
  Pair *arr = bg_lds<Pair>(lds.arr);
  uint32_t *nid = bg_lds<uint32_t>(lds.nid);
  float *nd = bg_lds<float>(lds.nd);
  uint32_t *kept = bg_lds<uint32_t>(lds.kept);
  float *keptd = F::kKeptD ? bg_lds<float>(lds.keptd) : nullptr;
  float *kd = bg_lds<float>(lds.kd);
  uint32_t *curl = bg_lds<uint32_t>(lds.curl);
  uint32_t *inc = bg_lds<uint32_t>(lds.inc);
  const int lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < nact; i += gridDim.x) {
    const uint32_t task = bg_active(i, begin, g.n);
    const uint32_t k = uni(rcnt[task]);
    if (k == 0) continue;
    const uint32_t off = uni(roff[task]);
    if (off >= rev_cap || k > rev_cap - off) continue;   // (never: the host sizes rev for every edge of the batch)
    const uint32_t u = task < g.n ? task : up_node[task - g.n], level = task < g.n ? 0u : up_level[task - g.n];
    const uint32_t lim = level ? g.maxM : g.maxM0;   // <= 64
    uint32_t *seg = rev + off;
    wave_sync();
    if (k <= 64) {   // the incoming ids in ascending order: distinct, so the rank of each is its place
      const uint32_t mine = (uint32_t)lane < k ? seg[lane] : kBgPad;
      if ((uint32_t)lane < k) inc[lane] = mine;
      wave_sync();
      uint32_t rank = 0;
      for (uint32_t j = 0; j < k; j++) rank += inc[j] < mine ? 1u : 0u;
      wave_sync();
      if ((uint32_t)lane < k) inc[rank] = mine;
    } else {   // bitonic network whose exchanges all put the smaller id first: the places beyond k count as +inf and never move
      uint32_t N = 128;
      while (N < k) N <<= 1;
      for (uint32_t kk = 2; kk <= N; kk <<= 1) {
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
          const bool flip = j == (kk >> 1);
          __syncthreads();   // (one wavefront per workgroup; uniform: orders the segment's stores before the next step's loads)
          for (uint32_t x = lane; x < N; x += 64) {
            const uint32_t y = flip ? (x ^ (kk - 1)) : (x ^ j);
            if (y > x && y < k) {
              const uint32_t a = seg[x], b = seg[y];
              if (a > b) { seg[x] = b; seg[y] = a; }
            }
          }
        }
      }
      __syncthreads();
    }
    uint32_t *lst = bg_list(g, u, level);
    uint32_t cnt = min(uni(lst[0]) & 0xFFFFu, lim);
    if ((uint32_t)lane < lim) curl[lane] = lst[1 + lane];
    bool have_row = false;
    wave_sync();
    for (uint32_t e = 0; e < k; e++) {
      const uint32_t p = k <= 64 ? inc[e] : uni(seg[e]);
      if (F::kSkipNamed && hs_ballot((uint32_t)lane < cnt && curl[lane] == p) != 0) continue;
      if (cnt < lim) {
        if (lane == 0) curl[cnt] = p;
        cnt++;
        wave_sync();
        continue;
      }
      if (!have_row) {
        for (uint32_t c = lane; c < g.dim; c += 64) qv[c] = g.vec[(size_t)u * g.dim + c];
        have_row = true;
      }
      const uint32_t sz = cnt + 1;   // < kLinkCap: {p} + the full list
      if (lane == 0) nid[0] = p;
      if ((uint32_t)lane < cnt) nid[1 + lane] = curl[lane];
      wave_sync();
      F::template dists<METRIC>(g.vec, g.dim, qv, nid, nd, sz, lane);
      wave_sync();
      F::rank_sort(nid, nd, sz, arr, lane);
      wave_sync();
      const uint32_t kc = cv_prune<METRIC, F>(g.vec, g.dim, arr, sz, lim, qc, kept, kd, lane, keptd);
      F::pop_order(arr, kept, keptd, kc, lane);
      wave_sync();
      if ((uint32_t)lane < kc) curl[lane] = F::selected(arr, kept, kc - 1 - lane);   // pop order; what it does not overwrite stays
      cnt = kc;
      wave_sync();
    }
    if ((uint32_t)lane < lim) lst[1 + lane] = curl[lane];
    if (lane == 0) { lst[0] = cnt; rcnt[task] = 0; rcur[task] = 0; }
  }
}

// hs_debug_rq_raw_dist: pair i is a[i] against b[i]; the row is measured five times in one call of rq_dists, so that pairs land in
// every sixteen-lane group and in the second pass.
template <int METRIC>
__global__ void __launch_bounds__(64) rq_dist_debug_kernel(const float *a, const float *b, uint32_t n_pairs, uint32_t dim, uint32_t dpad, float *out) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  uint32_t *nid = reinterpret_cast<uint32_t *>(qv + dpad);
  float *nd = reinterpret_cast<float *>(nid + 8);
  const int lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < n_pairs; i += gridDim.x) {
    wave_sync();
    for (uint32_t c = lane; c < dim; c += 64) qv[c] = a[(size_t)i * dim + c];
    if (lane < 5) nid[lane] = i;
    wave_sync();
    rq_dists<METRIC>(b, dim, qv, nid, nd, 5, lane);
    wave_sync();
    if (lane == 0) out[i] = nd[i % 5u];
  }
}

// ---- the add into a resident index: which lists of the old nodes changed, and only those come back ------------------------
// An old task is a list the graph held before the call: the level-0 lists of the n0 old nodes, then their nup0 upper slots.
struct BgMarks {
  uint8_t *mark;   // n0 + nup0 bytes, zeroed before the first batch
  uint32_t n0, nup0;
};
// Per batch, between the scan and the link kernel: every old task with incoming ids is marked.
__global__ void __launch_bounds__(256) bga_mark_kernel(const uint32_t *rcnt, uint32_t begin, uint32_t n, uint32_t nact, BgMarks m) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nact; i += gridDim.x * 256u) {
    const uint32_t task = bg_active(i, begin, n);
    if (rcnt[task] == 0) continue;
    if (task < m.n0) m.mark[task] = 1;
    else if (task >= n && task - n < m.nup0) m.mark[m.n0 + (task - n)] = 1;
  }
}
// Compaction in ascending order, as cd_count / cd_scan / cd_scatter (convert_diff.hip): one wavefront per 64 consecutive old tasks
// counts its marks, one workgroup turns the counts into offsets, the wavefronts write their tasks at their rank in the ballot.
__global__ void __launch_bounds__(256) bga_count_kernel(const uint8_t *mark, uint32_t nold, uint32_t *counts) {
  const uint32_t lane = threadIdx.x & 63u, w = blockIdx.x * 4u + (threadIdx.x >> 6), i = w * 64u + lane;
  if (w * 64u >= nold) return;
  const uint32_t c = __popcll(hs_ballot(i < nold && mark[i] != 0));
  if (lane == 0) counts[w] = c;
}
__global__ void __launch_bounds__(256) bga_scan_kernel(uint32_t *counts, uint32_t nw, uint32_t *total) {
  const uint32_t t = threadIdx.x, per = (nw + 255u) / 256u, lo = min(nw, t * per), hi = min(nw, lo + per);
  uint32_t sum = 0;
  for (uint32_t w = lo; w < hi; w++) sum += counts[w];
  sum = bg_scan256(sum, [=](uint32_t all) { *total = all; });
  for (uint32_t w = lo; w < hi; w++) { const uint32_t c = counts[w]; counts[w] = sum; sum += c; }
}
__global__ void __launch_bounds__(256) bga_scatter_kernel(const uint8_t *mark, uint32_t nold, uint32_t n0, uint32_t n, const uint32_t *offs, uint32_t *ids) {
  const uint32_t lane = threadIdx.x & 63u, w = blockIdx.x * 4u + (threadIdx.x >> 6), i = w * 64u + lane;
  if (w * 64u >= nold) return;
  const bool m = i < nold && mark[i] != 0;
  const unsigned long long bm = hs_ballot(m);
  const uint32_t at = offs[w] + __popcll(bm & ((1ull << lane) - 1ull));
  if (m && at < nold) ids[at] = i < n0 ? i : n + (i - n0);
}
// One wavefront per entry of the dense buffer: entry j < nchg is the slot of task ids[j]; then the level-0 slots of the new nodes
// n0 .. n - 1; then their upper slots nup0 .. nup - 1.  Lane i moves word i: consecutive lanes, consecutive words on both sides (a slot
// starts at a multiple of maxM0 + 1 or maxM + 1 words -- 4-byte alignment is all a slot has, so the words move one by one).  The task
// ids follow the nslots entries.
__global__ void __launch_bounds__(256) bga_gather_kernel(BgDev g, const uint32_t *ids, uint32_t nchg, uint32_t n0, uint32_t nup0, uint32_t nup,
                                                         uint32_t nslots, uint32_t *out) {
  const uint32_t lane = threadIdx.x & 63u, j = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (j >= nslots) return;
  const uint32_t nnew = g.n - n0;
  const uint32_t task = j < nchg ? ids[j] : (j - nchg < nnew ? n0 + (j - nchg) : g.n + nup0 + (j - nchg - nnew));
  if (task >= g.n + nup) return;   // (never: the host counts the entries)
  const uint32_t *src = task < g.n ? g.l0 + (size_t)task * g.s0 : g.lu + (size_t)(task - g.n) * g.su;
  const uint32_t words = task < g.n ? g.s0 : g.su;
  if (lane < g.s0) out[(size_t)j * g.s0 + lane] = lane < words ? src[lane] : 0u;
  if (lane == 0 && j < nchg) out[(size_t)nslots * g.s0 + j] = task;
}

// ---- host driver ------------------------------------------------------------------------------------------------------------------
// efc: max(ef_construction, M); scratch_ids: 0 for the default
template <class F>
static bool bg_shape_ok(uint32_t dim, uint32_t efc, uint32_t scratch_ids) {
  if (scratch_ids == 0) scratch_ids = kBgScratchIds;
  if (efc > kBgMaxEfc || dim == 0) return false;
  if (scratch_ids < 64 || (scratch_ids & (scratch_ids - 1)) != 0 || scratch_ids > 8192) return false;
  const uint32_t dpad = (dim + 3u) & ~3u;
  return bg_search_lds<F>(dpad, efc, scratch_ids) <= kBgLdsLimit && bg_link_lds<F>(dpad) <= kBgLdsLimit;
}
bool gpu_build_supported(uint32_t dim, uint32_t M, uint32_t efc, uint32_t scratch_ids) {
  return M != 0 && M <= kBgMaxM && bg_shape_ok<BgHnswlib>(dim, std::max(efc, M), scratch_ids);
}
bool gpu_rq_build_supported(uint32_t dim, uint32_t M, uint32_t efc, uint32_t scratch_ids) {
  return M >= 2 && M <= kRqMaxM && bg_shape_ok<BgRabitq>(dim, std::max(efc, M), scratch_ids);
}

#define BG_TRY(expr)                      \
  do {                                    \
    const hipError_t _e = (expr);         \
    if (_e != hipSuccess) return _e;      \
  } while (0)

// a device allocation that ends with its owner, so that every return frees it
template <class T>
struct BgBuf {
  T *p = nullptr;
  BgBuf() = default;
  BgBuf(const BgBuf &) = delete;
  BgBuf &operator=(const BgBuf &) = delete;
  ~BgBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count) { return hipMalloc((void **)&p, count * sizeof(T)); }
  hipError_t zero(size_t count) { return hipMemset(p, 0, count * sizeof(T)); }
  hipError_t upload(const T *src, size_t count) { return hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice); }
};

// What a run of batches works in, for a build and for an add: the lists and the per-node tables, the flags and scratch areas of the
// re-run pass, the reverse edges of one batch, the two events around the kernels.
struct BgWork {
  BgDev g{};                     // (vec is the caller's)
  uint32_t scratch_ids = 0;
  const uint32_t *h_upb = nullptr;   // the caller's n + 1 prefix sums of the levels
  BgBuf<uint32_t> l0, lu, upb, lev, upnode, uplevel, flagged, ctr, scratch, rcnt, roff, rcur, rev;
  size_t gstride = 0;            // words of one scratch area: bitmap (padded to a pair's alignment) + n pairs
  uint32_t rev_cap = 1;          // the most edges one batch can add: M per (row, level it is searched on)
  uint32_t max_batch = 1, nup = 0;
  std::vector<uint32_t> up_node, up_level;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~BgWork() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};
static constexpr size_t kBgCtrWords = 3;   // flagged rows of the batch, of the call; the add's changed old tasks

// shape: n, dim, M, maxM, maxM0, efc.  lists0 / lists_up: the host image the lists start from (an add), or null for empty lists.
static hipError_t bg_work_init(BgWork &w, const BgDev &shape, uint32_t scratch_ids, const uint32_t *lev, const std::vector<uint32_t> &upb,
                               const std::vector<BatchStep> &steps, const uint32_t *lists0, const uint32_t *lists_up) {
  BgDev &g = w.g;
  g = shape;
  g.dpad = (g.dim + 3u) & ~3u; g.s0 = g.maxM0 + 1; g.su = g.maxM + 1; g.topcap = bg_topcap(g.efc);
  const uint32_t n = g.n, nup = upb[n];
  w.scratch_ids = scratch_ids; w.h_upb = upb.data(); w.nup = nup;
  w.up_node.resize(nup); w.up_level.resize(nup);
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t l = 1; l <= lev[i]; l++) { w.up_node[upb[i] + l - 1] = i; w.up_level[upb[i] + l - 1] = l; }
  size_t rev_cap = 1;
  for (const BatchStep &s : steps) {
    w.max_batch = std::max(w.max_batch, s.size);
    if ((int32_t)s.ep == -1) continue;   // the first row of a build: no search, no edge
    size_t edges = 0;
    for (uint32_t k = 0; k < s.size; k++) edges += (size_t)g.M * (std::min<int64_t>(lev[s.begin + k], s.top) + 1);
    rev_cap = std::max(rev_cap, edges);
  }
  if (rev_cap > 0xFFFFFFF0u) return hipErrorInvalidValue;
  w.rev_cap = (uint32_t)rev_cap;
  w.gstride = (((size_t)n + 31) / 32 + 1) / 2 * 2 + 2 * (size_t)n;
  const size_t ntasks = (size_t)n + nup, words0 = (size_t)n * g.s0, words_up = std::max<size_t>((size_t)nup * g.su, 1);
  BG_TRY(w.l0.alloc(words0));
  BG_TRY(w.lu.alloc(words_up));
  BG_TRY(w.upb.alloc((size_t)n + 1));
  BG_TRY(w.lev.alloc(n));
  BG_TRY(w.upnode.alloc(std::max<size_t>(nup, 1)));
  BG_TRY(w.uplevel.alloc(std::max<size_t>(nup, 1)));
  BG_TRY(w.flagged.alloc(w.max_batch));
  BG_TRY(w.ctr.alloc(kBgCtrWords));
  BG_TRY(w.scratch.alloc(w.gstride * std::min(kBgRerunGrid, w.max_batch)));
  BG_TRY(w.rcnt.alloc(ntasks));
  BG_TRY(w.roff.alloc(ntasks));
  BG_TRY(w.rcur.alloc(ntasks));
  BG_TRY(w.rev.alloc(rev_cap));
  BG_TRY(w.upb.upload(upb.data(), (size_t)n + 1));
  BG_TRY(w.lev.upload(lev, n));
  if (nup) {
    BG_TRY(w.upnode.upload(w.up_node.data(), nup));
    BG_TRY(w.uplevel.upload(w.up_level.data(), nup));
  }
  BG_TRY(lists0 ? w.l0.upload(lists0, words0) : w.l0.zero(words0));
  BG_TRY(lists_up && nup ? w.lu.upload(lists_up, (size_t)nup * g.su) : w.lu.zero(words_up));
  BG_TRY(w.rcnt.zero(ntasks));
  BG_TRY(w.roff.zero(ntasks));
  BG_TRY(w.rcur.zero(ntasks));
  BG_TRY(w.ctr.zero(kBgCtrWords));
  g.l0 = w.l0.p; g.lu = w.lu.p; g.upb = w.upb.p; g.lev = w.lev.p;
  BG_TRY(hipEventCreate(&w.e0));
  return hipEventCreate(&w.e1);
}

// An instantiation whose dynamic LDS exceeds 64 KiB has to be told so.
template <class K>
static hipError_t bg_allow_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <class F, int METRIC>
static hipError_t bg_run_as(const BgWork &w, const std::vector<BatchStep> &steps, hipStream_t st, const BgMarks *marks) {
  const BgDev &g = w.g;
  const size_t lds_a = bg_search_lds<F>(g.dpad, g.efc, w.scratch_ids), lds_r = bg_search_lds<F>(g.dpad, g.efc, 0), lds_l = bg_link_lds<F>(g.dpad);
  BG_TRY(bg_allow_lds(bg_search_kernel<F, METRIC, true>, lds_a));
  BG_TRY(bg_allow_lds(bg_search_kernel<F, METRIC, false>, lds_r));
  BG_TRY(bg_allow_lds(bg_link_kernel<F, METRIC>, lds_l));
  for (const BatchStep &s : steps) {
    if ((int32_t)s.ep == -1) continue;   // the first row: an empty list, as the zeroed arrays have it
    const uint32_t nact = s.begin + w.h_upb[s.begin];
    BG_TRY(hipMemsetAsync(w.ctr.p, 0, 4, st));
    hipLaunchKernelGGL((bg_search_kernel<F, METRIC, true>), dim3(s.size), dim3(64), lds_a, st, g, s.begin, s.size, s.ep, s.top, w.scratch_ids,
                       w.flagged.p, w.ctr.p, (uint32_t *)nullptr, (size_t)0);
    hipLaunchKernelGGL((bg_search_kernel<F, METRIC, false>), dim3(std::min(kBgRerunGrid, s.size)), dim3(64), lds_r, st, g, s.begin, s.size, s.ep,
                       s.top, 0u, w.flagged.p, w.ctr.p, w.scratch.p, w.gstride);
    hipLaunchKernelGGL((bg_rev_kernel<false>), dim3((s.size + 3) / 4), dim3(256), 0, st, g, s.begin, s.size, s.top, w.rcnt.p, w.roff.p, w.rcur.p,
                       w.rev.p, w.rev_cap);
    hipLaunchKernelGGL(bg_scan_kernel, dim3(1), dim3(256), 0, st, w.rcnt.p, w.roff.p, s.begin, g.n, nact);
    hipLaunchKernelGGL((bg_rev_kernel<true>), dim3((s.size + 3) / 4), dim3(256), 0, st, g, s.begin, s.size, s.top, w.rcnt.p, w.roff.p, w.rcur.p,
                       w.rev.p, w.rev_cap);
    if (marks)   // (before the link kernel, which resets the counts)
      hipLaunchKernelGGL(bga_mark_kernel, dim3(std::min((nact + 255u) / 256u, 4096u)), dim3(256), 0, st, w.rcnt.p, s.begin, g.n, nact, *marks);
    hipLaunchKernelGGL((bg_link_kernel<F, METRIC>), dim3(std::min(nact, 8192u)), dim3(64), lds_l, st, g, s.begin, nact, w.upnode.p, w.uplevel.p,
                       w.rcnt.p, w.roff.p, w.rcur.p, w.rev.p, w.rev_cap);
    BG_TRY(hipGetLastError());
  }
  return hipSuccess;
}
// the batches of `steps` on stream `st`: the one place that turns metric and flavour into an instantiation
static hipError_t bg_run(const BgWork &w, const std::vector<BatchStep> &steps, int metric, bool rq, hipStream_t st, const BgMarks *marks = nullptr) {
  if (rq) return metric == METRIC_L2 ? bg_run_as<BgRabitq, METRIC_L2>(w, steps, st, marks) : bg_run_as<BgRabitq, METRIC_IP>(w, steps, st, marks);
  return metric == METRIC_L2 ? bg_run_as<BgHnswlib, METRIC_L2>(w, steps, st, marks) : bg_run_as<BgHnswlib, METRIC_IP>(w, steps, st, marks);
}

hipError_t gpu_batch_build(const GpuBuildInput &in, int device, std::vector<uint32_t> &lists0, std::vector<uint32_t> &lists_up,
                           std::vector<uint32_t> &upb, uint64_t &flagged_rows, double *kernel_ms) {
  const uint32_t n = in.n, scratch_ids = in.scratch_ids ? in.scratch_ids : kBgScratchIds;
  flagged_rows = 0;
  if (!(in.rq ? gpu_rq_build_supported(in.dim, in.M, in.efc, scratch_ids) : gpu_build_supported(in.dim, in.M, in.efc, scratch_ids)) || n == 0 ||
      n > 0x7FFFFFF0u)
    return hipErrorInvalidValue;
  upb.assign((size_t)n + 1, 0);
  std::vector<uint32_t> lev(n);
  for (uint32_t i = 0; i < n; i++) { lev[i] = (uint32_t)in.levels[i]; upb[i + 1] = upb[i] + lev[i]; }
  BgDev shape{};
  shape.n = n; shape.dim = in.dim; shape.M = in.M; shape.maxM = in.maxM; shape.maxM0 = in.maxM0; shape.efc = in.efc;
  BgWork w;
  BgBuf<float> d_vec;
  uint32_t ctr[2] = {0, 0};
  BG_TRY(hipSetDevice(device));
  BG_TRY(bg_work_init(w, shape, scratch_ids, lev.data(), upb, *in.steps, nullptr, nullptr));
  BG_TRY(d_vec.alloc((size_t)n * in.dim));
  BG_TRY(d_vec.upload(in.base, (size_t)n * in.dim));
  BG_TRY(hipDeviceSynchronize());
  w.g.vec = d_vec.p;
  BG_TRY(hipEventRecord(w.e0, nullptr));
  BG_TRY(bg_run(w, *in.steps, in.metric, in.rq, nullptr));
  BG_TRY(hipEventRecord(w.e1, nullptr));
  BG_TRY(hipEventSynchronize(w.e1));
  if (kernel_ms) { float ms = 0.f; BG_TRY(hipEventElapsedTime(&ms, w.e0, w.e1)); *kernel_ms = ms; }
  BG_TRY(hipMemcpy(ctr, w.ctr.p, 8, hipMemcpyDeviceToHost));
  flagged_rows = ctr[1];
  lists0.resize((size_t)n * w.g.s0);
  lists_up.resize((size_t)w.nup * w.g.su);
  BG_TRY(hipMemcpy(lists0.data(), w.l0.p, lists0.size() * 4, hipMemcpyDeviceToHost));
  if (w.nup) BG_TRY(hipMemcpy(lists_up.data(), w.lu.p, lists_up.size() * 4, hipMemcpyDeviceToHost));
  return hipSuccess;
}

// rq_dists over n_pairs pairs of host rows on `device` (hs_debug_rq_raw_dist)
hipError_t gpu_rq_raw_dist(const float *a, const float *b, size_t n_pairs, uint32_t dim, int metric, int device, float *out) {
  const uint32_t dpad = (dim + 3u) & ~3u;
  const size_t lds = (size_t)dpad * 4 + 64, count = n_pairs * dim;
  if (dim == 0 || lds > 64 * 1024 || n_pairs > 0x7FFFFFF0u) return hipErrorInvalidValue;
  if (n_pairs == 0) return hipSuccess;
  BgBuf<float> d_a, d_b, d_o;
  BG_TRY(hipSetDevice(device));
  BG_TRY(d_a.alloc(count));
  BG_TRY(d_b.alloc(count));
  BG_TRY(d_o.alloc(n_pairs));
  BG_TRY(d_a.upload(a, count));
  BG_TRY(d_b.upload(b, count));
  if (metric == METRIC_L2)
    hipLaunchKernelGGL(rq_dist_debug_kernel<METRIC_L2>, dim3((uint32_t)std::min<size_t>(n_pairs, 4096)), dim3(64), lds, nullptr, d_a.p, d_b.p, (uint32_t)n_pairs, dim, dpad, d_o.p);
  else
    hipLaunchKernelGGL(rq_dist_debug_kernel<METRIC_IP>, dim3((uint32_t)std::min<size_t>(n_pairs, 4096)), dim3(64), lds, nullptr, d_a.p, d_b.p, (uint32_t)n_pairs, dim, dpad, d_o.p);
  BG_TRY(hipGetLastError());
  return hipMemcpy(out, d_o.p, n_pairs * 4, hipMemcpyDeviceToHost);
}

// gpu_batch_build's batches continued on a resident index: the rows are the index's own array (the new ones copied behind the old --
// no list names them until a batch has run, so no search sees them), the lists are seeded from the host image, and what comes back
// is one dense buffer of the changed old slots and the new nodes' slots.
hipError_t gpu_batch_add(const GpuAddInput &in, int device, GpuAddOutput &out) {
  const uint32_t scratch_ids = in.scratch_ids ? in.scratch_ids : kBgScratchIds;
  out = GpuAddOutput();
  if (!gpu_build_supported(in.dim, in.M, in.efc, scratch_ids) || in.maxM != in.M || in.maxM0 != 2 * in.M || in.n0 == 0 || in.count == 0 ||
      (uint64_t)in.n0 + in.count > 0x7FFFFFF0u || !in.d_vec || !in.rows || !in.lev || !in.steps || !in.upb || !in.lists0 || !in.lists_up)
    return hipErrorInvalidValue;
  const uint32_t n0 = in.n0, n = in.n0 + in.count;
  const std::vector<uint32_t> &upb = *in.upb;
  if (upb.size() != (size_t)n + 1 || in.lists0->size() != (size_t)n * (in.maxM0 + 1) || in.lists_up->size() != (size_t)upb[n] * (in.maxM + 1))
    return hipErrorInvalidValue;
  for (const BatchStep &s : *in.steps)
    if (s.begin < n0 || (uint64_t)s.begin + s.size > n || s.ep >= s.begin || s.top < 0) return hipErrorInvalidValue;
  const uint32_t nup = upb[n], nup0 = upb[n0], nold = n0 + nup0, nw = (nold + 63u) / 64u;
  const uint32_t nnew_slots = in.count + (nup - nup0);
  BgDev shape{};
  shape.n = n; shape.dim = in.dim; shape.M = in.M; shape.maxM = in.maxM; shape.maxM0 = in.maxM0; shape.efc = in.efc;
  BgWork w;
  BgBuf<uint8_t> d_mark;
  BgBuf<uint32_t> d_counts, d_ids, d_out;
  uint32_t ctr[kBgCtrWords] = {0, 0, 0};
  BG_TRY(hipSetDevice(device));
  BG_TRY(bg_work_init(w, shape, scratch_ids, in.lev, upb, *in.steps, in.lists0->data(), in.lists_up->data()));
  const BgDev &g = w.g;
  BG_TRY(d_mark.alloc(nold));
  BG_TRY(d_counts.alloc(nw));
  BG_TRY(d_ids.alloc(nold));
  BG_TRY(hipMemcpy(in.d_vec + (size_t)n0 * in.dim, in.rows, (size_t)in.count * in.dim * 4, hipMemcpyHostToDevice));
  BG_TRY(d_mark.zero(nold));
  BG_TRY(hipDeviceSynchronize());
  w.g.vec = in.d_vec;
  const BgMarks marks{d_mark.p, n0, nup0};
  BG_TRY(hipEventRecord(w.e0, nullptr));
  BG_TRY(bg_run(w, *in.steps, in.metric, false, nullptr, &marks));
  hipLaunchKernelGGL(bga_count_kernel, dim3((nw + 3) / 4), dim3(256), 0, nullptr, d_mark.p, nold, d_counts.p);
  hipLaunchKernelGGL(bga_scan_kernel, dim3(1), dim3(256), 0, nullptr, d_counts.p, nw, w.ctr.p + 2);
  hipLaunchKernelGGL(bga_scatter_kernel, dim3((nw + 3) / 4), dim3(256), 0, nullptr, d_mark.p, nold, n0, n, d_counts.p, d_ids.p);
  BG_TRY(hipGetLastError());
  BG_TRY(hipMemcpy(ctr, w.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
  const uint32_t nchg = std::min(ctr[2], nold), nslots = nchg + nnew_slots;
  BG_TRY(d_out.alloc((size_t)nslots * g.s0 + std::max(nchg, 1u)));
  hipLaunchKernelGGL(bga_gather_kernel, dim3((nslots + 3) / 4), dim3(256), 0, nullptr, g, d_ids.p, nchg, n0, nup0, nup, nslots, d_out.p);
  BG_TRY(hipGetLastError());
  BG_TRY(hipEventRecord(w.e1, nullptr));
  BG_TRY(hipEventSynchronize(w.e1));
  float ms = 0.f;
  BG_TRY(hipEventElapsedTime(&ms, w.e0, w.e1));
  out.kernel_ms = ms;
  out.flagged_rows = ctr[1];
  std::vector<uint32_t> buf((size_t)nslots * g.s0 + nchg);
  BG_TRY(hipMemcpy(buf.data(), d_out.p, buf.size() * 4, hipMemcpyDeviceToHost));   // the one download
  out.tasks.assign(buf.begin() + (size_t)nslots * g.s0, buf.end());
  buf.resize((size_t)nslots * g.s0);
  out.slots.swap(buf);
  return hipSuccess;
}

}  // namespace hs
