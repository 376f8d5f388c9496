// build_gpu.hip -- batched addPoint on gfx950 (the host twin is host_batch_build.hpp, and the two write the same
// bytes).  Per batch, on one stream:
//   bg_search_kernel   one wavefront per new row: the upper-level descent, then per level the reference's build-time beam
//                      (searchBaseLayer, hnswalg.h:229-322: candidate and result heaps under CompareByFirst with libstdc++'s push /
//                      pop mechanics on one lane, heap_emul.hpp; an exact visited set; neighbours in adjacency order) and
//                      getNeighborsByHeuristic2 (:481-523: candidates by (distance ascending, id descending), the keep loop of
//                      cv_prune, the kept entries re-emplaced and popped, diff_prune.hpp).  It writes the row's own lists: no search
//                      of the batch can reach them, since no older node links to a row of the batch yet.
//                      The visited set (a hash) and the candidate heap live in LDS; a row that outgrows its share is flagged,
//                      and the same kernel runs again over the flagged rows with a bitmap and a heap in device memory.
//   bg_rev_count / bg_scan / bg_rev_fill   the new edges grouped by (target, level), as cv_rev_* and cd_scan_kernel do.
//   bg_link_kernel     one wavefront per target list with incoming ids: the reverse-link step of mutuallyConnectNewElement
//                      (:618-683) for its incoming ids in ascending order -- append while there is room, otherwise the heuristic
//                      over {new id} + the list at maxM / maxM0, stored in pop order (what it does not overwrite stays, as in
//                      the reference's memory).
// Every store is a vector store; nothing is read back between batches.
// The same batches for rabitqlib's builder, the graph HNSW-SlimQ converts from: rq_search_kernel / rq_link_kernel,
// between the same bg_rev / bg_scan launches (GpuBuildInput::rq).
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

// ascending sort of arr[0..N) (N a power of two, padding entries behind every candidate) in the candidate order of the heuristic
__device__ __forceinline__ void bg_sort_candidates(Pair *arr, uint32_t N, int lane) {
  for (uint32_t k = 2; k <= N; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = lane; i < N; i += 64) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const Pair a = arr[i], b = arr[p];
          const bool a_after_b = b.id != kBgPad && (a.id == kBgPad || h2_before(b, a));
          const bool up = (i & k) == 0;
          if (a_after_b == up) { arr[i] = b; arr[p] = a; }
        }
      }
      wave_sync();
    }
}

// ---- phase A ------------------------------------------------------------------------------------------------------------------------
// ONCHIP: grid = the rows of the batch.  Otherwise: the flagged rows, kBgRerunGrid workgroups, scratch area `blockIdx.x` of gscratch
// ((n + 31) / 32 bitmap words, then n candidate pairs).  ctr[0]: flagged rows of this batch, ctr[1]: of the build.
template <int METRIC, bool ONCHIP>
__global__ void __launch_bounds__(64) bg_search_kernel(BgDev g, uint32_t begin, uint32_t count, uint32_t ep, int32_t top, uint32_t scratch_ids,
                                                       uint32_t *flagged, uint32_t *ctr, uint32_t *gscratch, size_t gstride) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  float *qc = qv + g.dpad;
  Pair *topq = reinterpret_cast<Pair *>(qc + g.dpad);
  uint32_t *nid = reinterpret_cast<uint32_t *>(topq + g.topcap);
  float *nd = reinterpret_cast<float *>(nid + 64);
  uint32_t *kept = reinterpret_cast<uint32_t *>(nd + 64);
  float *keptd = reinterpret_cast<float *>(kept + 64);
  float *kd = keptd + 64;
  uint32_t *hash = reinterpret_cast<uint32_t *>(kd + 64);                      // ONCHIP: 2 * scratch_ids slots
  const uint32_t hmask = 2 * scratch_ids - 1;
  uint32_t *bitmap = gscratch + (size_t)blockIdx.x * gstride;                   // !ONCHIP
  Pair *cand = ONCHIP ? reinterpret_cast<Pair *>(hash + 2 * (size_t)scratch_ids) : reinterpret_cast<Pair *>(bitmap + (((size_t)g.n + 31) / 32 + 1) / 2 * 2);
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
    if ((int32_t)lp < top) {   // the greedy walk of the upper levels (hnswalg.h:1300-1326)
      if (lane == 0) nid[0] = cur;
      wave_sync();
      cv_dists<METRIC>(g.vec, g.dim, qv, nid, nd, 1, lane);
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
          cv_dists<METRIC>(g.vec, g.dim, qv, nid, nd, cnt, lane);
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
      // ---- searchBaseLayer --------------------------------------------------------------------------------------------------
      wave_sync();
      if (ONCHIP) for (uint32_t i = lane; i <= hmask; i += 64) hash[i] = kBgPad;
      else for (uint32_t i = lane; i < (begin + 31) / 32; i += 64) bitmap[i] = 0;
      if (lane == 0) nid[0] = cur;
      if (!ONCHIP) __syncthreads();   // (one wavefront per workgroup: orders the bitmap's plain stores before its atomics)
      wave_sync();
      cv_dists<METRIC>(g.vec, g.dim, qv, nid, nd, 1, lane);
      wave_sync();
      uint32_t topn = 1, candn = 1, nvis = 1;
      float lower = nd[0];
      if (lane == 0) {
        topq[0] = Pair{lower, cur};
        cand[0] = Pair{-lower, cur};
        if (ONCHIP) hash[(cur * 2654435761u) & hmask] = cur;
        else bitmap[cur >> 5] = 1u << (cur & 31);
      }
      if (!ONCHIP) __syncthreads();
      wave_sync();
      while (candn > 0) {
        Pair c{0.f, 0u};
        if (lane == 0) c = cand[0];   // (the lane that maintains the heap reads it: program order, whichever memory holds it)
        const uint32_t node = uni(c.id);
        if (-unif(c.d) > lower && topn == g.efc) break;
        if (lane == 0) pop_heap(cand, (long)candn, LessD());
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
        cv_dists<METRIC>(g.vec, g.dim, qv, nid, nd, nnew, lane);
        wave_sync();
        uint32_t ovf = 0;
        if (lane == 0) {
          for (uint32_t j = 0; j < nnew; j++) {
            const float d = nd[j];
            if (topn < g.efc || lower > d) {
              if (candn >= candcap) { ovf = 1; break; }
              cand[candn++] = Pair{-d, nid[j]};
              push_heap(cand, (long)candn, LessD());
              topq[topn++] = Pair{d, nid[j]};
              push_heap(topq, (long)topn, LessD());
              if (topn > g.efc) { pop_heap(topq, (long)topn, LessD()); topn--; }
              lower = topq[0].d;
            }
          }
        }
        topn = uni(topn); candn = uni(candn); lower = unif(lower); ovf = uni(ovf);
        wave_sync();
        if (ovf) { ok = false; break; }
      }
      if (!ok) break;
      // ---- getNeighborsByHeuristic2(top, M), then the pop order connect() reads -------------------------------------------------
      uint32_t kc;
      if (topn < g.M) {
        if (lane == 0)
          for (long m = topn; m > 1; m--) pop_heap(topq, m, LessD());
        kc = topn;
      } else {
        uint32_t N = 64;
        while (N < topn) N <<= 1;
        for (uint32_t i = topn + lane; i < N; i += 64) topq[i] = Pair{0.f, kBgPad};
        wave_sync();
        bg_sort_candidates(topq, N, lane);
        kc = cv_prune<METRIC>(g.vec, g.dim, topq, topn, g.M, qc, kept, kd, lane, keptd);
        wave_sync();
        if ((uint32_t)lane < kc) topq[lane] = Pair{keptd[lane], kept[lane]};
        wave_sync();
        if (lane == 0) h2_pop_order(topq, (long)kc);
      }
      wave_sync();
      uint32_t *own = bg_list(g, p, (uint32_t)level);
      if ((uint32_t)lane < kc) own[1 + lane] = topq[kc - 1 - lane].id;   // topq[kc - 1]: the first one popped
      if (lane == 0) own[0] = kc;
      cur = topq[0].id;   // sel.back()
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

// exclusive prefix sums of rcnt over the active tasks (one workgroup, as cd_scan_kernel)
__global__ void __launch_bounds__(256) bg_scan_kernel(const uint32_t *rcnt, uint32_t *roff, uint32_t begin, uint32_t n, uint32_t nact) {
  __shared__ uint32_t part[256];
  const uint32_t t = threadIdx.x, per = (nact + 255u) / 256u, lo = min(nact, t * per), hi = min(nact, lo + per);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; i++) sum += rcnt[bg_active(i, begin, n)];
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (uint32_t j = 0; j < 256; j++) { const uint32_t c = part[j]; part[j] = run; run += c; }
  }
  __syncthreads();
  sum = part[t];
  for (uint32_t i = lo; i < hi; i++) { const uint32_t a = bg_active(i, begin, n); roff[a] = sum; sum += rcnt[a]; }
}

// ---- phase B: the reverse links ------------------------------------------------------------------------------------------------------
// up_node / up_level: node and level of upper slot j (task n + j)
template <int METRIC>
__global__ void __launch_bounds__(64) bg_link_kernel(BgDev g, uint32_t begin, uint32_t nact, const uint32_t *up_node, const uint32_t *up_level,
                                                     uint32_t *rcnt, const uint32_t *roff, uint32_t *rcur, uint32_t *rev, uint32_t rev_cap) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  float *qc = qv + g.dpad;
  Pair *arr = reinterpret_cast<Pair *>(qc + g.dpad);
  uint32_t *nid = reinterpret_cast<uint32_t *>(arr + 64);
  float *nd = reinterpret_cast<float *>(nid + 64);
  uint32_t *kept = reinterpret_cast<uint32_t *>(nd + 64);
  float *keptd = reinterpret_cast<float *>(kept + 64);
  float *kd = keptd + 64;
  uint32_t *curl = reinterpret_cast<uint32_t *>(kd + 64);
  uint32_t *inc = curl + 64;
  const int lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < nact; i += gridDim.x) {
    const uint32_t task = bg_active(i, begin, g.n);
    const uint32_t k = uni(rcnt[task]);
    if (k == 0) continue;
    const uint32_t off = uni(roff[task]);
    if (off >= rev_cap || k > rev_cap - off) continue;   // (never: the host sizes rev for every edge of the batch)
    const uint32_t u = task < g.n ? task : up_node[task - g.n], level = task < g.n ? 0u : up_level[task - g.n];
    const uint32_t lim = level ? g.maxM : g.maxM0;
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
      const uint32_t sz = cnt + 1;   // <= 63: {p} + the full list
      if (lane == 0) nid[0] = p;
      if ((uint32_t)lane < cnt) nid[1 + lane] = curl[lane];
      wave_sync();
      cv_dists<METRIC>(g.vec, g.dim, qv, nid, nd, sz, lane);
      wave_sync();
      {
        const bool act = (uint32_t)lane < sz;
        const Pair mine{act ? nd[lane] : 0.f, act ? nid[lane] : 0u};
        uint32_t rank = 0;
        for (uint32_t j = 0; j < sz; j++) rank += h2_before(Pair{nd[j], nid[j]}, mine) ? 1u : 0u;
        if (act) arr[rank] = mine;
      }
      wave_sync();
      const uint32_t kc = cv_prune<METRIC>(g.vec, g.dim, arr, sz, lim, qc, kept, kd, lane, keptd);
      wave_sync();
      if ((uint32_t)lane < kc) arr[lane] = Pair{keptd[lane], kept[lane]};
      wave_sync();
      if (lane == 0) h2_pop_order(arr, (long)kc);
      wave_sync();
      if ((uint32_t)lane < kc) curl[lane] = arr[kc - 1 - lane].id;
      cnt = kc;
      wave_sync();
    }
    if ((uint32_t)lane < lim) lst[1 + lane] = curl[lane];
    if (lane == 0) { lst[0] = cnt; rcnt[task] = 0; rcur[task] = 0; }
  }
}

// ---- rabitqlib's builder (the host twin is host_rq_batch_build.hpp) ---------------------------------------------------
// The same batches for the graph HNSW-SlimQ converts from (RqGraph, host_rq_graph.hpp), at M up to 32.  Kernels of their own, with
// the signatures of the two above, so that the vanilla instantiations stay what they were: every distance is rq_dists (rq_dist.hpp),
// both heaps order (distance, id) pairs -- a total order, so libstdc++'s heap mechanics decide nothing and any correct heap or sort
// serves -- the heuristic takes its candidates by ascending pair and what it keeps leaves the max-heap in descending pair order,
// i.e. reversed; a list that already names the new id is left alone.  bg_rev_kernel and bg_scan_kernel serve both flavours.
__device__ __forceinline__ bool rq_less(const Pair &a, const Pair &b) { return a.d < b.d || (a.d == b.d && a.id < b.id); }
struct RqLess { __device__ __forceinline__ bool operator()(const Pair &a, const Pair &b) const { return rq_less(a, b); } };      // maxheap (hnsw.hpp:33-34)
struct RqGreater { __device__ __forceinline__ bool operator()(const Pair &a, const Pair &b) const { return rq_less(b, a); } };   // minheap (:35-36)

// ascending (distance, id) sort of arr[0..N) (N a power of two, padding entries behind every candidate)
__device__ __forceinline__ void rq_sort_asc(Pair *arr, uint32_t N, int lane) {
  for (uint32_t k = 2; k <= N; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = lane; i < N; i += 64) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const Pair a = arr[i], b = arr[p];
          const bool a_after_b = b.id != kBgPad && (a.id == kBgPad || rq_less(b, a));
          const bool up = (i & k) == 0;
          if (a_after_b == up) { arr[i] = b; arr[p] = a; }
        }
      }
      wave_sync();
    }
}

// The keep loop of get_neighbors_by_heuristic2 (hnsw.hpp:1016-1054) over arr[0..sz) in ascending pair order: a candidate is kept
// unless a kept one is closer to it than the node is.  kept / kd hold mlim <= 64 entries.
template <int METRIC>
__device__ __forceinline__ uint32_t rq_prune(const float *vec, uint32_t dim, const Pair *arr, uint32_t sz, uint32_t mlim, float *qc /*LDS dim*/,
                                             uint32_t *kept, float *kd, int lane) {
  uint32_t kc = 0;
  for (uint32_t t = 0; t < sz && kc < mlim; t++) {
    const float cd = unif(arr[t].d);
    const uint32_t cid = uni(arr[t].id);
    bool good = true;
    if (kc > 0) {
      for (uint32_t i = lane; i < dim; i += 64) qc[i] = vec[(size_t)cid * dim + i];
      wave_sync();
      rq_dists<METRIC>(vec, dim, qc, kept, kd, kc, lane);
      wave_sync();
      good = hs_ballot((uint32_t)lane < kc && kd[lane] < cd) == 0;
    }
    if (good) {
      if (lane == 0) kept[kc] = cid;
      kc++;
    }
    wave_sync();
  }
  return kc;
}

// phase A: bg_search_kernel's grid, flags and scratch; the LDS layout is rq_search_lds.
template <int METRIC, bool ONCHIP>
__global__ void __launch_bounds__(64) rq_search_kernel(BgDev g, uint32_t begin, uint32_t count, uint32_t ep, int32_t top, uint32_t scratch_ids,
                                                       uint32_t *flagged, uint32_t *ctr, uint32_t *gscratch, size_t gstride) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  float *qc = qv + g.dpad;
  Pair *topq = reinterpret_cast<Pair *>(qc + g.dpad);
  uint32_t *nid = reinterpret_cast<uint32_t *>(topq + g.topcap);
  float *nd = reinterpret_cast<float *>(nid + 64);
  uint32_t *kept = reinterpret_cast<uint32_t *>(nd + 64);
  float *kd = reinterpret_cast<float *>(kept + 64);
  uint32_t *hash = reinterpret_cast<uint32_t *>(kd + 64);                      // ONCHIP: 2 * scratch_ids slots
  const uint32_t hmask = 2 * scratch_ids - 1;
  uint32_t *bitmap = gscratch + (size_t)blockIdx.x * gstride;                   // !ONCHIP
  Pair *cand = ONCHIP ? reinterpret_cast<Pair *>(hash + 2 * (size_t)scratch_ids) : reinterpret_cast<Pair *>(bitmap + (((size_t)g.n + 31) / 32 + 1) / 2 * 2);
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
    if ((int32_t)lp < top) {   // the greedy walk of the upper levels (hnsw.hpp:733-760)
      if (lane == 0) nid[0] = cur;
      wave_sync();
      rq_dists<METRIC>(g.vec, g.dim, qv, nid, nd, 1, lane);
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
          rq_dists<METRIC>(g.vec, g.dim, qv, nid, nd, cnt, lane);
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
      // ---- search_base_layer (hnsw.hpp:827-905) -------------------------------------------------------------------------------
      wave_sync();
      if (ONCHIP) for (uint32_t i = lane; i <= hmask; i += 64) hash[i] = kBgPad;
      else for (uint32_t i = lane; i < (begin + 31) / 32; i += 64) bitmap[i] = 0;
      if (lane == 0) nid[0] = cur;
      if (!ONCHIP) __syncthreads();   // (one wavefront per workgroup: orders the bitmap's plain stores before its atomics)
      wave_sync();
      rq_dists<METRIC>(g.vec, g.dim, qv, nid, nd, 1, lane);
      wave_sync();
      uint32_t topn = 1, candn = 1, nvis = 1;
      float lower = nd[0];
      if (lane == 0) {
        topq[0] = Pair{lower, cur};
        cand[0] = Pair{lower, cur};
        if (ONCHIP) hash[(cur * 2654435761u) & hmask] = cur;
        else bitmap[cur >> 5] = 1u << (cur & 31);
      }
      if (!ONCHIP) __syncthreads();
      wave_sync();
      while (candn > 0) {
        Pair c{0.f, 0u};
        if (lane == 0) c = cand[0];   // (the lane that maintains the heap reads it: program order, whichever memory holds it)
        const uint32_t node = uni(c.id);
        if (unif(c.d) > lower && topn == g.efc) break;
        if (lane == 0) pop_heap(cand, (long)candn, RqGreater());
        candn--;
        const uint32_t lim = level ? g.maxM : g.maxM0;
        const uint32_t *l = bg_list(g, node, (uint32_t)level);
        const uint32_t cnt = min(uni(l[0]) & 0xFFFFu, lim);
        const uint32_t id = (uint32_t)lane < cnt ? l[1 + lane] : kBgPad;
        bool isnew = false;
        if (id < begin) {   // (every id of the graph so far is; the test keeps a damaged list inside the arrays)
          if (ONCHIP) {
            uint32_t slot = (id * 2654435761u) & hmask;
            while (true) {   // at most scratch_ids + 64 <= 2 * scratch_ids distinct ids ever reach the table: every probe sequence
              const uint32_t old = lds_cas(&hash[slot], kBgPad, id);   // meets an empty slot or its own id
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
        rq_dists<METRIC>(g.vec, g.dim, qv, nid, nd, nnew, lane);
        wave_sync();
        uint32_t ovf = 0;
        if (lane == 0) {
          for (uint32_t j = 0; j < nnew; j++) {
            const float d = nd[j];
            if (topn < g.efc || lower > d) {
              if (candn >= candcap) { ovf = 1; break; }
              cand[candn++] = Pair{d, nid[j]};
              push_heap(cand, (long)candn, RqGreater());
              topq[topn++] = Pair{d, nid[j]};
              push_heap(topq, (long)topn, RqLess());
              if (topn > g.efc) { pop_heap(topq, (long)topn, RqLess()); topn--; }
              lower = topq[0].d;
            }
          }
        }
        topn = uni(topn); candn = uni(candn); lower = unif(lower); ovf = uni(ovf);
        wave_sync();
        if (ovf) { ok = false; break; }
      }
      if (!ok) break;
      // ---- get_neighbors_by_heuristic2(top, M) (:1016-1054: nothing below M entries), then the pop order of :917-922 -----------------
      uint32_t N = 64;
      while (N < topn) N <<= 1;
      for (uint32_t i = topn + lane; i < N; i += 64) topq[i] = Pair{0.f, kBgPad};
      wave_sync();
      rq_sort_asc(topq, N, lane);
      uint32_t kc = topn;
      if (topn < g.M) {
        if ((uint32_t)lane < kc) kept[lane] = topq[lane].id;
      } else {
        kc = rq_prune<METRIC>(g.vec, g.dim, topq, topn, g.M, qc, kept, kd, lane);
      }
      wave_sync();
      uint32_t *own = bg_list(g, p, (uint32_t)level);
      if ((uint32_t)lane < kc) own[1 + lane] = kept[kc - 1 - lane];   // descending pair order: the max-heap's pops
      if (lane == 0) own[0] = kc;
      cur = uni(kept[0]);   // sel.back()
    }
    if (!ok && ONCHIP && lane == 0) {
      flagged[atomicAdd(&ctr[0], 1u)] = p;
      atomicAdd(&ctr[1], 1u);
    }
  }
}

// phase B: bg_link_kernel's tasks and segments; a full level-0 list at M = 32 plus the new id is 65 candidates, so the candidate
// arrays hold 128 entries, the rank sort takes two entries per lane and the keep loop keeps at most 64, one lane per kept entry.
template <int METRIC>
__global__ void __launch_bounds__(64) rq_link_kernel(BgDev g, uint32_t begin, uint32_t nact, const uint32_t *up_node, const uint32_t *up_level,
                                                     uint32_t *rcnt, const uint32_t *roff, uint32_t *rcur, uint32_t *rev, uint32_t rev_cap) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  float *qc = qv + g.dpad;
  Pair *arr = reinterpret_cast<Pair *>(qc + g.dpad);
  uint32_t *nid = reinterpret_cast<uint32_t *>(arr + 128);
  float *nd = reinterpret_cast<float *>(nid + 128);
  uint32_t *kept = reinterpret_cast<uint32_t *>(nd + 128);
  float *kd = reinterpret_cast<float *>(kept + 64);
  uint32_t *curl = reinterpret_cast<uint32_t *>(kd + 64);
  uint32_t *inc = curl + 64;
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
      if (hs_ballot((uint32_t)lane < cnt && curl[lane] == p) != 0) continue;   // the list names p already (hnsw.hpp:973-980)
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
      const uint32_t sz = cnt + 1;   // <= 65: {p} + the full list
      if (lane == 0) nid[0] = p;
      if ((uint32_t)lane < cnt) nid[1 + lane] = curl[lane];
      wave_sync();
      rq_dists<METRIC>(g.vec, g.dim, qv, nid, nd, sz, lane);
      wave_sync();
      for (uint32_t x = lane; x < sz; x += 64) {   // ascending pair order by rank; equal pairs (a damaged list) by their place
        const Pair mine{nd[x], nid[x]};
        uint32_t rank = 0;
        for (uint32_t j = 0; j < sz; j++) {
          const Pair o{nd[j], nid[j]};
          rank += (rq_less(o, mine) || (!rq_less(mine, o) && j < x)) ? 1u : 0u;
        }
        arr[rank] = mine;
      }
      wave_sync();
      const uint32_t kc = rq_prune<METRIC>(g.vec, g.dim, arr, sz, lim, qc, kept, kd, lane);
      wave_sync();
      if ((uint32_t)lane < kc) curl[lane] = kept[kc - 1 - lane];   // pop order; what it does not overwrite stays
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
  __shared__ uint32_t part[256];
  const uint32_t t = threadIdx.x, per = (nw + 255u) / 256u, lo = min(nw, t * per), hi = min(nw, lo + per);
  uint32_t sum = 0;
  for (uint32_t w = lo; w < hi; w++) sum += counts[w];
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (uint32_t j = 0; j < 256; j++) { const uint32_t c = part[j]; part[j] = run; run += c; }
    *total = run;
  }
  __syncthreads();
  sum = part[t];
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
static uint32_t bg_topcap(uint32_t efc) {
  uint32_t c = 64;
  while (c < efc + 1) c <<= 1;
  return c;
}
static size_t bg_search_lds(uint32_t dpad, uint32_t efc, uint32_t scratch_ids) {
  return (size_t)dpad * 8 + (size_t)bg_topcap(efc) * 8 + 5 * 256 + (size_t)scratch_ids * 12;
}
static size_t bg_link_lds(uint32_t dpad) { return (size_t)dpad * 8 + 64 * 8 + 7 * 256; }
static size_t rq_search_lds(uint32_t dpad, uint32_t efc, uint32_t scratch_ids) {
  return (size_t)dpad * 8 + (size_t)bg_topcap(efc) * 8 + 4 * 256 + (size_t)scratch_ids * 12;
}
static size_t rq_link_lds(uint32_t dpad) { return (size_t)dpad * 8 + 128 * 8 + 2 * 512 + 4 * 256; }

bool gpu_build_supported(uint32_t dim, uint32_t M, uint32_t efc, uint32_t scratch_ids) {
  if (scratch_ids == 0) scratch_ids = kBgScratchIds;
  if (M == 0 || M > kBgMaxM || std::max(efc, M) > kBgMaxEfc || dim == 0) return false;
  if (scratch_ids < 64 || (scratch_ids & (scratch_ids - 1)) != 0 || scratch_ids > 8192) return false;
  const uint32_t dpad = (dim + 3u) & ~3u;
  return bg_search_lds(dpad, std::max(efc, M), scratch_ids) <= kBgLdsLimit && bg_link_lds(dpad) <= kBgLdsLimit;
}

bool gpu_rq_build_supported(uint32_t dim, uint32_t M, uint32_t efc, uint32_t scratch_ids) {
  if (scratch_ids == 0) scratch_ids = kBgScratchIds;
  if (M < 2 || M > kRqMaxM || std::max(efc, M) > kBgMaxEfc || dim == 0) return false;
  if (scratch_ids < 64 || (scratch_ids & (scratch_ids - 1)) != 0 || scratch_ids > 8192) return false;
  const uint32_t dpad = (dim + 3u) & ~3u;
  return rq_search_lds(dpad, std::max(efc, M), scratch_ids) <= kBgLdsLimit && rq_link_lds(dpad) <= kBgLdsLimit;
}

#define BG_TRY(expr)                               \
  do {                                             \
    hipError_t _e = (expr);                        \
    if (_e != hipSuccess) { err = _e; goto done; } \
  } while (0)

template <int METRIC, bool RQ = false>
static hipError_t bg_run(const std::vector<BatchStep> &steps, const BgDev &g, const std::vector<uint32_t> &upb, uint32_t scratch_ids, uint32_t *d_flagged,
                         uint32_t *d_ctr, uint32_t *d_scratch, size_t gstride, uint32_t *d_rcnt, uint32_t *d_roff, uint32_t *d_rcur, uint32_t *d_rev,
                         uint32_t rev_cap, const uint32_t *d_upnode, const uint32_t *d_uplevel, hipStream_t st, const BgMarks *marks = nullptr) {
  // the flavour's three kernels (the rq ones have the vanilla signatures)
  const auto search_chip = RQ ? rq_search_kernel<METRIC, true> : bg_search_kernel<METRIC, true>;
  const auto search_mem = RQ ? rq_search_kernel<METRIC, false> : bg_search_kernel<METRIC, false>;
  const auto link = RQ ? rq_link_kernel<METRIC> : bg_link_kernel<METRIC>;
  const size_t lds_a = RQ ? rq_search_lds(g.dpad, g.efc, scratch_ids) : bg_search_lds(g.dpad, g.efc, scratch_ids);
  const size_t lds_r = RQ ? rq_search_lds(g.dpad, g.efc, 0) : bg_search_lds(g.dpad, g.efc, 0), lds_l = RQ ? rq_link_lds(g.dpad) : bg_link_lds(g.dpad);
  hipError_t e;
  if (lds_a > 64 * 1024 && (e = hipFuncSetAttribute(reinterpret_cast<const void *>(search_chip), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a)) != hipSuccess) return e;
  if (lds_r > 64 * 1024 && (e = hipFuncSetAttribute(reinterpret_cast<const void *>(search_mem), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r)) != hipSuccess) return e;
  if (lds_l > 64 * 1024 && (e = hipFuncSetAttribute(reinterpret_cast<const void *>(link), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_l)) != hipSuccess) return e;
  for (const BatchStep &s : steps) {
    if ((int32_t)s.ep == -1) continue;   // the first row: an empty list, as the zeroed arrays have it
    const uint32_t nact = s.begin + upb[s.begin];
    if ((e = hipMemsetAsync(d_ctr, 0, 4, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(search_chip, dim3(s.size), dim3(64), lds_a, st, g, s.begin, s.size, s.ep, s.top, scratch_ids, d_flagged, d_ctr,
                       (uint32_t *)nullptr, (size_t)0);
    hipLaunchKernelGGL(search_mem, dim3(std::min(kBgRerunGrid, s.size)), dim3(64), lds_r, st, g, s.begin, s.size, s.ep, s.top, 0u,
                       d_flagged, d_ctr, d_scratch, gstride);
    hipLaunchKernelGGL((bg_rev_kernel<false>), dim3((s.size + 3) / 4), dim3(256), 0, st, g, s.begin, s.size, s.top, d_rcnt, d_roff, d_rcur, d_rev, rev_cap);
    hipLaunchKernelGGL(bg_scan_kernel, dim3(1), dim3(256), 0, st, d_rcnt, d_roff, s.begin, g.n, nact);
    hipLaunchKernelGGL((bg_rev_kernel<true>), dim3((s.size + 3) / 4), dim3(256), 0, st, g, s.begin, s.size, s.top, d_rcnt, d_roff, d_rcur, d_rev, rev_cap);
    if (marks)   // (before the link kernel, which resets the counts)
      hipLaunchKernelGGL(bga_mark_kernel, dim3(std::min((nact + 255u) / 256u, 4096u)), dim3(256), 0, st, d_rcnt, s.begin, g.n, nact, *marks);
    hipLaunchKernelGGL(link, dim3(std::min(nact, 8192u)), dim3(64), lds_l, st, g, s.begin, nact, d_upnode, d_uplevel, d_rcnt, d_roff,
                       d_rcur, d_rev, rev_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t gpu_batch_build(const GpuBuildInput &in, int device, std::vector<uint32_t> &lists0, std::vector<uint32_t> &lists_up,
                           std::vector<uint32_t> &upb, uint64_t &flagged_rows, double *kernel_ms) {
  hipError_t err = hipSuccess;
  const uint32_t n = in.n, scratch_ids = in.scratch_ids ? in.scratch_ids : kBgScratchIds;
  flagged_rows = 0;
  if (!(in.rq ? gpu_rq_build_supported(in.dim, in.M, in.efc, scratch_ids) : gpu_build_supported(in.dim, in.M, in.efc, scratch_ids)) || n == 0 ||
      n > 0x7FFFFFF0u)
    return hipErrorInvalidValue;
  BgDev g{};
  g.n = n; g.dim = in.dim; g.dpad = (in.dim + 3u) & ~3u; g.M = in.M; g.maxM = in.maxM; g.maxM0 = in.maxM0;
  g.s0 = in.maxM0 + 1; g.su = in.maxM + 1; g.efc = in.efc; g.topcap = bg_topcap(in.efc);
  upb.assign((size_t)n + 1, 0);
  std::vector<uint32_t> lev(n);
  for (uint32_t i = 0; i < n; i++) { lev[i] = (uint32_t)in.levels[i]; upb[i + 1] = upb[i] + lev[i]; }
  const uint32_t nup = upb[n];
  std::vector<uint32_t> up_node(nup), up_level(nup);
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t l = 1; l <= lev[i]; l++) { up_node[upb[i] + l - 1] = i; up_level[upb[i] + l - 1] = l; }
  uint32_t max_batch = 1;
  size_t rev_cap = 1;   // the most edges one batch can add: M per (row, level it is searched on)
  for (const BatchStep &s : *in.steps) {
    max_batch = std::max(max_batch, s.size);
    size_t edges = 0;
    for (uint32_t k = 0; k < s.size; k++) edges += (size_t)in.M * (std::min<int64_t>(in.levels[s.begin + k], s.top) + 1);
    rev_cap = std::max(rev_cap, (int32_t)s.ep == -1 ? (size_t)1 : edges);
  }
  if (rev_cap > 0xFFFFFFF0u) return hipErrorInvalidValue;
  const size_t ntasks = (size_t)n + nup;
  const size_t gstride = (((size_t)n + 31) / 32 + 1) / 2 * 2 + 2 * (size_t)n;   // words: bitmap (padded to a pair's alignment) + n pairs
  float *d_vec = nullptr;
  uint32_t *d_l0 = nullptr, *d_lu = nullptr, *d_upb = nullptr, *d_lev = nullptr, *d_upnode = nullptr, *d_uplevel = nullptr, *d_flagged = nullptr,
           *d_ctr = nullptr, *d_scratch = nullptr, *d_rcnt = nullptr, *d_roff = nullptr, *d_rcur = nullptr, *d_rev = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint32_t ctr[2] = {0, 0};
  BG_TRY(hipSetDevice(device));
  BG_TRY(hipMalloc((void **)&d_vec, (size_t)n * in.dim * 4));
  BG_TRY(hipMalloc((void **)&d_l0, (size_t)n * g.s0 * 4));
  BG_TRY(hipMalloc((void **)&d_lu, std::max<size_t>((size_t)nup * g.su, 1) * 4));
  BG_TRY(hipMalloc((void **)&d_upb, ((size_t)n + 1) * 4));
  BG_TRY(hipMalloc((void **)&d_lev, (size_t)n * 4));
  BG_TRY(hipMalloc((void **)&d_upnode, std::max<size_t>(nup, 1) * 4));
  BG_TRY(hipMalloc((void **)&d_uplevel, std::max<size_t>(nup, 1) * 4));
  BG_TRY(hipMalloc((void **)&d_flagged, (size_t)max_batch * 4));
  BG_TRY(hipMalloc((void **)&d_ctr, 8));
  BG_TRY(hipMalloc((void **)&d_scratch, gstride * 4 * std::min(kBgRerunGrid, max_batch)));
  BG_TRY(hipMalloc((void **)&d_rcnt, ntasks * 4));
  BG_TRY(hipMalloc((void **)&d_roff, ntasks * 4));
  BG_TRY(hipMalloc((void **)&d_rcur, ntasks * 4));
  BG_TRY(hipMalloc((void **)&d_rev, rev_cap * 4));
  BG_TRY(hipMemcpy(d_vec, in.base, (size_t)n * in.dim * 4, hipMemcpyHostToDevice));
  BG_TRY(hipMemcpy(d_upb, upb.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
  BG_TRY(hipMemcpy(d_lev, lev.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  if (nup) {
    BG_TRY(hipMemcpy(d_upnode, up_node.data(), (size_t)nup * 4, hipMemcpyHostToDevice));
    BG_TRY(hipMemcpy(d_uplevel, up_level.data(), (size_t)nup * 4, hipMemcpyHostToDevice));
  }
  BG_TRY(hipMemset(d_l0, 0, (size_t)n * g.s0 * 4));
  BG_TRY(hipMemset(d_lu, 0, std::max<size_t>((size_t)nup * g.su, 1) * 4));
  BG_TRY(hipMemset(d_rcnt, 0, ntasks * 4));
  BG_TRY(hipMemset(d_roff, 0, ntasks * 4));
  BG_TRY(hipMemset(d_rcur, 0, ntasks * 4));
  BG_TRY(hipMemset(d_ctr, 0, 8));
  BG_TRY(hipDeviceSynchronize());
  g.vec = d_vec; g.l0 = d_l0; g.lu = d_lu; g.upb = d_upb; g.lev = d_lev;
  BG_TRY(hipEventCreate(&e0)); BG_TRY(hipEventCreate(&e1));
  BG_TRY(hipEventRecord(e0, nullptr));
  if (in.rq && in.metric == METRIC_L2)
    BG_TRY((bg_run<METRIC_L2, true>(*in.steps, g, upb, scratch_ids, d_flagged, d_ctr, d_scratch, gstride, d_rcnt, d_roff, d_rcur, d_rev, (uint32_t)rev_cap, d_upnode, d_uplevel, nullptr)));
  else if (in.rq)
    BG_TRY((bg_run<METRIC_IP, true>(*in.steps, g, upb, scratch_ids, d_flagged, d_ctr, d_scratch, gstride, d_rcnt, d_roff, d_rcur, d_rev, (uint32_t)rev_cap, d_upnode, d_uplevel, nullptr)));
  else if (in.metric == METRIC_L2)
    BG_TRY(bg_run<METRIC_L2>(*in.steps, g, upb, scratch_ids, d_flagged, d_ctr, d_scratch, gstride, d_rcnt, d_roff, d_rcur, d_rev, (uint32_t)rev_cap, d_upnode, d_uplevel, nullptr));
  else
    BG_TRY(bg_run<METRIC_IP>(*in.steps, g, upb, scratch_ids, d_flagged, d_ctr, d_scratch, gstride, d_rcnt, d_roff, d_rcur, d_rev, (uint32_t)rev_cap, d_upnode, d_uplevel, nullptr));
  BG_TRY(hipEventRecord(e1, nullptr));
  BG_TRY(hipEventSynchronize(e1));
  if (kernel_ms) { float ms = 0.f; BG_TRY(hipEventElapsedTime(&ms, e0, e1)); *kernel_ms = ms; }
  BG_TRY(hipMemcpy(ctr, d_ctr, 8, hipMemcpyDeviceToHost));
  flagged_rows = ctr[1];
  lists0.resize((size_t)n * g.s0);
  lists_up.resize((size_t)nup * g.su);
  BG_TRY(hipMemcpy(lists0.data(), d_l0, lists0.size() * 4, hipMemcpyDeviceToHost));
  if (nup) BG_TRY(hipMemcpy(lists_up.data(), d_lu, lists_up.size() * 4, hipMemcpyDeviceToHost));
done:
  for (void *p : {(void *)d_vec, (void *)d_l0, (void *)d_lu, (void *)d_upb, (void *)d_lev, (void *)d_upnode, (void *)d_uplevel, (void *)d_flagged,
                  (void *)d_ctr, (void *)d_scratch, (void *)d_rcnt, (void *)d_roff, (void *)d_rcur, (void *)d_rev})
    if (p) (void)hipFree(p);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return err;
}

// rq_dists over n_pairs pairs of host rows on `device` (hs_debug_rq_raw_dist)
hipError_t gpu_rq_raw_dist(const float *a, const float *b, size_t n_pairs, uint32_t dim, int metric, int device, float *out) {
  hipError_t err = hipSuccess;
  const uint32_t dpad = (dim + 3u) & ~3u;
  const size_t lds = (size_t)dpad * 4 + 64, bytes = n_pairs * dim * 4;
  if (dim == 0 || lds > 64 * 1024 || n_pairs > 0x7FFFFFF0u) return hipErrorInvalidValue;
  if (n_pairs == 0) return hipSuccess;
  float *d_a = nullptr, *d_b = nullptr, *d_o = nullptr;
  BG_TRY(hipSetDevice(device));
  BG_TRY(hipMalloc((void **)&d_a, bytes));
  BG_TRY(hipMalloc((void **)&d_b, bytes));
  BG_TRY(hipMalloc((void **)&d_o, n_pairs * 4));
  BG_TRY(hipMemcpy(d_a, a, bytes, hipMemcpyHostToDevice));
  BG_TRY(hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice));
  if (metric == METRIC_L2)
    hipLaunchKernelGGL(rq_dist_debug_kernel<METRIC_L2>, dim3((uint32_t)std::min<size_t>(n_pairs, 4096)), dim3(64), lds, nullptr, d_a, d_b, (uint32_t)n_pairs, dim, dpad, d_o);
  else
    hipLaunchKernelGGL(rq_dist_debug_kernel<METRIC_IP>, dim3((uint32_t)std::min<size_t>(n_pairs, 4096)), dim3(64), lds, nullptr, d_a, d_b, (uint32_t)n_pairs, dim, dpad, d_o);
  BG_TRY(hipGetLastError());
  BG_TRY(hipMemcpy(out, d_o, n_pairs * 4, hipMemcpyDeviceToHost));
done:
  for (void *p : {(void *)d_a, (void *)d_b, (void *)d_o})
    if (p) (void)hipFree(p);
  return err;
}

// gpu_batch_build's batches continued on a resident index: the rows are the index's own array (the new ones copied behind the old --
// no list names them until a batch has run, so no search sees them), the lists are seeded from the host image, and what comes back
// is one dense buffer of the changed old slots and the new nodes' slots.
hipError_t gpu_batch_add(const GpuAddInput &in, int device, GpuAddOutput &out) {
  hipError_t err = hipSuccess;
  const uint32_t scratch_ids = in.scratch_ids ? in.scratch_ids : kBgScratchIds;
  out = GpuAddOutput();
  if (!gpu_build_supported(in.dim, in.M, in.efc, scratch_ids) || in.maxM != in.M || in.maxM0 != 2 * in.M || in.n0 == 0 || in.count == 0 ||
      (uint64_t)in.n0 + in.count > 0x7FFFFFF0u || !in.d_vec || !in.rows || !in.lev || !in.steps || !in.upb || !in.lists0 || !in.lists_up)
    return hipErrorInvalidValue;
  const uint32_t n0 = in.n0, n = in.n0 + in.count;
  const std::vector<uint32_t> &upb = *in.upb;
  BgDev g{};
  g.n = n; g.dim = in.dim; g.dpad = (in.dim + 3u) & ~3u; g.M = in.M; g.maxM = in.maxM; g.maxM0 = in.maxM0;
  g.s0 = in.maxM0 + 1; g.su = in.maxM + 1; g.efc = in.efc; g.topcap = bg_topcap(in.efc);
  if (upb.size() != (size_t)n + 1 || in.lists0->size() != (size_t)n * g.s0 || in.lists_up->size() != (size_t)upb[n] * g.su) return hipErrorInvalidValue;
  const uint32_t nup = upb[n], nup0 = upb[n0], nold = n0 + nup0, nw = (nold + 63u) / 64u;
  std::vector<uint32_t> up_node(nup), up_level(nup);
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t l = 1; l <= in.lev[i]; l++) { up_node[upb[i] + l - 1] = i; up_level[upb[i] + l - 1] = l; }
  uint32_t max_batch = 1;
  size_t rev_cap = 1;   // the most edges one batch can add: M per (row, level it is searched on)
  for (const BatchStep &s : *in.steps) {
    if (s.begin < n0 || (uint64_t)s.begin + s.size > n || s.ep >= s.begin || s.top < 0) return hipErrorInvalidValue;
    max_batch = std::max(max_batch, s.size);
    size_t edges = 0;
    for (uint32_t k = 0; k < s.size; k++) edges += (size_t)in.M * (std::min<int64_t>(in.lev[s.begin + k], s.top) + 1);
    rev_cap = std::max(rev_cap, edges);
  }
  if (rev_cap > 0xFFFFFFF0u) return hipErrorInvalidValue;
  const size_t ntasks = (size_t)n + nup;
  const size_t gstride = (((size_t)n + 31) / 32 + 1) / 2 * 2 + 2 * (size_t)n;   // words: bitmap (padded to a pair's alignment) + n pairs
  const uint32_t nnew_slots = in.count + (nup - nup0);
  uint32_t *d_l0 = nullptr, *d_lu = nullptr, *d_upb = nullptr, *d_lev = nullptr, *d_upnode = nullptr, *d_uplevel = nullptr, *d_flagged = nullptr,
           *d_ctr = nullptr, *d_scratch = nullptr, *d_rcnt = nullptr, *d_roff = nullptr, *d_rcur = nullptr, *d_rev = nullptr, *d_counts = nullptr,
           *d_ids = nullptr, *d_out = nullptr;
  uint8_t *d_mark = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint32_t ctr[3] = {0, 0, 0};   // flagged rows of the batch, of the call; changed old tasks
  uint32_t nchg = 0, nslots = 0;
  BG_TRY(hipSetDevice(device));
  BG_TRY(hipMalloc((void **)&d_l0, (size_t)n * g.s0 * 4));
  BG_TRY(hipMalloc((void **)&d_lu, std::max<size_t>((size_t)nup * g.su, 1) * 4));
  BG_TRY(hipMalloc((void **)&d_upb, ((size_t)n + 1) * 4));
  BG_TRY(hipMalloc((void **)&d_lev, (size_t)n * 4));
  BG_TRY(hipMalloc((void **)&d_upnode, std::max<size_t>(nup, 1) * 4));
  BG_TRY(hipMalloc((void **)&d_uplevel, std::max<size_t>(nup, 1) * 4));
  BG_TRY(hipMalloc((void **)&d_flagged, (size_t)max_batch * 4));
  BG_TRY(hipMalloc((void **)&d_ctr, 12));
  BG_TRY(hipMalloc((void **)&d_scratch, gstride * 4 * std::min(kBgRerunGrid, max_batch)));
  BG_TRY(hipMalloc((void **)&d_rcnt, ntasks * 4));
  BG_TRY(hipMalloc((void **)&d_roff, ntasks * 4));
  BG_TRY(hipMalloc((void **)&d_rcur, ntasks * 4));
  BG_TRY(hipMalloc((void **)&d_rev, rev_cap * 4));
  BG_TRY(hipMalloc((void **)&d_mark, nold));
  BG_TRY(hipMalloc((void **)&d_counts, (size_t)nw * 4));
  BG_TRY(hipMalloc((void **)&d_ids, (size_t)nold * 4));
  BG_TRY(hipMemcpy(in.d_vec + (size_t)n0 * in.dim, in.rows, (size_t)in.count * in.dim * 4, hipMemcpyHostToDevice));
  BG_TRY(hipMemcpy(d_l0, in.lists0->data(), (size_t)n * g.s0 * 4, hipMemcpyHostToDevice));
  if (nup) {
    BG_TRY(hipMemcpy(d_lu, in.lists_up->data(), (size_t)nup * g.su * 4, hipMemcpyHostToDevice));
    BG_TRY(hipMemcpy(d_upnode, up_node.data(), (size_t)nup * 4, hipMemcpyHostToDevice));
    BG_TRY(hipMemcpy(d_uplevel, up_level.data(), (size_t)nup * 4, hipMemcpyHostToDevice));
  }
  BG_TRY(hipMemcpy(d_upb, upb.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
  BG_TRY(hipMemcpy(d_lev, in.lev, (size_t)n * 4, hipMemcpyHostToDevice));
  BG_TRY(hipMemset(d_rcnt, 0, ntasks * 4));
  BG_TRY(hipMemset(d_roff, 0, ntasks * 4));
  BG_TRY(hipMemset(d_rcur, 0, ntasks * 4));
  BG_TRY(hipMemset(d_ctr, 0, 12));
  BG_TRY(hipMemset(d_mark, 0, nold));
  BG_TRY(hipDeviceSynchronize());
  g.vec = in.d_vec; g.l0 = d_l0; g.lu = d_lu; g.upb = d_upb; g.lev = d_lev;
  {
    const BgMarks marks{d_mark, n0, nup0};
    BG_TRY(hipEventCreate(&e0)); BG_TRY(hipEventCreate(&e1));
    BG_TRY(hipEventRecord(e0, nullptr));
    if (in.metric == METRIC_L2)
      BG_TRY(bg_run<METRIC_L2>(*in.steps, g, upb, scratch_ids, d_flagged, d_ctr, d_scratch, gstride, d_rcnt, d_roff, d_rcur, d_rev, (uint32_t)rev_cap, d_upnode, d_uplevel, nullptr, &marks));
    else
      BG_TRY(bg_run<METRIC_IP>(*in.steps, g, upb, scratch_ids, d_flagged, d_ctr, d_scratch, gstride, d_rcnt, d_roff, d_rcur, d_rev, (uint32_t)rev_cap, d_upnode, d_uplevel, nullptr, &marks));
    hipLaunchKernelGGL(bga_count_kernel, dim3((nw + 3) / 4), dim3(256), 0, nullptr, d_mark, nold, d_counts);
    hipLaunchKernelGGL(bga_scan_kernel, dim3(1), dim3(256), 0, nullptr, d_counts, nw, d_ctr + 2);
    hipLaunchKernelGGL(bga_scatter_kernel, dim3((nw + 3) / 4), dim3(256), 0, nullptr, d_mark, nold, n0, n, d_counts, d_ids);
    BG_TRY(hipGetLastError());
    BG_TRY(hipMemcpy(ctr, d_ctr, 12, hipMemcpyDeviceToHost));
    nchg = std::min(ctr[2], nold);
    nslots = nchg + nnew_slots;
    BG_TRY(hipMalloc((void **)&d_out, ((size_t)nslots * g.s0 + std::max(nchg, 1u)) * 4));
    hipLaunchKernelGGL(bga_gather_kernel, dim3((nslots + 3) / 4), dim3(256), 0, nullptr, g, d_ids, nchg, n0, nup0, nup, nslots, d_out);
    BG_TRY(hipGetLastError());
    BG_TRY(hipEventRecord(e1, nullptr));
    BG_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    BG_TRY(hipEventElapsedTime(&ms, e0, e1));
    out.kernel_ms = ms;
  }
  out.flagged_rows = ctr[1];
  {
    std::vector<uint32_t> buf((size_t)nslots * g.s0 + nchg);
    BG_TRY(hipMemcpy(buf.data(), d_out, buf.size() * 4, hipMemcpyDeviceToHost));   // the one download
    out.tasks.assign(buf.begin() + (size_t)nslots * g.s0, buf.end());
    buf.resize((size_t)nslots * g.s0);
    out.slots.swap(buf);
  }
done:
  for (void *p : {(void *)d_l0, (void *)d_lu, (void *)d_upb, (void *)d_lev, (void *)d_upnode, (void *)d_uplevel, (void *)d_flagged, (void *)d_ctr,
                  (void *)d_scratch, (void *)d_rcnt, (void *)d_roff, (void *)d_rcur, (void *)d_rev, (void *)d_mark, (void *)d_counts, (void *)d_ids,
                  (void *)d_out})
    if (p) (void)hipFree(p);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return err;
}

}  // namespace hs
