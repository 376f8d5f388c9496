// convert_diff.hip -- the list passes of HierarchicalNSWSlim::convertFromHNSWWithDiff on gfx950 (hnswalg_slim.h:1189-1303), the
// conversion a server runs after every batch of addPoint calls before it ships the difference to its clients (genPatch).  Not
// convertFromHNSW with a compare behind it: both prunes are hnsw->getNeighborsByHeuristic2 (hnswalg.h:481-523), whose candidate
// order, tie rule and output order are its own (diff_prune.hpp).  One wavefront per (node, level) list, as convert_gpu.hip, and
// the same distance recipes; the rows are read where they already are, in the resident HNSW index's fp32 array.
//   phase 1  every source list below its degree budget passes as it is; any other is ordered by (distance ascending, id
//            descending) -- a total order, so a rank sort by the whole wave serves every size up to 64 -- and goes through the
//            keep loop (sequential in the candidates, the kept set tested in parallel).  Only the kept SET matters: phase 3
//            sorts by id.
//   phase 2  reverse edges: convert_gpu.hip's two kernels.
//   phase 3  own list + reverse edges sorted by id, duplicates removed; a union above its level's capacity is ordered the same
//            way (bitonic sort in LDS, up to 2048 ids), pruned to the capacity, and stored in the POP order of the heap the
//            heuristic returns: descending distance, and where two kept entries are at the same distance the push_heap /
//            pop_heap mechanics of libstdc++ on one lane (heap_emul.hpp).  The list holds every kept entry (the reference pops
//            `limit` entries whatever was kept, which reads an empty queue when fewer were).
// The pruned and final lists have `keep` slots per task (ConvertInput::keep, 32 or 64), which these kernels take as an argument;
// kept / keptd / kd in LDS hold as many entries.  (convert_gpu.hip's kernels, whose names and registers are pinned, take it as a
// template parameter instead.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "convert_common.hpp"
#include "convert_engine.hpp"
#include "diff_prune.hpp"

namespace hs {

static constexpr uint32_t kCdPad = 0xFFFFFFFFu;   // id of a padding entry of the bitonic sort: behind every candidate

// ---- phase 1 (hnswalg_slim.h:1189-1232) -----------------------------------------------------------------------------------------
template <int METRIC>
__global__ void __launch_bounds__(64) cd_prune_kernel(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_off,
                                                      const uint32_t *t_size, const uint32_t *t_mlim, const uint32_t *lists, uint32_t ntasks,
                                                      uint32_t keep, uint32_t *out_nn, uint32_t *out_cnt) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  float *qc = qv + dim;
  uint32_t *nid = reinterpret_cast<uint32_t *>(qc + dim);
  float *nd = reinterpret_cast<float *>(nid + kCvMaxList);
  Pair *arr = reinterpret_cast<Pair *>(nd + kCvMaxList);
  uint32_t *kept = reinterpret_cast<uint32_t *>(arr + kCvMaxList);
  float *keptd = reinterpret_cast<float *>(kept + keep);
  float *kd = keptd + keep;
  const int lane = threadIdx.x;
  for (uint32_t t = blockIdx.x; t < ntasks; t += gridDim.x) {
    const uint32_t v = t_node[t], sz = min(t_size[t], kCvMaxList), mlim = min(t_mlim[t], keep);
    wave_sync();
    if ((uint32_t)lane < sz) nid[lane] = lists[t_off[t] + lane];
    if (sz < mlim) {   // `if (top_candidates.size() < M) return;` (hnswalg.h:484-486)
      if ((uint32_t)lane < sz) out_nn[(size_t)t * keep + lane] = nid[lane];   // sz < mlim <= keep <= 64: one lane per entry
      if (lane == 0) out_cnt[t] = sz;
      continue;
    }
    for (uint32_t i = lane; i < dim; i += 64) qv[i] = vec[(size_t)v * dim + i];
    wave_sync();
    cv_dists<METRIC>(vec, dim, qv, nid, nd, sz, lane);
    wave_sync();
    {
      const bool act = (uint32_t)lane < sz;
      const Pair mine{act ? nd[lane] : 0.f, act ? nid[lane] : 0u};
      uint32_t rank = 0;
      for (uint32_t i = 0; i < sz; i++) rank += h2_before(Pair{nd[i], nid[i]}, mine) ? 1u : 0u;
      if (act) arr[rank] = mine;
    }
    wave_sync();
    const uint32_t kc = cv_prune<METRIC>(vec, dim, arr, sz, mlim, qc, kept, kd, lane, keptd);
    if ((uint32_t)lane < kc) out_nn[(size_t)t * keep + lane] = kept[lane];
    if (lane == 0) out_cnt[t] = kc;
  }
}

// ---- phase 3 (hnswalg_slim.h:1264-1307) -----------------------------------------------------------------------------------------
// flags[0]: lists outside the on-chip buffers (the host redoes the conversion), flags[1]: lists that were re-pruned
template <int METRIC>
__global__ void __launch_bounds__(64) cd_union_kernel(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_limit,
                                                      const uint32_t *nn, const uint32_t *cnt, const uint32_t *roff, const uint32_t *rcnt,
                                                      const uint32_t *rev, uint32_t ntasks, uint32_t keep, uint32_t *fin, uint32_t *fin_cnt,
                                                      uint32_t *flags) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  float *qc = qv + dim;
  uint32_t *ids = reinterpret_cast<uint32_t *>(qc + dim);
  float *nd = reinterpret_cast<float *>(ids + kCvUnionCap);
  Pair *arr = reinterpret_cast<Pair *>(nd + kCvUnionCap);
  uint32_t *kept = reinterpret_cast<uint32_t *>(arr + kCvUnionCap);
  float *keptd = reinterpret_cast<float *>(kept + keep);
  float *kd = keptd + keep;
  const int lane = threadIdx.x;
  for (uint32_t t = blockIdx.x; t < ntasks; t += gridDim.x) {
    const uint32_t m1 = min(cnt[t], keep), r = rcnt[t], total = m1 + r, limit = t_limit[t];
    wave_sync();
    if (total > kCvUnionCap) {
      if (lane == 0) { atomicAdd(flags, 1u); fin_cnt[t] = 0; }
      continue;
    }
    uint32_t N = 64;
    while (N < total) N <<= 1;
    for (uint32_t i = lane; i < N; i += 64)
      ids[i] = i < m1 ? nn[(size_t)t * keep + i] : (i < total ? rev[roff[t] + (i - m1)] : 0xFFFFFFFFu);
    wave_sync();
    for (uint32_t k = 2; k <= N; k <<= 1)   // std::sort of plain ids (:1269): any correct sort gives the same array
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t i = lane; i < N; i += 64) {
          const uint32_t p = i ^ j;
          if (p > i) {
            const uint32_t a = ids[i], b = ids[p];
            const bool up = (i & k) == 0;
            if ((a > b) == up) { ids[i] = b; ids[p] = a; }
          }
        }
        wave_sync();
      }
    uint32_t m = 0;   // std::unique (:1273)
    for (uint32_t base = 0; base < total; base += 64) {
      const uint32_t i = base + lane;
      const uint32_t x = i < total ? ids[i] : 0u;
      const bool first = i < total && (i == 0 || ids[i - 1] != x);
      const unsigned long long fm = hs_ballot(first);
      wave_sync();
      if (first) ids[m + __popcll(fm & ((1ull << lane) - 1ull))] = x;   // m + prefix <= i: never overwrites an unread entry of a later chunk
      m += __popcll(fm);
      wave_sync();
    }
    if (m <= limit) {   // not re-pruned: ascending id (:1305-1307)
      if (m <= keep) {   // (keep <= 64: one lane per entry, here and below)
        if ((uint32_t)lane < m) fin[(size_t)t * keep + lane] = ids[lane];
        if (lane == 0) fin_cnt[t] = m;
      } else if (lane == 0) { atomicAdd(flags, 1u); fin_cnt[t] = 0; }   // capacity above `keep` ids: host path
      continue;
    }
    const uint32_t v = t_node[t];
    for (uint32_t i = lane; i < dim; i += 64) qv[i] = vec[(size_t)v * dim + i];
    wave_sync();
    cv_dists<METRIC>(vec, dim, qv, ids, nd, m, lane);
    wave_sync();
    uint32_t N2 = 64;
    while (N2 < m) N2 <<= 1;
    for (uint32_t i = lane; i < N2; i += 64) arr[i] = i < m ? Pair{nd[i], ids[i]} : Pair{0.f, kCdPad};
    wave_sync();
    for (uint32_t k = 2; k <= N2; k <<= 1)   // candidate order (diff_prune.hpp); padding entries last
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t i = lane; i < N2; i += 64) {
          const uint32_t p = i ^ j;
          if (p > i) {
            const Pair a = arr[i], b = arr[p];
            const bool a_after_b = b.id != kCdPad && (a.id == kCdPad || h2_before(b, a));
            const bool up = (i & k) == 0;
            if (a_after_b == up) { arr[i] = b; arr[p] = a; }
          }
        }
        wave_sync();
      }
    const uint32_t kc = cv_prune<METRIC>(vec, dim, arr, m, min(limit, keep), qc, kept, kd, lane, keptd);
    // pop order of the returned heap: kept order is ascending distance, so without equal distances it is the kept order reversed
    const bool eq = (uint32_t)lane + 1 < kc && keptd[lane] == keptd[lane + 1];
    if (hs_ballot(eq) == 0) {
      if ((uint32_t)lane < kc) fin[(size_t)t * keep + lane] = kept[kc - 1 - lane];
    } else {
      if ((uint32_t)lane < kc) arr[lane] = Pair{keptd[lane], kept[lane]};
      wave_sync();
      if (lane == 0) h2_pop_order(arr, (long)kc);
      wave_sync();
      if ((uint32_t)lane < kc) fin[(size_t)t * keep + lane] = arr[kc - 1 - lane].id;
    }
    if (lane == 0) { fin_cnt[t] = kc; atomicAdd(flags + 1, 1u); }
  }
}

// ---- the diff (hnswalg_slim.h:1309-1378) ------------------------------------------------------------------------------------------
// One wavefront per node: its final lists through the hierarchical filter (:1309-1330), level by level against the resident Slim
// index's own lists -- the level-0 tile row, the upper-level CSR slices -- counts and ids in order, which is the memcmp of
// :1369-1371 without a second copy of the old graph; and its row and label in the Slim index against the HNSW index's.
// flags[i]: bit 0 some level differs, bit 1 the node has neighbours, bit 2 row or label differs (or the node is beyond the previous
// count, whose slots count as empty).
__global__ void __launch_bounds__(256) cd_diff_kernel(const uint32_t *fin, const uint32_t *fin_cnt, uint32_t fstride, const uint32_t *levels,
                                                      const uint32_t *upb, uint32_t n, uint32_t prev, int32_t thr, const uint32_t *s_tile0, uint32_t stride,
                                                      const uint32_t *s_up_base, const uint32_t *s_up_ptr, uint32_t n_up, const uint32_t *s_cols,
                                                      const uint64_t *s_labels, const uint64_t *h_labels, const float *s_vec, const float *h_vec,
                                                      uint32_t dim, uint8_t *flags) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (i >= n) return;
  const uint32_t L = levels[i];
  const bool old = i < prev;
  const uint32_t ub = old ? s_up_base[i] : 0xFFFFFFFFu;
  bool changed = false;
  uint32_t total = 0;
  for (uint32_t l = 0; l <= L; l++) {
    const uint32_t t = cv_task_of(i, l, n, upb);
    const uint32_t cnt = min(fin_cnt[t], fstride);   // fstride = the call's slots per task <= 64: one lane per entry of a final list
    const uint32_t my = lane < cnt ? fin[(size_t)t * fstride + lane] : 0xFFFFFFFFu;
    const bool keep = lane < cnt && ((int32_t)l == thr || (my < n && levels[my] == l));
    const unsigned long long km = hs_ballot(keep);
    const uint32_t nk = __popcll(km), pos = __popcll(km & ((1ull << lane) - 1ull));
    const uint32_t *optr = nullptr;
    uint32_t ocnt = 0;
    if (old && l == 0) {
      optr = s_tile0 + (size_t)i * stride;
      ocnt = __popcll(hs_ballot(lane < stride && optr[lane] != 0xFFFFFFFFu));   // the row is packed at the front, padded behind
    } else if (old && ub != 0xFFFFFFFFu) {
      if (ub + l >= n_up) { changed = true; total += nk; continue; }   // (a Slim node with fewer levels than the HNSW node: never equal)
      const uint32_t s = s_up_ptr[ub + l - 1], e = s_up_ptr[ub + l];
      optr = s_cols + s;
      ocnt = e - s;
    }
    if (nk != ocnt) changed = true;
    else if (hs_ballot(keep && optr[pos] != my) != 0) changed = true;
    total += nk;
  }
  bool stale = !old;
  if (old) {
    bool d = lane == 0 && s_labels[i] != h_labels[i];
    const uint32_t *a = reinterpret_cast<const uint32_t *>(s_vec + (size_t)i * dim), *b = reinterpret_cast<const uint32_t *>(h_vec + (size_t)i * dim);
    for (uint32_t c = lane; c < dim; c += 64) d = d || a[c] != b[c];
    stale = hs_ballot(d) != 0;
  }
  if (lane == 0) flags[i] = (uint8_t)((changed ? 1u : 0u) | (total ? 2u : 0u) | (stale ? 4u : 0u));
}

// membership of node i in list k (0 changed old, 1 new, 2 image changed, 3 row or label changed) from its flag byte
__device__ __forceinline__ bool cd_member(uint32_t k, uint32_t f, bool old) {
  return k == 0 ? old && (f & 3u) == 3u : k == 1 ? !old && (f & 2u) != 0 : k == 2 ? !old || (f & 5u) != 0 : !old || (f & 4u) != 0;
}
// Compaction in ascending id: one wavefront per 64 consecutive nodes counts its members of each list (ballot + popcount), one
// workgroup turns the counts into offsets, and the wavefronts write their members behind their offset at their rank in the ballot.
__global__ void __launch_bounds__(256) cd_count_kernel(const uint8_t *flags, uint32_t n, uint32_t prev, uint32_t *counts /* nw x 4 */) {
  const uint32_t lane = threadIdx.x & 63u, w = blockIdx.x * 4u + (threadIdx.x >> 6), i = w * 64u + lane;
  if (w * 64u >= n) return;
  const uint32_t f = i < n ? flags[i] : 0u;
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t c = __popcll(hs_ballot(i < n && cd_member(k, f, i < prev)));
    if (lane == k) counts[(size_t)w * 4 + k] = c;
  }
}
__global__ void __launch_bounds__(256) cd_scan_kernel(uint32_t *counts, uint32_t nw, uint32_t *totals /* 4 */) {
  __shared__ uint32_t part[256][4];
  const uint32_t t = threadIdx.x, per = (nw + 255u) / 256u, lo = min(nw, t * per), hi = min(nw, lo + per);
  uint32_t sum[4] = {0, 0, 0, 0};
  for (uint32_t w = lo; w < hi; w++)
    for (uint32_t k = 0; k < 4; k++) sum[k] += counts[(size_t)w * 4 + k];
  for (uint32_t k = 0; k < 4; k++) part[t][k] = sum[k];
  __syncthreads();
  if (t < 4) {
    uint32_t run = 0;
    for (uint32_t j = 0; j < 256; j++) { const uint32_t c = part[j][t]; part[j][t] = run; run += c; }
    totals[t] = run;
  }
  __syncthreads();
  for (uint32_t k = 0; k < 4; k++) sum[k] = part[t][k];
  for (uint32_t w = lo; w < hi; w++)
    for (uint32_t k = 0; k < 4; k++) { const uint32_t c = counts[(size_t)w * 4 + k]; counts[(size_t)w * 4 + k] = sum[k]; sum[k] += c; }
}
// out: four arrays of n ids each, list k at out + k * n
__global__ void __launch_bounds__(256) cd_scatter_kernel(const uint8_t *flags, uint32_t n, uint32_t prev, const uint32_t *offs, uint32_t *out) {
  const uint32_t lane = threadIdx.x & 63u, w = blockIdx.x * 4u + (threadIdx.x >> 6), i = w * 64u + lane;
  if (w * 64u >= n) return;
  const uint32_t f = i < n ? flags[i] : 0u;
  for (uint32_t k = 0; k < 4; k++) {
    const bool m = i < n && cd_member(k, f, i < prev);
    const unsigned long long bm = hs_ballot(m);
    const uint32_t at = offs[(size_t)w * 4 + k] + __popcll(bm & ((1ull << lane) - 1ull));
    if (m && at < n) out[(size_t)k * n + at] = i;
  }
}

// ---- host driver ------------------------------------------------------------------------------------------------------------------
#define CD_TRY(expr)                        \
  do {                                      \
    hipError_t _e = (expr);                 \
    if (_e != hipSuccess) { err = _e; goto done; } \
  } while (0)

template <typename T>
static hipError_t cd_upload(T **dp, const std::vector<T> &v) {
  hipError_t e = hipMalloc((void **)dp, std::max<size_t>(v.size(), 1) * sizeof(T));
  if (e != hipSuccess) return e;
  return v.empty() ? hipSuccess : hipMemcpy(*dp, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

hipError_t gpu_convert_diff_lists(const ConvertInput &in, const float *d_vec, int device, std::vector<uint32_t> &fin, std::vector<uint32_t> &fin_cnt,
                                  bool &needs_host, uint32_t &n_reprune, double *kernel_ms, DiffDev *diff) {
  hipError_t err = hipSuccess;
  needs_host = false;
  n_reprune = 0;
  const uint32_t nt = (uint32_t)in.t_node.size();
  uint32_t *d_node = nullptr, *d_off = nullptr, *d_size = nullptr, *d_mlim = nullptr, *d_limit = nullptr, *d_level = nullptr, *d_lists = nullptr,
           *d_upb = nullptr, *d_nn = nullptr, *d_cnt = nullptr, *d_rcnt = nullptr, *d_roff = nullptr, *d_rcur = nullptr, *d_rev = nullptr,
           *d_fin = nullptr, *d_fcnt = nullptr, *d_flags = nullptr, *d_lev = nullptr, *d_counts = nullptr, *d_tot = nullptr, *d_ids = nullptr;
  uint8_t *d_nf = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<uint32_t> rcnt(nt), roff(nt + 1, 0);
  uint32_t flags[2] = {0, 0};
  bool timed = false;
  const uint32_t keep = in.keep;   // slots per task of nn / fin, entries of kept / keptd / kd in LDS
  const size_t lds1 = (size_t)in.dim * 8 + kCvMaxList * 16 + keep * 12;
  const size_t lds3 = (size_t)in.dim * 8 + (size_t)kCvUnionCap * 16 + keep * 12;
  const uint32_t grid = 256 * 16;
  if (nt == 0) return hipSuccess;
  if (!d_vec) return hipErrorInvalidDevicePointer;
  if (keep != 32 && keep != kCvMaxKeep) return hipErrorInvalidValue;
  if (lds3 > 160 * 1024) { needs_host = true; return hipSuccess; }   // rows too long for the on-chip buffers
  CD_TRY(hipSetDevice(device));
  CD_TRY(cd_upload(&d_node, in.t_node)); CD_TRY(cd_upload(&d_off, in.t_off)); CD_TRY(cd_upload(&d_size, in.t_size));
  CD_TRY(cd_upload(&d_mlim, in.t_mlim)); CD_TRY(cd_upload(&d_limit, in.t_limit)); CD_TRY(cd_upload(&d_level, in.t_level));
  CD_TRY(cd_upload(&d_lists, in.lists)); CD_TRY(cd_upload(&d_upb, in.upb));
  CD_TRY(hipMalloc((void **)&d_nn, (size_t)nt * keep * 4)); CD_TRY(hipMalloc((void **)&d_cnt, (size_t)nt * 4));
  CD_TRY(hipMalloc((void **)&d_rcnt, (size_t)nt * 4)); CD_TRY(hipMalloc((void **)&d_roff, (size_t)(nt + 1) * 4)); CD_TRY(hipMalloc((void **)&d_rcur, (size_t)nt * 4));
  CD_TRY(hipMalloc((void **)&d_fin, (size_t)nt * keep * 4)); CD_TRY(hipMalloc((void **)&d_fcnt, (size_t)nt * 4)); CD_TRY(hipMalloc((void **)&d_flags, 8));
  CD_TRY(hipMemset(d_rcnt, 0, (size_t)nt * 4)); CD_TRY(hipMemset(d_rcur, 0, (size_t)nt * 4)); CD_TRY(hipMemset(d_flags, 0, 8));
  CD_TRY(hipEventCreate(&e0)); CD_TRY(hipEventCreate(&e1));
  if (lds3 > 64 * 1024) {
    CD_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(in.metric == METRIC_L2 ? cd_union_kernel<METRIC_L2> : cd_union_kernel<METRIC_IP>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
  }
  if (lds1 > 64 * 1024) {
    CD_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(in.metric == METRIC_L2 ? cd_prune_kernel<METRIC_L2> : cd_prune_kernel<METRIC_IP>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
  }
  CD_TRY(hipEventRecord(e0, nullptr));
  if (in.metric == METRIC_L2) hipLaunchKernelGGL(cd_prune_kernel<METRIC_L2>, dim3(std::min(grid, nt)), dim3(64), lds1, nullptr, d_vec, in.dim, d_node, d_off, d_size, d_mlim, d_lists, nt, keep, d_nn, d_cnt);
  else hipLaunchKernelGGL(cd_prune_kernel<METRIC_IP>, dim3(std::min(grid, nt)), dim3(64), lds1, nullptr, d_vec, in.dim, d_node, d_off, d_size, d_mlim, d_lists, nt, keep, d_nn, d_cnt);
  CD_TRY(hipGetLastError());
  CD_TRY(launch_cv_rev_count(d_nn, d_cnt, d_level, d_upb, in.n, nt, keep, d_rcnt));
  CD_TRY(hipMemcpy(rcnt.data(), d_rcnt, (size_t)nt * 4, hipMemcpyDeviceToHost));
  for (uint32_t t = 0; t < nt; t++) roff[t + 1] = roff[t] + rcnt[t];
  CD_TRY(hipMemcpy(d_roff, roff.data(), (size_t)(nt + 1) * 4, hipMemcpyHostToDevice));
  CD_TRY(hipMalloc((void **)&d_rev, std::max<size_t>(roff[nt], 1) * 4));
  CD_TRY(launch_cv_rev_fill(d_nn, d_cnt, d_node, d_level, d_upb, in.n, nt, keep, d_roff, d_rcur, d_rev));
  if (in.metric == METRIC_L2) hipLaunchKernelGGL(cd_union_kernel<METRIC_L2>, dim3(std::min(grid, nt)), dim3(64), lds3, nullptr, d_vec, in.dim, d_node, d_limit, d_nn, d_cnt, d_roff, d_rcnt, d_rev, nt, keep, d_fin, d_fcnt, d_flags);
  else hipLaunchKernelGGL(cd_union_kernel<METRIC_IP>, dim3(std::min(grid, nt)), dim3(64), lds3, nullptr, d_vec, in.dim, d_node, d_limit, d_nn, d_cnt, d_roff, d_rcnt, d_rev, nt, keep, d_fin, d_fcnt, d_flags);
  CD_TRY(hipGetLastError());
  CD_TRY(hipMemcpy(flags, d_flags, 8, hipMemcpyDeviceToHost));
  needs_host = flags[0] != 0;
  n_reprune = flags[1];
  if (diff && !needs_host) {
    const uint32_t n = in.n, nw = (n + 63u) / 64u;
    uint32_t tot[4] = {0, 0, 0, 0};
    if (diff->levels.size() != n || !diff->s_tile0 || diff->s_stride == 0 || diff->s_stride > 64 || !diff->s_vec || diff->prev_count > n) { err = hipErrorInvalidValue; goto done; }
    CD_TRY(cd_upload(&d_lev, diff->levels));
    CD_TRY(hipMalloc((void **)&d_nf, n)); CD_TRY(hipMalloc((void **)&d_counts, (size_t)nw * 16)); CD_TRY(hipMalloc((void **)&d_tot, 16));
    CD_TRY(hipMalloc((void **)&d_ids, (size_t)n * 16));
    hipLaunchKernelGGL(cd_diff_kernel, dim3((n + 3) / 4), dim3(256), 0, nullptr, d_fin, d_fcnt, keep, d_lev, d_upb, n, diff->prev_count, diff->threshold_level,
                       diff->s_tile0, diff->s_stride, diff->s_up_base, diff->s_up_ptr, diff->n_up, diff->s_cols, diff->s_labels, diff->h_labels, diff->s_vec, d_vec,
                       in.dim, d_nf);
    CD_TRY(hipGetLastError());
    hipLaunchKernelGGL(cd_count_kernel, dim3((nw + 3) / 4), dim3(256), 0, nullptr, d_nf, n, diff->prev_count, d_counts);
    CD_TRY(hipGetLastError());
    hipLaunchKernelGGL(cd_scan_kernel, dim3(1), dim3(256), 0, nullptr, d_counts, nw, d_tot);
    CD_TRY(hipGetLastError());
    hipLaunchKernelGGL(cd_scatter_kernel, dim3((nw + 3) / 4), dim3(256), 0, nullptr, d_nf, n, diff->prev_count, d_counts, d_ids);
    CD_TRY(hipGetLastError());
    CD_TRY(hipEventRecord(e1, nullptr));   // (the diff and compaction kernels are inside kernel_ms)
    CD_TRY(hipEventSynchronize(e1));
    timed = true;
    CD_TRY(hipMemcpy(tot, d_tot, 16, hipMemcpyDeviceToHost));
    std::vector<uint32_t> *outs[4] = {&diff->old_ids, &diff->new_ids, &diff->dirty, &diff->stale};
    for (int k = 0; k < 4; k++) {
      if (tot[k] > n) { err = hipErrorUnknown; goto done; }
      outs[k]->resize(tot[k]);
      if (tot[k]) CD_TRY(hipMemcpy(outs[k]->data(), d_ids + (size_t)k * n, (size_t)tot[k] * 4, hipMemcpyDeviceToHost));
    }
    if (diff->want_flags) {
      diff->flags.resize(n);
      CD_TRY(hipMemcpy(diff->flags.data(), d_nf, n, hipMemcpyDeviceToHost));
    }
  }
  if (!timed) {
    CD_TRY(hipEventRecord(e1, nullptr));
    CD_TRY(hipEventSynchronize(e1));
  }
  if (kernel_ms) { float ms = 0.f; CD_TRY(hipEventElapsedTime(&ms, e0, e1)); *kernel_ms = ms; }
  fin.resize((size_t)nt * keep);
  fin_cnt.resize(nt);
  CD_TRY(hipMemcpy(fin.data(), d_fin, fin.size() * 4, hipMemcpyDeviceToHost));
  CD_TRY(hipMemcpy(fin_cnt.data(), d_fcnt, (size_t)nt * 4, hipMemcpyDeviceToHost));
done:
  for (void *p : {(void *)d_node, (void *)d_off, (void *)d_size, (void *)d_mlim, (void *)d_limit, (void *)d_level, (void *)d_lists, (void *)d_upb,
                  (void *)d_nn, (void *)d_cnt, (void *)d_rcnt, (void *)d_roff, (void *)d_rcur, (void *)d_rev, (void *)d_fin, (void *)d_fcnt, (void *)d_flags,
                  (void *)d_lev, (void *)d_nf, (void *)d_counts, (void *)d_tot, (void *)d_ids})
    if (p) (void)hipFree(p);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return err;
}

}  // namespace hs
