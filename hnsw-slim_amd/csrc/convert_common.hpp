// convert_common.hpp -- what the device conversions share (convert_gpu.hip: convertFromHNSW, convert_diff.hip:
// convertFromHNSWWithDiff, convert_slimq.hip: HierarchicalNSWSlimQ's convertFromHNSW): buffer sizes, the distances of one list, the
// by-distance std::sort, the keep loop of the pruning heuristics, the union's id sort, the task index, the reverse-edge kernels'
// launchers and the host driver of the three phases (kernels and driver live in convert_gpu.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "dist_recipe.hpp"
#include "heap_emul.hpp"
#include "wave_util.hpp"

namespace hs {

static constexpr uint32_t kCvMaxList = 64;     // a source list (level-0 list of the vanilla graph) holds at most this many ids
static constexpr uint32_t kCvMaxKeep = 64;     // pruned / final lists hold at most this many ids (every capacity and budget <= 64 .. see host check)
static constexpr uint32_t kCvUnionCap = 2048;  // own list + reverse edges of one (node, level), in LDS

// `keep` in the kernels and launchers below and in the .hip files is ConvertInput::keep (convert_engine.hpp): the slots per task of
// the pruned (nn) and final (fin) lists of one call and the entries of the kernels' kept / keptd / kd arrays in LDS, 32 or kCvMaxKeep.
// A wavefront handles a kept or final list with one lane per entry, which holds because keep <= 64.

// distances query (LDS, dim floats) -> rows nid[0..cnt) (LDS) into nd[0..cnt) (LDS)
template <int METRIC>
__device__ __forceinline__ void cv_dists(const float *vec, uint32_t dim, const float *qv, const uint32_t *nid, float *nd, uint32_t cnt, int lane) {
  if ((dim & 15u) == 0) {
    const int sub = lane & 3, grp = lane >> 2;
    const uint32_t steps = dim >> 4;
    const float4 *qq = reinterpret_cast<const float4 *>(qv) + sub;
    for (uint32_t base = 0; base < cnt; base += 16) {
      const uint32_t j = base + grp;
      const bool act = j < cnt;
      const uint32_t id = nid[act ? j : base];
      const float4 *row = reinterpret_cast<const float4 *>(vec + (size_t)id * dim) + sub;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (uint32_t r0 = 0; r0 < steps; r0 += 8) {
        const uint32_t nb = min(8u, steps - r0);
        float4 buf[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++)
          if (i < nb) buf[i] = row[(r0 + i) * 4];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++)
          if (i < nb) step4<METRIC>(acc, qq[(r0 + i) * 4], buf[i]);
      }
      bool owner;
      const float r = lane4_reduce<METRIC>(acc, sub, owner);
      if (act && owner) nd[j] = r;
    }
  } else {
    for (uint32_t base = 0; base < cnt; base += 64) {
      const uint32_t j = base + lane;
      if (j < cnt) {
        const float *row = vec + (size_t)nid[j] * dim;
        nd[j] = METRIC == METRIC_L2 ? l2_general(qv, row, dim) : ip_general(qv, row, dim);
      }
    }
  }
}

// cv_dists as a type: the default distance of cv_prune (build_gpu.hip's flavours are the others)
struct CvDists {
  template <int METRIC>
  static __device__ __forceinline__ void dists(const float *vec, uint32_t dim, const float *qv, const uint32_t *nid, float *nd, uint32_t cnt, int lane) {
    cv_dists<METRIC>(vec, dim, qv, nid, nd, cnt, lane);
  }
};

// by-distance std::sort of (nd[j], nid[j]), j < sz, into arr[]: rank sort when libstdc++'s result is the stable order (sz <= 16:
// pure insertion sort) or no two keys are equal; otherwise the step-for-step emulation on one lane
__device__ __forceinline__ void cv_sort_by_dist(const uint32_t *nid, const float *nd, uint32_t sz, Pair *arr, int lane) {
  if (sz <= 64) {
    const bool act = (uint32_t)lane < sz;
    const float my_d = act ? nd[lane] : 0.f;
    const uint32_t my_id = act ? nid[lane] : 0u;
    uint32_t rank = 0;
    bool tie = false;
    for (uint32_t i = 0; i < sz; i++) {
      const float di = nd[i];
      rank += (di < my_d || (di == my_d && i < (uint32_t)lane)) ? 1u : 0u;
      tie = tie || (di == my_d && i != (uint32_t)lane);
    }
    const bool anytie = hs_ballot(act && tie) != 0;
    if (sz <= 16 || !anytie) {
      if (act) arr[rank] = Pair{my_d, my_id};
      wave_sync();
      return;
    }
  }
  for (uint32_t i = lane; i < sz; i += 64) arr[i] = Pair{nd[i], nid[i]};
  wave_sync();
  if (lane == 0) (void)std_sort(arr, (long)sz, LessD());
  wave_sync();
}

// PruneByHeuristic (hnswalg_slim.h:836-865) over arr[0..sz) sorted ascending by distance: a candidate is kept unless a kept
// neighbour is closer to it than the node itself.  Sequential in the candidates, parallel over the kept set.  This is also the
// keep loop of getNeighborsByHeuristic2 (hnswalg.h:495-517) once arr[] is in ITS candidate order (diff_prune.hpp), and of
// rabitqlib's get_neighbors_by_heuristic2 (hnsw.hpp:1016-1054) with DIST its distance (build_gpu.hip).
template <int METRIC, class DIST = CvDists>
__device__ __forceinline__ uint32_t cv_prune(const float *vec, uint32_t dim, const Pair *arr, uint32_t sz, uint32_t mlim, float *qc /*LDS dim*/,
                                             uint32_t *kept, float *kd, int lane, float *keptd = nullptr) {
  uint32_t kc = 0;   // (kept / kd / keptd hold `keep` entries: the caller passes mlim <= keep)
  for (uint32_t t = 0; t < sz && kc < mlim; t++) {
    const float cd = unif(arr[t].d);
    const uint32_t cid = uni(arr[t].id);
    bool good = true;
    if (kc > 0) {
      for (uint32_t i = lane; i < dim; i += 64) qc[i] = vec[(size_t)cid * dim + i];
      wave_sync();
      DIST::template dists<METRIC>(vec, dim, qc, kept, kd, kc, lane);
      wave_sync();
      bool bad = false;
      for (uint32_t i = lane; i < kc; i += 64) bad = bad || kd[i] < cd;
      good = hs_ballot(bad) == 0;
    }
    if (good) {
      if (lane == 0) {
        kept[kc] = cid;
        if (keptd) keptd[kc] = cd;   // (convertFromHNSWWithDiff's re-prune: the kept distances, in kept order)
      }
      kc++;
    }
    wave_sync();
  }
  return kc;
}

// Phase 3's list of one task (hnswalg_slim.h:999-1012): own[0..m1) followed by rv[0..total - m1) gathered into ids[] (LDS,
// kCvUnionCap entries; the caller has checked total <= kCvUnionCap), sorted by id, duplicates removed.  Returns the entries left.
__device__ __forceinline__ uint32_t cv_union_ids(const uint32_t *own, uint32_t m1, const uint32_t *rv, uint32_t total, uint32_t *ids, int lane) {
  uint32_t N = 64;
  while (N < total) N <<= 1;
  for (uint32_t i = lane; i < N; i += 64)
    ids[i] = i < m1 ? own[i] : (i < total ? rv[i - m1] : 0xFFFFFFFFu);
  wave_sync();
  // bitonic sort ascending (std::sort of plain ids: equal keys are equal values, any correct sort gives the same array)
  for (uint32_t k = 2; k <= N; k <<= 1)
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
  // std::unique
  uint32_t m = 0;
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
  return m;
}

// (node u, level l) -> task index: level 0 = u, level l >= 1 = n + upb[u] + l - 1
__device__ __forceinline__ uint32_t cv_task_of(uint32_t u, uint32_t l, uint32_t n, const uint32_t *upb) { return l == 0 ? u : n + upb[u] + l - 1; }

// reverse edges (hnswalg_slim.h:988-998 / 1234-1241), counted then filled: nn / cnt = the pruned lists (`keep` ids per task, 32 or 64)
hipError_t launch_cv_rev_count(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_level, const uint32_t *upb, uint32_t n, uint32_t ntasks,
                               uint32_t keep, uint32_t *rcnt);
hipError_t launch_cv_rev_fill(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_node, const uint32_t *t_level, const uint32_t *upb, uint32_t n,
                              uint32_t ntasks, uint32_t keep, const uint32_t *roff, uint32_t *rcur, uint32_t *rev);

// The kernels of phase 1 (a task's source list -> its pruned list) and phase 3 (pruned list + reverse edges -> final list), as
// convert_gpu.hip and convert_slimq.hip define them, and the host driver of the three phases that launches a pair of them
// (convert_gpu.hip).  lds1 / lds3: dynamic LDS bytes of the two kernels.
typedef void (*CvPruneKernel)(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_off, const uint32_t *t_size,
                              const uint32_t *t_mlim, const uint32_t *lists, uint32_t ntasks, uint32_t *out_nn, uint32_t *out_cnt);
typedef void (*CvUnionKernel)(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_limit, const uint32_t *nn, const uint32_t *cnt,
                              const uint32_t *roff, const uint32_t *rcnt, const uint32_t *rev, uint32_t ntasks, uint32_t *fin, uint32_t *fin_cnt,
                              uint32_t *flags);
struct ConvertInput;
hipError_t cv_run_lists(const ConvertInput &in, int device, CvPruneKernel prune_k, CvUnionKernel union_k, size_t lds1, size_t lds3,
                        std::vector<uint32_t> &fin, std::vector<uint32_t> &fin_cnt, bool &needs_host, double *kernel_ms);

}  // namespace hs
