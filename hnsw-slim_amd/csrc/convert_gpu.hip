// convert_gpu.hip -- HierarchicalNSWSlim::convertFromHNSW on gfx950 (hnswalg_slim.h:867-1108, PruneByHeuristic :836-865):
// the step immediately before the search path.  The list-level work -- distances, the by-distance
// std::sort, the pruning heuristic, the reverse-edge union, the re-prune of over-full lists -- runs on the device, one
// wavefront per (node, level) list; the degree histograms / hub thresholds (:904-945) and the final assembly of the element
// array and blobs (hierarchical filter :1063-1084, offsets, labels, vectors) stay on the host (slim_convert_gpu.hpp), they are a
// few linear passes.  The output is the same bytes as the CPU harness SlimGraph::convert:
//   * distances by the same fp32 recipes as the search kernels (dist_recipe.hpp; 4 lanes per row for dim % 16 == 0, the
//     reference's SIMD4 / residual / scalar recipes one lane per row otherwise),
//   * std::sort by distance with libstdc++'s own tie behaviour: lists of <= 16 entries are an insertion sort (stable), done
//     as a rank sort by the whole wave; longer lists with equal keys run heap_emul.hpp's std_sort emulation on one lane,
//   * the reverse-edge lists are filled with atomics in any order and then sorted by id (as :1003-1011 does).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "convert_common.hpp"
#include "convert_engine.hpp"
#include "dist_recipe.hpp"
#include "heap_emul.hpp"
#include "wave_util.hpp"

namespace hs {

// Every kernel of this file exists once per stride of the pruned / final lists (ConvertInput::keep).  Its body is a device
// function with the stride as the template parameter KEEP; the kernel `name` runs it with 32 slots per task -- the kernel as it was
// before the 64-slot stride, same name, same code, so a call with every capacity and budget <= 32 launches what it always did and
// its lines of resource_usage.txt (pinned by tests/test_f32_free_cpu.py) stand -- and `name_wide` runs it with kCvMaxKeep = 64.

// ---- phase 1 (hnswalg_slim.h:951-986): every source list sorted by distance to its node and pruned to its degree budget ----
template <int METRIC, uint32_t KEEP>
__device__ __forceinline__ void cv_prune_tasks(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_off,
                                               const uint32_t *t_size, const uint32_t *t_mlim, const uint32_t *lists, uint32_t ntasks,
                                               uint32_t *out_nn, uint32_t *out_cnt) {
  constexpr uint32_t keep = KEEP;
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  float *qc = qv + dim;
  uint32_t *nid = reinterpret_cast<uint32_t *>(qc + dim);
  float *nd = reinterpret_cast<float *>(nid + kCvMaxList);
  Pair *arr = reinterpret_cast<Pair *>(nd + kCvMaxList);
  uint32_t *kept = reinterpret_cast<uint32_t *>(arr + kCvMaxList);
  float *kd = reinterpret_cast<float *>(kept + keep);
  const int lane = threadIdx.x;
  for (uint32_t t = blockIdx.x; t < ntasks; t += gridDim.x) {
    const uint32_t v = t_node[t], sz = t_size[t], mlim = t_mlim[t];
    wave_sync();
    for (uint32_t i = lane; i < dim; i += 64) qv[i] = vec[(size_t)v * dim + i];
    if ((uint32_t)lane < sz) nid[lane] = lists[t_off[t] + lane];
    wave_sync();
    cv_dists<METRIC>(vec, dim, qv, nid, nd, sz, lane);
    wave_sync();
    cv_sort_by_dist(nid, nd, sz, arr, lane);
    const uint32_t kc = cv_prune<METRIC>(vec, dim, arr, sz, mlim, qc, kept, kd, lane);
    if ((uint32_t)lane < kc) out_nn[(size_t)t * keep + lane] = kept[lane];   // kc <= mlim <= keep <= 64: one lane per kept entry
    if (lane == 0) out_cnt[t] = kc;
  }
}
template <int METRIC>
__global__ void __launch_bounds__(64) cv_prune_kernel(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_off,
                                                      const uint32_t *t_size, const uint32_t *t_mlim, const uint32_t *lists, uint32_t ntasks,
                                                      uint32_t *out_nn, uint32_t *out_cnt) {
  cv_prune_tasks<METRIC, 32>(vec, dim, t_node, t_off, t_size, t_mlim, lists, ntasks, out_nn, out_cnt);
}
template <int METRIC>
__global__ void __launch_bounds__(64) cv_prune_kernel_wide(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_off,
                                                           const uint32_t *t_size, const uint32_t *t_mlim, const uint32_t *lists, uint32_t ntasks,
                                                           uint32_t *out_nn, uint32_t *out_cnt) {
  cv_prune_tasks<METRIC, kCvMaxKeep>(vec, dim, t_node, t_off, t_size, t_mlim, lists, ntasks, out_nn, out_cnt);
}

// ---- phase 2 (hnswalg_slim.h:988-998): reverse edges, counted then filled ---------------------------------------------------
// one thread per slot of nn (the host keeps ntasks * KEEP below 2^32: make_convert_input)
template <uint32_t KEEP>
__device__ __forceinline__ void cv_rev_count_slot(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_level, const uint32_t *upb, uint32_t n,
                                                  uint32_t ntasks, uint32_t *rcnt) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t t = g / KEEP, i = g % KEEP;
  if (t >= ntasks || i >= cnt[t]) return;
  atomicAdd(&rcnt[cv_task_of(nn[(size_t)t * KEEP + i], t_level[t], n, upb)], 1u);
}
template <uint32_t KEEP>
__device__ __forceinline__ void cv_rev_fill_slot(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_node, const uint32_t *t_level,
                                                 const uint32_t *upb, uint32_t n, uint32_t ntasks, const uint32_t *roff, uint32_t *rcur, uint32_t *rev) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t t = g / KEEP, i = g % KEEP;
  if (t >= ntasks || i >= cnt[t]) return;
  const uint32_t tu = cv_task_of(nn[(size_t)t * KEEP + i], t_level[t], n, upb);
  rev[roff[tu] + atomicAdd(&rcur[tu], 1u)] = t_node[t];
}
__global__ void cv_rev_count_kernel(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_level, const uint32_t *upb, uint32_t n,
                                    uint32_t ntasks, uint32_t *rcnt) {
  cv_rev_count_slot<32>(nn, cnt, t_level, upb, n, ntasks, rcnt);
}
__global__ void cv_rev_count_kernel_wide(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_level, const uint32_t *upb, uint32_t n,
                                         uint32_t ntasks, uint32_t *rcnt) {
  cv_rev_count_slot<kCvMaxKeep>(nn, cnt, t_level, upb, n, ntasks, rcnt);
}
__global__ void cv_rev_fill_kernel(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_node, const uint32_t *t_level, const uint32_t *upb,
                                   uint32_t n, uint32_t ntasks, const uint32_t *roff, uint32_t *rcur, uint32_t *rev) {
  cv_rev_fill_slot<32>(nn, cnt, t_node, t_level, upb, n, ntasks, roff, rcur, rev);
}
__global__ void cv_rev_fill_kernel_wide(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_node, const uint32_t *t_level, const uint32_t *upb,
                                        uint32_t n, uint32_t ntasks, const uint32_t *roff, uint32_t *rcur, uint32_t *rev) {
  cv_rev_fill_slot<kCvMaxKeep>(nn, cnt, t_node, t_level, upb, n, ntasks, roff, rcur, rev);
}

hipError_t launch_cv_rev_count(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_level, const uint32_t *upb, uint32_t n, uint32_t ntasks,
                               uint32_t keep, uint32_t *rcnt) {
  const dim3 grid((uint32_t)(((size_t)ntasks * keep + 255) / 256));
  if (keep == 32) hipLaunchKernelGGL(cv_rev_count_kernel, grid, dim3(256), 0, nullptr, nn, cnt, t_level, upb, n, ntasks, rcnt);
  else hipLaunchKernelGGL(cv_rev_count_kernel_wide, grid, dim3(256), 0, nullptr, nn, cnt, t_level, upb, n, ntasks, rcnt);
  return hipGetLastError();
}
hipError_t launch_cv_rev_fill(const uint32_t *nn, const uint32_t *cnt, const uint32_t *t_node, const uint32_t *t_level, const uint32_t *upb, uint32_t n,
                              uint32_t ntasks, uint32_t keep, const uint32_t *roff, uint32_t *rcur, uint32_t *rev) {
  const dim3 grid((uint32_t)(((size_t)ntasks * keep + 255) / 256));
  if (keep == 32) hipLaunchKernelGGL(cv_rev_fill_kernel, grid, dim3(256), 0, nullptr, nn, cnt, t_node, t_level, upb, n, ntasks, roff, rcur, rev);
  else hipLaunchKernelGGL(cv_rev_fill_kernel_wide, grid, dim3(256), 0, nullptr, nn, cnt, t_node, t_level, upb, n, ntasks, roff, rcur, rev);
  return hipGetLastError();
}

// ---- phase 3 (hnswalg_slim.h:999-1012, 1038-1062): own list + reverse edges, sorted by id, duplicates removed; a list over
//      its level's capacity is sorted by distance and pruned again ---------------------------------------------------------------
template <int METRIC, uint32_t KEEP>
__device__ __forceinline__ void cv_union_tasks(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_limit,
                                               const uint32_t *nn, const uint32_t *cnt, const uint32_t *roff, const uint32_t *rcnt,
                                               const uint32_t *rev, uint32_t ntasks, uint32_t *fin, uint32_t *fin_cnt, uint32_t *flags) {
  constexpr uint32_t keep = KEEP;
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  float *qc = qv + dim;
  uint32_t *ids = reinterpret_cast<uint32_t *>(qc + dim);
  float *nd = reinterpret_cast<float *>(ids + kCvUnionCap);
  Pair *arr = reinterpret_cast<Pair *>(nd + kCvUnionCap);
  uint32_t *kept = reinterpret_cast<uint32_t *>(arr + kCvUnionCap);
  float *kd = reinterpret_cast<float *>(kept + keep);
  const int lane = threadIdx.x;
  for (uint32_t t = blockIdx.x; t < ntasks; t += gridDim.x) {
    const uint32_t m1 = cnt[t], r = rcnt[t], total = m1 + r, limit = t_limit[t];
    wave_sync();
    if (total > kCvUnionCap) {   // does not fit the on-chip buffers: the host redoes the conversion on the CPU
      if (lane == 0) { atomicAdd(flags, 1u); fin_cnt[t] = 0; }
      continue;
    }
    const uint32_t m = cv_union_ids(nn + (size_t)t * keep, m1, rev + roff[t], total, ids, lane);
    if (m <= limit) {
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
    cv_sort_by_dist(ids, nd, m, arr, lane);
    const uint32_t kc = cv_prune<METRIC>(vec, dim, arr, m, min(limit, keep), qc, kept, kd, lane);
    if ((uint32_t)lane < kc) fin[(size_t)t * keep + lane] = kept[lane];
    if (lane == 0) fin_cnt[t] = kc;
  }
}
template <int METRIC>
__global__ void __launch_bounds__(64) cv_union_kernel(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_limit,
                                                      const uint32_t *nn, const uint32_t *cnt, const uint32_t *roff, const uint32_t *rcnt,
                                                      const uint32_t *rev, uint32_t ntasks, uint32_t *fin, uint32_t *fin_cnt, uint32_t *flags) {
  cv_union_tasks<METRIC, 32>(vec, dim, t_node, t_limit, nn, cnt, roff, rcnt, rev, ntasks, fin, fin_cnt, flags);
}
template <int METRIC>
__global__ void __launch_bounds__(64) cv_union_kernel_wide(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_limit,
                                                           const uint32_t *nn, const uint32_t *cnt, const uint32_t *roff, const uint32_t *rcnt,
                                                           const uint32_t *rev, uint32_t ntasks, uint32_t *fin, uint32_t *fin_cnt, uint32_t *flags) {
  cv_union_tasks<METRIC, kCvMaxKeep>(vec, dim, t_node, t_limit, nn, cnt, roff, rcnt, rev, ntasks, fin, fin_cnt, flags);
}

// ---- host driver ----------------------------------------------------------------------------------------------------------
#define CV_TRY(expr)                        \
  do {                                      \
    hipError_t _e = (expr);                 \
    if (_e != hipSuccess) { err = _e; goto done; } \
  } while (0)

template <typename T>
static hipError_t cv_upload(T **dp, const std::vector<T> &v) {
  hipError_t e = hipMalloc((void **)dp, std::max<size_t>(v.size(), 1) * sizeof(T));
  if (e != hipSuccess) return e;
  return v.empty() ? hipSuccess : hipMemcpy(*dp, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// The three phases with the given phase-1 and phase-3 kernels (this file's, or convert_slimq.hip's) and their LDS bytes
hipError_t cv_run_lists(const ConvertInput &in, int device, CvPruneKernel prune_k, CvUnionKernel union_k, size_t lds1, size_t lds3,
                        std::vector<uint32_t> &fin, std::vector<uint32_t> &fin_cnt, bool &needs_host, double *kernel_ms) {
  hipError_t err = hipSuccess;
  needs_host = false;
  const uint32_t nt = (uint32_t)in.t_node.size();
  float *d_vec = nullptr;
  uint32_t *d_node = nullptr, *d_off = nullptr, *d_size = nullptr, *d_mlim = nullptr, *d_limit = nullptr, *d_level = nullptr, *d_lists = nullptr,
           *d_upb = nullptr, *d_nn = nullptr, *d_cnt = nullptr, *d_rcnt = nullptr, *d_roff = nullptr, *d_rcur = nullptr, *d_rev = nullptr,
           *d_fin = nullptr, *d_fcnt = nullptr, *d_flags = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<uint32_t> rcnt(nt), roff(nt + 1, 0);
  uint32_t flags = 0;
  const uint32_t keep = in.keep;   // slots per task of nn / fin, entries of kept / kd in LDS
  const uint32_t grid = 256 * 16;
  if (nt == 0) return hipSuccess;
  if (keep != 32 && keep != kCvMaxKeep) return hipErrorInvalidValue;
  CV_TRY(hipSetDevice(device));
  CV_TRY(hipMalloc((void **)&d_vec, (size_t)in.n * in.dim * 4));
  CV_TRY(hipMemcpy(d_vec, in.vec, (size_t)in.n * in.dim * 4, hipMemcpyHostToDevice));
  CV_TRY(cv_upload(&d_node, in.t_node)); CV_TRY(cv_upload(&d_off, in.t_off)); CV_TRY(cv_upload(&d_size, in.t_size));
  CV_TRY(cv_upload(&d_mlim, in.t_mlim)); CV_TRY(cv_upload(&d_limit, in.t_limit)); CV_TRY(cv_upload(&d_level, in.t_level));
  CV_TRY(cv_upload(&d_lists, in.lists)); CV_TRY(cv_upload(&d_upb, in.upb));
  CV_TRY(hipMalloc((void **)&d_nn, (size_t)nt * keep * 4)); CV_TRY(hipMalloc((void **)&d_cnt, (size_t)nt * 4));
  CV_TRY(hipMalloc((void **)&d_rcnt, (size_t)nt * 4)); CV_TRY(hipMalloc((void **)&d_roff, (size_t)(nt + 1) * 4)); CV_TRY(hipMalloc((void **)&d_rcur, (size_t)nt * 4));
  CV_TRY(hipMalloc((void **)&d_fin, (size_t)nt * keep * 4)); CV_TRY(hipMalloc((void **)&d_fcnt, (size_t)nt * 4)); CV_TRY(hipMalloc((void **)&d_flags, 4));
  CV_TRY(hipMemset(d_rcnt, 0, (size_t)nt * 4)); CV_TRY(hipMemset(d_rcur, 0, (size_t)nt * 4)); CV_TRY(hipMemset(d_flags, 0, 4));
  CV_TRY(hipEventCreate(&e0)); CV_TRY(hipEventCreate(&e1));
  if (lds3 > 64 * 1024) CV_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(union_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
  CV_TRY(hipEventRecord(e0, nullptr));
  hipLaunchKernelGGL(prune_k, dim3(std::min(grid, nt)), dim3(64), lds1, nullptr, d_vec, in.dim, d_node, d_off, d_size, d_mlim, d_lists, nt, d_nn, d_cnt);
  CV_TRY(hipGetLastError());
  CV_TRY(launch_cv_rev_count(d_nn, d_cnt, d_level, d_upb, in.n, nt, keep, d_rcnt));
  CV_TRY(hipMemcpy(rcnt.data(), d_rcnt, (size_t)nt * 4, hipMemcpyDeviceToHost));
  for (uint32_t t = 0; t < nt; t++) roff[t + 1] = roff[t] + rcnt[t];
  CV_TRY(hipMemcpy(d_roff, roff.data(), (size_t)(nt + 1) * 4, hipMemcpyHostToDevice));
  CV_TRY(hipMalloc((void **)&d_rev, std::max<size_t>(roff[nt], 1) * 4));
  CV_TRY(launch_cv_rev_fill(d_nn, d_cnt, d_node, d_level, d_upb, in.n, nt, keep, d_roff, d_rcur, d_rev));
  hipLaunchKernelGGL(union_k, dim3(std::min(grid, nt)), dim3(64), lds3, nullptr, d_vec, in.dim, d_node, d_limit, d_nn, d_cnt, d_roff, d_rcnt, d_rev, nt, d_fin, d_fcnt, d_flags);
  CV_TRY(hipGetLastError());
  CV_TRY(hipEventRecord(e1, nullptr));
  CV_TRY(hipEventSynchronize(e1));
  if (kernel_ms) { float ms = 0.f; CV_TRY(hipEventElapsedTime(&ms, e0, e1)); *kernel_ms = ms; }
  CV_TRY(hipMemcpy(&flags, d_flags, 4, hipMemcpyDeviceToHost));
  needs_host = flags != 0;
  fin.resize((size_t)nt * keep);
  fin_cnt.resize(nt);
  CV_TRY(hipMemcpy(fin.data(), d_fin, fin.size() * 4, hipMemcpyDeviceToHost));
  CV_TRY(hipMemcpy(fin_cnt.data(), d_fcnt, (size_t)nt * 4, hipMemcpyDeviceToHost));
done:
  for (void *p : {(void *)d_vec, (void *)d_node, (void *)d_off, (void *)d_size, (void *)d_mlim, (void *)d_limit, (void *)d_level, (void *)d_lists, (void *)d_upb,
                  (void *)d_nn, (void *)d_cnt, (void *)d_rcnt, (void *)d_roff, (void *)d_rcur, (void *)d_rev, (void *)d_fin, (void *)d_fcnt, (void *)d_flags})
    if (p) (void)hipFree(p);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return err;
}

hipError_t gpu_convert_lists(const ConvertInput &in, int device, std::vector<uint32_t> &fin, std::vector<uint32_t> &fin_cnt, bool &needs_host,
                             double *kernel_ms) {
  const uint32_t keep = in.keep;
  const size_t lds1 = (size_t)in.dim * 8 + kCvMaxList * 16 + keep * 8;
  const size_t lds3 = (size_t)in.dim * 8 + (size_t)kCvUnionCap * 16 + keep * 8;
  const bool l2 = in.metric == METRIC_L2, wide = keep != 32;
  const CvPruneKernel prune_k = wide ? (l2 ? cv_prune_kernel_wide<METRIC_L2> : cv_prune_kernel_wide<METRIC_IP>) : (l2 ? cv_prune_kernel<METRIC_L2> : cv_prune_kernel<METRIC_IP>);
  const CvUnionKernel union_k = wide ? (l2 ? cv_union_kernel_wide<METRIC_L2> : cv_union_kernel_wide<METRIC_IP>) : (l2 ? cv_union_kernel<METRIC_L2> : cv_union_kernel<METRIC_IP>);
  return cv_run_lists(in, device, prune_k, union_k, lds1, lds3, fin, fin_cnt, needs_host, kernel_ms);
}

}  // namespace hs
