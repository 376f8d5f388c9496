// convert_slimq.hip -- HierarchicalNSWSlimQ::convertFromHNSW on gfx950 (hnswalg_slimq.h:1471-1790): the graph passes and the
// RaBitQ records, the two steps between the base graph (build_gpu.hip) and a searchable SlimQ index.  DESIGN.md 4p.
//   * Graph passes (:1546-1762): the three phases of convert_gpu.hip, one wavefront per (node, level) task over the same
//     ConvertInput, the same by-distance sort (cv_sort_by_dist), the same reverse-edge kernels and host driver (cv_run_lists).
//     Two things differ: every distance is rabitqlib's raw distance (rq_dist.hpp: sixteen lanes per row), and the prune is
//     SlimQ's own PruneByHeuristic (:1334-1362) in its closed form (slimq_prune.hpp), a chunk of candidates per round.
//   * Records (:1764-1786, one_bit_code_with_factor rabitq_impl.hpp:75-138): one wavefront per row rotates it in LDS
//     (rabitq_rotate.hpp), picks its cluster, and runs rq_quantize_data (rabitq_host.hpp) -- five strict left-to-right fp32 chains,
//     one per lane, the sign code from ballots, the factors with the host's expressions -- bit for bit the host's output.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "convert_common.hpp"
#include "convert_engine.hpp"
#include "rabitq_rotate.hpp"
#include "rq_dist.hpp"
#include "slimq_prune.hpp"

namespace hs {

// prune_slimq (host_rq_graph.hpp) over arr[0..sz) sorted ascending by distance, into kept[0..return): slimq_prune.hpp's closed form.
// Round by round: the pair distances d(row i, row id_i) of kSlimqPruneChunk candidates, a ballot of the survivors, their slots by
// prefix count; it stops measuring once mlim entries are kept.  mlim == 0 keeps nothing.  pd: kSlimqPruneChunk floats of LDS.
// Premise (slimq_prune.hpp): sz <= n, so that row i exists for every i < sz -- checked by the host for the source lists
// (cq_input_ok), true of a union because its entries are distinct ids below n.
template <int METRIC>
__device__ __forceinline__ uint32_t cq_prune(const float *vec, uint32_t dim, const Pair *arr, uint32_t sz, uint32_t mlim, uint32_t *kept, float *pd,
                                             int lane) {
  uint32_t kc = 0;
  for (uint32_t base = 0; base < sz && kc < mlim; base += kSlimqPruneChunk) {
    const uint32_t cnt = min(kSlimqPruneChunk, sz - base);
    rq_pair_dists<METRIC>(vec, dim, base, arr + base, pd, cnt, lane);
    wave_sync();
    const bool act = (uint32_t)lane < cnt;
    const Pair c = arr[act ? base + lane : base];
    const bool good = act && slimq_keeps(base + lane, pd[act ? lane : 0], c.d);
    const unsigned long long gm = hs_ballot(good);
    const uint32_t slot = slimq_slot(gm, (uint32_t)lane, kc);
    if (good && slot < mlim) kept[slot] = c.id;
    kc = slimq_kept_after(gm, kc, mlim);
    wave_sync();
  }
  return kc;
}

// LDS of the two list kernels: the node's row, then per list entry an id, a distance and a sorted pair, the kept list, a chunk of
// pair distances
static size_t cq_lds(uint32_t dim, uint32_t entries, uint32_t keep) { return (size_t)dim * 4 + (size_t)entries * 16 + keep * 4 + kSlimqPruneChunk * 4; }

// ---- phase 1 (hnswalg_slimq.h:1600-1640): every source list sorted by raw distance to its node and pruned to its degree budget ----
template <int METRIC, uint32_t KEEP>
__device__ __forceinline__ void cq_prune_tasks(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_off, const uint32_t *t_size,
                                               const uint32_t *t_mlim, const uint32_t *lists, uint32_t ntasks, uint32_t *out_nn, uint32_t *out_cnt) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  uint32_t *nid = reinterpret_cast<uint32_t *>(qv + dim);
  float *nd = reinterpret_cast<float *>(nid + kCvMaxList);
  Pair *arr = reinterpret_cast<Pair *>(nd + kCvMaxList);
  uint32_t *kept = reinterpret_cast<uint32_t *>(arr + kCvMaxList);
  float *pd = reinterpret_cast<float *>(kept + KEEP);
  const int lane = threadIdx.x;
  for (uint32_t t = blockIdx.x; t < ntasks; t += gridDim.x) {
    const uint32_t v = t_node[t], sz = t_size[t], mlim = t_mlim[t];   // sz <= kCvMaxList, mlim <= KEEP (host checks)
    wave_sync();
    for (uint32_t i = lane; i < dim; i += 64) qv[i] = vec[(size_t)v * dim + i];
    if ((uint32_t)lane < sz) nid[lane] = lists[t_off[t] + lane];
    wave_sync();
    rq_dists<METRIC>(vec, dim, qv, nid, nd, sz, lane);
    wave_sync();
    cv_sort_by_dist(nid, nd, sz, arr, lane);
    const uint32_t kc = cq_prune<METRIC>(vec, dim, arr, sz, mlim, kept, pd, lane);
    if ((uint32_t)lane < kc) out_nn[(size_t)t * KEEP + lane] = kept[lane];   // kc <= mlim <= KEEP <= 64: one lane per kept entry
    if (lane == 0) out_cnt[t] = kc;
  }
}
template <int METRIC>
__global__ void __launch_bounds__(64) cq_prune_kernel(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_off,
                                                      const uint32_t *t_size, const uint32_t *t_mlim, const uint32_t *lists, uint32_t ntasks,
                                                      uint32_t *out_nn, uint32_t *out_cnt) {
  cq_prune_tasks<METRIC, 32>(vec, dim, t_node, t_off, t_size, t_mlim, lists, ntasks, out_nn, out_cnt);
}
template <int METRIC>
__global__ void __launch_bounds__(64) cq_prune_kernel_wide(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_off,
                                                           const uint32_t *t_size, const uint32_t *t_mlim, const uint32_t *lists, uint32_t ntasks,
                                                           uint32_t *out_nn, uint32_t *out_cnt) {
  cq_prune_tasks<METRIC, kCvMaxKeep>(vec, dim, t_node, t_off, t_size, t_mlim, lists, ntasks, out_nn, out_cnt);
}

// ---- phase 3 (hnswalg_slimq.h:1660-1740): own list + reverse edges, sorted by id, duplicates removed; a list over its level's
//      capacity is sorted by raw distance and pruned again ----
template <int METRIC, uint32_t KEEP>
__device__ __forceinline__ void cq_union_tasks(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_limit, const uint32_t *nn,
                                               const uint32_t *cnt, const uint32_t *roff, const uint32_t *rcnt, const uint32_t *rev, uint32_t ntasks,
                                               uint32_t *fin, uint32_t *fin_cnt, uint32_t *flags) {
  constexpr uint32_t keep = KEEP;
  extern __shared__ __align__(16) unsigned char smem[];
  float *qv = reinterpret_cast<float *>(smem);
  uint32_t *ids = reinterpret_cast<uint32_t *>(qv + dim);
  float *nd = reinterpret_cast<float *>(ids + kCvUnionCap);
  Pair *arr = reinterpret_cast<Pair *>(nd + kCvUnionCap);
  uint32_t *kept = reinterpret_cast<uint32_t *>(arr + kCvUnionCap);
  float *pd = reinterpret_cast<float *>(kept + keep);
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
    rq_dists<METRIC>(vec, dim, qv, ids, nd, m, lane);
    wave_sync();
    cv_sort_by_dist(ids, nd, m, arr, lane);
    // (m distinct ids below n: m <= n, cq_prune's premise)
    const uint32_t kc = cq_prune<METRIC>(vec, dim, arr, m, min(limit, keep), kept, pd, lane);
    if ((uint32_t)lane < kc) fin[(size_t)t * keep + lane] = kept[lane];
    if (lane == 0) fin_cnt[t] = kc;
  }
}
template <int METRIC>
__global__ void __launch_bounds__(64) cq_union_kernel(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_limit,
                                                      const uint32_t *nn, const uint32_t *cnt, const uint32_t *roff, const uint32_t *rcnt,
                                                      const uint32_t *rev, uint32_t ntasks, uint32_t *fin, uint32_t *fin_cnt, uint32_t *flags) {
  cq_union_tasks<METRIC, 32>(vec, dim, t_node, t_limit, nn, cnt, roff, rcnt, rev, ntasks, fin, fin_cnt, flags);
}
template <int METRIC>
__global__ void __launch_bounds__(64) cq_union_kernel_wide(const float *vec, uint32_t dim, const uint32_t *t_node, const uint32_t *t_limit,
                                                           const uint32_t *nn, const uint32_t *cnt, const uint32_t *roff, const uint32_t *rcnt,
                                                           const uint32_t *rev, uint32_t ntasks, uint32_t *fin, uint32_t *fin_cnt, uint32_t *flags) {
  cq_union_tasks<METRIC, kCvMaxKeep>(vec, dim, t_node, t_limit, nn, cnt, roff, rcnt, rev, ntasks, fin, fin_cnt, flags);
}

bool gpu_convert_slimq_fits(uint32_t dim) { return cq_lds(dim, kCvUnionCap, kCvMaxKeep) <= 64 * 1024; }

hipError_t gpu_convert_slimq_lists(const ConvertInput &in, int device, std::vector<uint32_t> &fin, std::vector<uint32_t> &fin_cnt, bool &needs_host,
                                   double *kernel_ms) {
  if (!gpu_convert_slimq_fits(in.dim)) return hipErrorInvalidValue;
  const bool l2 = in.metric == METRIC_L2, wide = in.keep != 32;
  const CvPruneKernel prune_k = wide ? (l2 ? cq_prune_kernel_wide<METRIC_L2> : cq_prune_kernel_wide<METRIC_IP>) : (l2 ? cq_prune_kernel<METRIC_L2> : cq_prune_kernel<METRIC_IP>);
  const CvUnionKernel union_k = wide ? (l2 ? cq_union_kernel_wide<METRIC_L2> : cq_union_kernel_wide<METRIC_IP>) : (l2 ? cq_union_kernel<METRIC_L2> : cq_union_kernel<METRIC_IP>);
  return cv_run_lists(in, device, prune_k, union_k, cq_lds(in.dim, kCvMaxList, in.keep), cq_lds(in.dim, kCvUnionCap, in.keep), fin, fin_cnt, needs_host,
                      kernel_ms);
}

// ---- RaBitQ records ---------------------------------------------------------------------------------------------------------
struct RqQuantDev {
  DevSlimQ sq;            // padded, trunc, fht_scale, flips, ncl; cent = the ROTATED centroids (ncl x padded)
  const float *rows;      // row r at rows + r * row_stride, dim floats
  size_t row_stride;
  uint32_t dim, n;
  const float *cent_raw;  // ncl x dim
  const uint32_t *cluster_in;   // nullable: n cluster ids, each below ncl (the caller checked)
  float *out_rot;         // nullable: n x padded
  uint32_t *out_cluster;  // n
  uint64_t *out_code;     // n x padded/64
  float *out_fac;         // n x 3
};

// rows (zero-padded to `padded`) -> their rotation; the centroids go through it once, before the rows
__global__ void __launch_bounds__(64) rq_rotate_kernel(DevSlimQ sq, uint32_t dim, const float *in, uint32_t n, float *out) {
  extern __shared__ __align__(16) unsigned char smem[];
  float *y = reinterpret_cast<float *>(smem);
  const int lane = threadIdx.x;
  const uint32_t P = sq.padded;
  for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
    wave_sync();
    for (uint32_t i = lane; i < P; i += 64) y[i] = i < dim ? in[(size_t)r * dim + i] : 0.f;
    rotate_lds(sq, y, lane);
    for (uint32_t i = lane; i < P; i += 64) out[(size_t)r * P + i] = y[i];
  }
}

// One wavefront per row.  Every fp32 reduction is a strict left-to-right chain of rounded multiply then rounded add on ONE lane
// (the definition rabitq_host.hpp documents; the build has -ffp-contract=off); sqrtf and / are the correctly rounded ones (plain
// operators under hipcc's default, see the note in slimq_prep_kernel).
template <int METRIC>
__global__ void __launch_bounds__(64) rq_quantize_kernel(RqQuantDev a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const uint32_t P = a.sq.padded, dim = a.dim, ncl = a.sq.ncl;
  float *y = reinterpret_cast<float *>(smem);   // the row: raw and zero-padded, then rotated
  float *cl = y + P;                            // the rotated centroid of its cluster
  float *red = cl + P;                          // the five sums
  for (uint32_t r = blockIdx.x; r < a.n; r += gridDim.x) {
    wave_sync();
    const float *row = a.rows + (size_t)r * a.row_stride;
    for (uint32_t i = lane; i < P; i += 64) y[i] = i < dim ? row[i] : 0.f;
    wave_sync();
    uint32_t cid = 0;
    if (a.cluster_in) {
      cid = uni(a.cluster_in[r]);
    } else {
      // nearest RAW centroid by rq_l2sqr, one centroid per lane, rounds of 64; `dd < best` from FLT_MAX: the first minimum wins
      float best = FLT_MAX;
      for (uint32_t c0 = 0; c0 < ncl; c0 += 64) {
        const uint32_t c = c0 + lane;
        const bool live = c < ncl;
        const float *ce = a.cent_raw + (size_t)(live ? c : 0) * dim;
        float s = 0.f;
        for (uint32_t k = 0; k < dim; k++) {
          const float t = y[k] - ce[k];
          s += t * t;
        }
        const float v = (live && s < FLT_MAX) ? s : INFINITY;
        const float m = wave_min_f32<true>(v);
        if (m < best) {
          best = m;
          cid = c0 + (uint32_t)__ffsll((long long)hs_ballot(v == m)) - 1u;
        }
      }
    }
    rotate_lds(a.sq, y, lane);
    const float *ce = a.sq.cent + (size_t)cid * P;
    for (uint32_t i = lane; i < P; i += 64) {
      cl[i] = ce[i];
      if (a.out_rot) a.out_rot[(size_t)r * P + i] = y[i];
    }
    wave_sync();
    // sign code (pack_binary): 64 dimensions per ballot, dimension i -> bit 63 - i % 64
    for (uint32_t b = 0; b < P / 64; b++) {
      const float res = y[b * 64 + lane] - cl[b * 64 + lane];
      const unsigned long long m = hs_ballot(res > 0.f);
      if (lane == 0) a.out_code[(size_t)r * (P / 64) + b] = __brevll(m);
    }
    {  // l2_sqr, ip_resi, ip_cent, l2_xucb, ip_resi_cent on lanes 0..4, one loop (the lanes above repeat lane 4)
      float s = 0.f;
      for (uint32_t i = 0; i < P; i += 4) {
        const float4 yv = *reinterpret_cast<const float4 *>(y + i), cv = *reinterpret_cast<const float4 *>(cl + i);
        const float ys[4] = {yv.x, yv.y, yv.z, yv.w}, cs[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float c = cs[j], rr = ys[j] - c;
          const float xu = (rr > 0.f ? 1.f : 0.f) + (-0.5f);
          const float p = lane == 2 ? c : (lane == 3 ? xu : rr);
          const float q = lane == 0 ? rr : (lane >= 4 ? c : xu);
          s += p * q;
        }
      }
      if (lane < 5) red[lane] = s;
    }
    wave_sync();
    {  // rq_quantize_data's factor arithmetic, expression for expression
      constexpr float kConstEpsilon = 1.9f;
      const float l2_sqr = red[0], ip_cent = red[2], l2_xucb = red[3], ip_resi_cent = red[4];
      float ip_resi = red[1];
      const float l2_norm = __builtin_sqrtf(l2_sqr);
      if (ip_resi == 0) ip_resi = INFINITY;
      const float tmp_error = l2_norm * kConstEpsilon * __builtin_sqrtf((((l2_sqr * l2_xucb) / (ip_resi * ip_resi)) - 1) / (float)(P - 1));
      float f0, f1, f2;
      if (METRIC == METRIC_L2) {
        f0 = l2_sqr + 2 * l2_sqr * ip_cent / ip_resi;
        f1 = -2 * l2_sqr / ip_resi;
        f2 = 2 * tmp_error;
      } else {
        f0 = 1 - ip_resi_cent + l2_sqr * ip_cent / ip_resi;
        f1 = -l2_sqr / ip_resi;
        f2 = 1 * tmp_error;
      }
      if (lane == 0) {
        a.out_cluster[r] = cid;
        a.out_fac[(size_t)r * 3] = f0; a.out_fac[(size_t)r * 3 + 1] = f1; a.out_fac[(size_t)r * 3 + 2] = f2;
      }
    }
  }
}

#define CQ_TRY(expr)                        \
  do {                                      \
    hipError_t _e = (expr);                 \
    if (_e != hipSuccess) { err = _e; goto done; } \
  } while (0)

hipError_t gpu_rq_quantize(const RqQuantInput &in, int device, float *out_cent_rot, float *out_rot, uint32_t *out_cluster, uint64_t *out_code,
                           float *out_fac, double *kernel_ms) {
  hipError_t err = hipSuccess;
  const uint32_t dim = (uint32_t)in.dim, P = (dim + 63) / 64 * 64, ncl = (uint32_t)in.ncl;
  uint32_t lg = 0;
  while ((2u << lg) <= dim) lg++;
  // rows in flight at once: at most kRqChunkBytes of them, so that n x dim x 4 bytes need not be resident
  const size_t chunk = std::max<size_t>(1, std::min<size_t>(in.n, kRqChunkBytes / (in.row_stride * 4)));
  const size_t chunk_floats = in.n ? (chunk - 1) * in.row_stride + dim : 0;   // (the last row of a chunk ends after dim floats)
  const size_t lds = (size_t)P * 8 + 32;
  const uint32_t max_grid = 256 * 16;
  uint8_t *d_flips = nullptr;
  float *d_craw = nullptr, *d_crot = nullptr, *d_rows = nullptr, *d_rot = nullptr, *d_fac = nullptr;
  uint32_t *d_cin = nullptr, *d_cluster = nullptr;
  uint64_t *d_code = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double ms_sum = 0.0;
  RqQuantDev a{};
  CQ_TRY(hipSetDevice(device));
  CQ_TRY(hipMalloc((void **)&d_flips, 4 * P / 8)); CQ_TRY(hipMemcpy(d_flips, in.flips, 4 * P / 8, hipMemcpyHostToDevice));
  CQ_TRY(hipMalloc((void **)&d_craw, (size_t)ncl * dim * 4)); CQ_TRY(hipMemcpy(d_craw, in.cent_raw, (size_t)ncl * dim * 4, hipMemcpyHostToDevice));
  CQ_TRY(hipMalloc((void **)&d_crot, (size_t)ncl * P * 4));
  CQ_TRY(hipMalloc((void **)&d_rows, std::max<size_t>(chunk_floats, 1) * 4));
  if (out_rot) CQ_TRY(hipMalloc((void **)&d_rot, chunk * P * 4));
  if (in.cluster_ids) CQ_TRY(hipMalloc((void **)&d_cin, chunk * 4));
  CQ_TRY(hipMalloc((void **)&d_cluster, chunk * 4)); CQ_TRY(hipMalloc((void **)&d_code, chunk * (P / 64) * 8)); CQ_TRY(hipMalloc((void **)&d_fac, chunk * 12));
  CQ_TRY(hipEventCreate(&e0)); CQ_TRY(hipEventCreate(&e1));
  a.sq.padded = P; a.sq.trunc = 1u << lg; a.sq.fht_scale = 1.0f / std::sqrt((float)a.sq.trunc); a.sq.flips = d_flips; a.sq.ncl = ncl; a.sq.cent = d_crot;
  a.rows = d_rows; a.row_stride = in.row_stride; a.dim = dim; a.cent_raw = d_craw; a.cluster_in = d_cin;
  a.out_rot = d_rot; a.out_cluster = d_cluster; a.out_code = d_code; a.out_fac = d_fac;
  CQ_TRY(hipEventRecord(e0, nullptr));
  hipLaunchKernelGGL(rq_rotate_kernel, dim3(std::min(max_grid, ncl)), dim3(64), (size_t)P * 4, nullptr, a.sq, dim, d_craw, ncl, d_crot);
  CQ_TRY(hipGetLastError());
  CQ_TRY(hipEventRecord(e1, nullptr));
  CQ_TRY(hipMemcpy(out_cent_rot, d_crot, (size_t)ncl * P * 4, hipMemcpyDeviceToHost));
  { float ms = 0.f; CQ_TRY(hipEventElapsedTime(&ms, e0, e1)); ms_sum += ms; }
  for (size_t first = 0; first < in.n; first += chunk) {
    const size_t cnt = std::min(chunk, in.n - first);
    CQ_TRY(hipMemcpy(d_rows, in.rows + first * in.row_stride, ((cnt - 1) * in.row_stride + dim) * 4, hipMemcpyHostToDevice));
    if (d_cin) CQ_TRY(hipMemcpy(d_cin, in.cluster_ids + first, cnt * 4, hipMemcpyHostToDevice));
    a.n = (uint32_t)cnt;
    CQ_TRY(hipEventRecord(e0, nullptr));
    if (in.metric == METRIC_L2) hipLaunchKernelGGL(rq_quantize_kernel<METRIC_L2>, dim3(std::min<uint32_t>(max_grid, a.n)), dim3(64), lds, nullptr, a);
    else hipLaunchKernelGGL(rq_quantize_kernel<METRIC_IP>, dim3(std::min<uint32_t>(max_grid, a.n)), dim3(64), lds, nullptr, a);
    CQ_TRY(hipGetLastError());
    CQ_TRY(hipEventRecord(e1, nullptr));
    CQ_TRY(hipMemcpy(out_cluster + first, d_cluster, cnt * 4, hipMemcpyDeviceToHost));
    CQ_TRY(hipMemcpy(out_code + first * (P / 64), d_code, cnt * (P / 64) * 8, hipMemcpyDeviceToHost));
    CQ_TRY(hipMemcpy(out_fac + first * 3, d_fac, cnt * 12, hipMemcpyDeviceToHost));
    if (out_rot) CQ_TRY(hipMemcpy(out_rot + first * P, d_rot, cnt * P * 4, hipMemcpyDeviceToHost));
    { float ms = 0.f; CQ_TRY(hipEventElapsedTime(&ms, e0, e1)); ms_sum += ms; }
  }
  if (kernel_ms) *kernel_ms = ms_sum;
done:
  for (void *p : {(void *)d_flips, (void *)d_craw, (void *)d_crot, (void *)d_rows, (void *)d_rot, (void *)d_cin, (void *)d_cluster, (void *)d_code, (void *)d_fac})
    if (p) (void)hipFree(p);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return err;
}

}  // namespace hs
